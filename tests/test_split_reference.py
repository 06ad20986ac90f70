"""Host half of DESIGN 4.6: the split-format models (split_models.py) and the exact nets (split_nets.py).

No GPU: the quantisers against their own decode tables, the models against ref64 on seeded random nets, the exactness
and coverage conditions of every exact net the device test runs, and the named faults."""
import importlib

import numpy as np
import pytest

import ref64
import split_models as sm
import split_nets as sn

from test_gpu_plan_sweep import TOL

SHAPES = sn.TIER_B  # Tier B: (channels, blocks); Tier A runs two blocks everywhere


@pytest.mark.parametrize("enc,dec,table,sign,top", [(sm.e2m3_encode, sm.e2m3_decode, sm.E2M3, 0x20, 7.5),
                                                     (sm.e4m3_encode, sm.e4m3_decode, sm.E4M3, 0x80, 448.0)],
                         ids=["e2m3", "e4m3"])
def test_quantiser_tables(enc, dec, table, sign, top):
    codes = np.arange(2 * sign, dtype=np.uint8)
    vals = dec(codes)
    finite = np.isfinite(vals)
    assert finite.sum() == (64 if sign == 0x20 else 254)
    assert (enc(vals[finite]) == codes[finite]).all(), "a code does not decode and re-encode to itself"
    assert (enc(vals[~finite]) & (sign - 1) == (sign - 1)).all()
    mags = table[np.isfinite(table)]
    assert (np.diff(mags) > 0).all() and mags[-1] == top
    for c in range(len(mags) - 1):  # every midpoint goes to the even code, either side of it to the nearer code
        mid = (mags[c] + mags[c + 1]) / 2
        even = c if c % 2 == 0 else c + 1
        for s, bit in ((1.0, 0), (-1.0, sign)):
            assert enc(s * mid) == (even | bit), (c, mid)
            assert enc(s * np.nextafter(mid, 0)) == (c | bit) and enc(s * np.nextafter(mid, np.inf)) == ((c + 1) | bit)
    for v in (top, np.nextafter(top, np.inf), top * 1.03, top * 1.04, 2 * top, 1e30, np.inf):
        assert enc(v) == len(mags) - 1 and enc(-v) == ((len(mags) - 1) | sign), v
    assert enc(0.0) == 0 and enc(-0.0) == sign


def test_e8m0_rules():
    blk = np.zeros((4, 32))
    blk[1, 3] = 2.0 ** -20      # f16 subnormal
    blk[2, 5] = 5.0             # f16 exponent field 17
    blk[3, 0] = -0.75
    assert sm.e8m0_activations(sm.f16(blk)).ravel().tolist() == [110, 110, 127, 124]
    assert sm.e8m0_weights(blk).ravel().tolist() == [0, 127 - 22, 127, 127 - 3]
    assert (sm.mx6(blk, sm.e8m0_weights(blk)) == blk).all()
    assert sm.mx6(np.full((1, 32), 3.0), np.array([[0]])).max() == 0.0  # byte 0: codes 0


@pytest.mark.parametrize("F,boards", [(64, 4), (256, 2)])
def test_models_against_float64_on_random_nets(F, boards):
    nsg = importlib.import_module("nshogi-engine_amd")
    w = nsg.weights.make_random(2, F, seed=2000 + F, bn="random")
    planes = sn.pool_planes()[:boards]
    ref = ref64.forward(w, planes)
    out = {a: sm.forward(w, planes, a) for a in sm.PRECS}
    for a, o in out.items():
        assert np.abs(o["policy"] - ref["policy"]).max() <= TOL[a], a
        assert np.abs(o["trunk"] - ref["trunk"]).max() <= TOL[a] * max(1.0, np.abs(ref["trunk"]).max()), a
    # the models are the formats, nothing better: each differs from the next finer one
    assert (sn.bits(out["f16m6"]["trunk"]) != sn.bits(out["f16x3"]["trunk"])).any()
    assert (sn.bits(out["f16m8"]["trunk"]) != sn.bits(out["f16x3"]["trunk"])).any()
    assert (sn.bits(out["f16m6"]["trunk"]) != sn.bits(out["f16m8"]["trunk"])).any()
    assert (out["f16x3"]["trunk"].astype(np.float64) != ref["trunk"]).any()


@pytest.mark.parametrize("F", [64, 128, 192, 256, 384])
def test_tier_a_is_exact_in_every_precision(F):
    """Integer nets: the fold is the identity, every activation is an integer that bf16 holds, every lo is zero, the
    float32 sums are exact -- and then every split model IS float64."""
    import torch
    w = sn.net(F, 2, "int")
    for k, v in w.items():
        if k.endswith("_w") or k.endswith("_w1") or k.endswith("_w2"):
            assert (sm.fold(v, sn._identity_bn(v.shape[0]), 0.0)[0] == v).all()
    ref = sn.reference(F, 2, "int")
    rep, keep = [], []
    out = sn.model(F, 2, "int", "f16m6", report=rep, keep=keep)
    assert all(r["exact"] for r in rep), rep
    for k in keep:
        v = np.maximum(k["v"], 0)
        assert (v == np.rint(v)).all() and (sm.f16(v) == v).all(), k["name"]
        if F in (64, 192, 256):  # the widths of the issue; bf16 runs at 256 only (the sweep's rows), 8 bits
            assert (torch.from_numpy(v).to(torch.bfloat16).double().numpy() == v).all(), k["name"]
        assert not k["x"]["lo"][..., :64].any() or k["name"] == "stem_w"
    assert (sn.bits(out["trunk"]) == sn.bits(ref["trunk"])).all() and (sn.bits(out["policy"]) == sn.bits(ref["policy"])).all()
    # the value head: every stage up to the two logits is an integer (fc2 in units of 2^-8) that the narrowest format
    # of the width holds, so the device's logits are float64's and only tanhf / expf stand between them and the outputs
    tr = ref["trunk"].astype(np.float64).transpose(0, 2, 1)                       # [B, 81, F]
    vc = np.maximum(tr @ w["value_w"].astype(np.float64).T, 0).transpose(0, 2, 1).reshape(sn.POOL, -1)
    h = np.maximum(vc @ w["fc1_w"].astype(np.float64).T + w["fc1_b"], 0)
    o = h @ w["fc2_w"].astype(np.float64).T + w["fc2_b"]
    for a in (vc, h, o * 256):
        assert (a == np.rint(a)).all() and np.abs(a).max() < 2048
        if F in (64, 192, 256):
            assert (torch.from_numpy(a).to(torch.bfloat16).double().numpy() == a).all() or a is not vc and a is not h
    assert np.abs(0.5 * (np.tanh(o[:, 0]) + 1) - ref["value"]).max() < 1e-15
    assert np.abs(h).sum(axis=1).max() * 2 + 1 < 2.0 ** 16  # sum |h w2| + |b2| in units of 2^-8: far inside 2^24
    tr = ref["trunk"]
    assert len({b.tobytes() for b in tr}) >= sn.POOL // 4 and tr.std(axis=0).max() > 0 and ref["policy"].std(axis=0).max() > 0


@pytest.mark.parametrize("F,blocks", SHAPES)
def test_tier_b_exactness_and_coverage(F, blocks):
    family = sn.cases(F, blocks)
    for arith in sm.PRECS:
        covered, wbytes3, xbytes3, hl_differ, zero_block, res_lo = set(), False, False, False, False, False
        for name in family:
            if arith not in sn.ariths(name):
                continue
            rep, keep = [], []
            out = sn.model(F, blocks, name, arith, report=rep, keep=keep)
            assert all(r["exact"] for r in rep), (name, arith, rep)
            assert out["trunk"].std(axis=0).max() > 0 and out["policy"].std(axis=0).max() > 0, (name, "constant over the pool")
            assert len({b.tobytes() for b in out["trunk"]}) >= sn.POOL // 4, name
            for li, k in enumerate(keep[1:], start=1):
                x, (w_hi, w_lo, w_hi6) = k["x"], k["w"]
                shown = (k["v"] > 0).reshape(-1, F).astype(np.float32)  # outputs that pass the ReLU
                if li == len(keep) - 1:
                    shown *= (out["trunk"].transpose(0, 2, 1).reshape(-1, F) > 0)
                for term, (xa, wa) in enumerate(((x["xq"], w_lo), (x["lo"], w_hi6))):
                    xp = np.zeros((xa.shape[0], 11, 11, xa.shape[-1]), dtype=np.float32)
                    xp[:, 1:10, 1:10] = (xa != 0).reshape(-1, 9, 9, xa.shape[-1])
                    for t in range(9):
                        wt = wa[:, :, t // 3, t % 3] != 0
                        if not wt.any():
                            continue
                        # the operand this tap reads at each output position, against the outputs shown there: an
                        # actual nonzero product w[n, c, t] x[c at pos + t] in an output that is positive
                        at = xp[:, t // 3:t // 3 + 9, t % 3:t % 3 + 9].reshape(-1, xa.shape[-1])
                        n, c = np.nonzero(wt & ((shown.T @ at) > 0))
                        for p_, j in set(zip(((c // 32) % 2).tolist(), ((n % 16) // 4).tolist())):
                            covered.add((t, p_, term, j))
                if arith == "f16m6":
                    for wv in (w_hi, w_lo):  # the blocks of the e2m3 copy of w_hi take w_hi's bytes; and those of w_lo
                        by = sm.e8m0_weights(np.ascontiguousarray(np.moveaxis(wv, 1, -1)))  # [F, 3, 3, C / 32]
                        g = by.reshape(F // 16, 4, 4, -1)  # out channel = 16 a + 4 j + r: one dword holds j = 0..3
                        srt = np.sort(g, axis=1)
                        wbytes3 |= bool(((np.diff(srt, axis=1) != 0).sum(axis=1) >= 2).any())
                    bh, bl = sm.e8m0_activations(x["hi"]), sm.e8m0_activations(sm.f16(x["lo"]))
                    rows = np.concatenate([bh, bl], axis=-1).reshape(-1, 2 * bh.shape[-1])
                    xbytes3 |= bool(max(len(set(r)) for r in rows[:: max(1, len(rows) // 400)]) >= 3)
                    hl_differ |= bool(((bh != bl) & (sm._blocks(x["lo"]) != 0).any(-1)).any())
                nzrow = (x["hi"] != 0).any(-1)
                zero_block |= bool(((sm._blocks(x["hi"]) == 0).all(-1) & nzrow[..., None]).any())
            if blocks == 2:  # the second block's residual is keep[3]'s input: a nonzero lo under a positive output
                res_lo |= bool(((keep[3]["x"]["lo"] != 0) & (out["trunk"].transpose(0, 2, 1) > 0)).any())
            if name == "edge":
                lo = keep[2]["x"]["lo"]
                b1 = sm.e8m0_activations(sm.f16(lo))[..., 1]
                assert (b1 == 110).all() and (lo[..., 32:64] != 0).all(), "block 1 is not a nonzero block of f16 subnormals"
        if blocks == 2:
            assert res_lo, arith
        if "tap0" in family:
            want = {(t, p, term, j) for t in range(9) for p in range(2) for term in range(2) for j in range(4)}
            assert not want - covered, (arith, sorted(want - covered)[:8])
            assert zero_block, arith
            if arith == "f16m6":
                assert wbytes3 and xbytes3 and hl_differ, (wbytes3, xbytes3, hl_differ)


# fault -> {(channels, blocks, arithmetic): cases on which the trunk's bits must change}.  The device compares the 64
# channel family in f16x3 arithmetic only (an MX evaluator of that width runs the fallback) and the 192 / 256 channel
# families in the evaluator's own, so an MX fault is listed on the wide families.  tap4, blk0 and res run in every launch
# form, edge in every form of f16m6 arithmetic, the other cases on one per-layer and one persistent form.
_WIDE = ((192, 1), (256, 1))
FAULT_CASES = {
    "drop_wlo_xhi": {**{(64, 2, "f16x3"): ("tap0", "tap4", "tap8", "blk0", "blk1")},
                     **{(F, b, a): ("tap4", "blk0") for F, b in _WIDE for a in ("f16m6", "f16m8")}},
    "drop_whi_xlo": {**{(64, 2, "f16x3"): ("tap0", "tap4", "tap8", "blk0", "blk1")},
                     **{(F, b, a): ("tap4", "blk0") for F, b in _WIDE for a in ("f16m6", "f16m8")},
                     **{(F, 2, "f16m6"): ("res",) for F in (192, 256)}},
    "wexp_fragment_xor1": {(F, b, "f16m6"): ("tap4", "blk0") for F, b in _WIDE},
    "xlo_under_hi_exponent": {(F, b, "f16m6"): ("tap4", "blk0") for F, b in _WIDE},
    "residual_lo_dropped": {**{(64, 2, "f16x3"): ("tap4", "blk0")},
                            **{(F, 2, a): ("res",) for F in (192, 256) for a in sm.PRECS}},
    "lo_direct_to_e2m3": {(F, b, "f16m6"): ("edge",) for F, b in _WIDE},
    "subnormal_block_exponent_127": {(F, b, "f16m6"): ("edge",) for F, b in _WIDE},
    "xhi_copy_is_xhi": {**{(F, b, "f16m6"): ("tap4", "blk0") for F, b in _WIDE},
                        **{(F, b, "f16m8"): ("blk0",) for F, b in _WIDE}},
    "tap_transposed": {**{(64, 2, "f16x3"): ("tap1", "tap2", "tap3", "tap5", "tap6", "tap7", "blk0")},
                       **{(F, b, a): ("tap1", "blk0") for F, b in _WIDE for a in ("f16m6", "f16m8")}},
}
FAULT_BOARDS = 8  # boards are independent: a fault shown on the first eight pool entries is shown on the pool


@pytest.mark.parametrize("fault", sorted(FAULT_CASES))
def test_named_fault_changes_compared_bits(fault):
    for (F, blocks, arith), names in FAULT_CASES[fault].items():
        for name in names:
            assert name in sn.cases(F, blocks) and arith in sn.ariths(name)
            good = sn.model(F, blocks, name, arith, boards=FAULT_BOARDS)
            bad = sn.model(F, blocks, name, arith, fault=fault, boards=FAULT_BOARDS)
            assert (sn.bits(good["trunk"]) != sn.bits(bad["trunk"])).any(), (fault, F, blocks, arith, name)


def test_fault_table_is_complete():
    assert set(FAULT_CASES) == set(sm.FAULTS)
    for fault in ("wexp_fragment_xor1", "xlo_under_hi_exponent", "xhi_copy_is_xhi", "lo_direct_to_e2m3",
                  "subnormal_block_exponent_127", "residual_lo_dropped", "drop_wlo_xhi", "drop_whi_xlo"):
        assert any(F > 64 and a == "f16m6" for F, _, a in FAULT_CASES[fault]), fault
