"""The L1 / L2 norms, the sum of squares and the log-sum-exp over the channels of a row (graphChanReduce) and the fused
F.normalize launch (graphNormalize) on the device, almost directly: an exact stem, views of it, the ops under test and a
policy that shows their results through nothing that rounds (tests/normalize_models.py).

The bounds, with u = 2^-24 and t_i the terms |x_i| or x_i^2 of a row of C elements.  The inputs are exact.
  * L1: the terms are non-negative, so every partial sum, in any order (lane chains and butterfly alike), is at most
    S (1 + u)^(C-1) with S = sum t_i; a row takes C - 1 adds (adds of an exact 0 do not round), each rounding at most u
    times its partial sum, so |err| <= (C - 1) u S (1 + u)^(C-1) <= C 2^-24 sum t_i for C <= 100.  The assertion adds
    the one final rounding the bound is stated with: C u sum t_i + u |ref|.
  * SumSquare: fmaf(x, x, acc) rounds once per element, the butterfly once per add: the same count, the same bound.
  * L2: sqrt halves the relative error of its argument and sqrtf rounds once: relative C 2^-25 + 2^-24.
  * normalize: d = fmaxf(n, eps) is exact, the division rounds once: relative C 2^-25 + 2^-24 + 2^-24 <= C 2^-25 + 2^-23.
  * On the coarse grid (small integers times 2^-3) every partial sum is exact, so L1 and SumSquare equal float64 rounded
    once, 0 ulps; sqrt and the division of float32 values are correctly rounded, so L2 and the whole F.normalize output
    have one right float32 answer there too, and are compared bit for bit.
  * The log-sum-exp goes through the device's expf and logf, whose error this project measures.  Its
    error against the float64 reference, in float32 ulps of the reference, measured on an MI355X over the grids below
    (the stem's grid of 1/8 and that grid times 2^10, C = 1 .. 100, offsets 0 .. 4, constant channels of +-20, +-90 and
    +-1e4): 30.75 ulps (LSE_ULPS_MEASURED), asserted at twice that.  The figure is large because it counts ulps of the
    result: the worst element is a row of C = 3 at offset 4 whose max m is negative and whose logf(s) nearly cancels
    it, so the result is some 16 times smaller than its two terms and their ordinary roundings weigh 16 times more.
    Away from such cancellation the largest error measured in the same run is 3.9 ulps (C = 3, offset 3), and 1.3 ulps
    on the flat rows."""
import numpy as np
import pytest

import elt_models as em
import gate_models as gm
import normalize_models as nm
from test_gpu_onnx_elementwise import device, heads_close

F = nm.F
U = nm.U
BATCHES = (1, 2, 3)
LSE_ULPS_MEASURED = 30.75  # the largest error of the run described above; the assertion is twice this
KINDS = ["spatial", "token", "flat"]


@pytest.fixture(scope="module")
def boards(nsg):
    bb = nsg.synth.random_batch(3, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


@pytest.fixture(scope="module")
def real_boards(nsg, golden_dir):
    bb = np.load(f"{golden_dir}/net_graph.npz")["bitboards86"][:3]
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def shown(policy, kind):
    return policy[:, :F] if kind == "flat" else policy.reshape(len(policy), F, 81)


def same_in_every_batch(outs):
    for (_, one), (_, whole) in zip(outs, outs[1:]):
        np.testing.assert_array_equal(one[0], whole[0][:len(one[0])])


def lse_check(got, ref, what):
    fin = np.isfinite(ref)
    np.testing.assert_array_equal(got[~fin], ref[~fin].astype(np.float32))
    worst = float(nm.ulps(got[fin], ref[fin]).max()) if fin.any() else 0.0
    print("LSE ulps", what, worst)
    assert worst <= 2 * LSE_ULPS_MEASURED, (what, worst)
    return worst


# ---- 1 + 2: every lane split, bit for bit on the exact grid ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("off", nm.OFFSETS)
@pytest.mark.parametrize("kind", KINDS)
def test_the_four_reductions_at_every_lane_split(nsg, boards, tmp_path, kind, off):
    """C in {1, 3, 4, 5, 15, 16, 17, 24, 63, 64, 65, 100} at the offset: head 0..3, an empty body, tail 0..3, more than one
    float4 per lane.  The channel in front of the offset and the one behind the widest view hold 1e30.  On the grid of 1/8
    every partial sum is exact: L1 and SumSquare equal float64 rounded once, L2 is its correctly rounded sqrt."""
    bb, x = boards
    W = off + 100 + 1 + F
    poison = {off + 100: gm.POISON, **({off - 1: gm.POISON} if off else {})}
    for ops in (("ReduceL1", "ReduceSumSquare"), ("ReduceL2", "ReduceLogSumExp")):
        items = [(op, off, C) for op in ops for C in nm.WIDTHS]
        net, data = nm.pack_model(nsg, kind, items, W, channels=poison, seed=off)
        rows = nm.rows64(net, x, kind)[..., off:off + 100]
        assert gm.sums_exact(rows, -3) and gm.sums_exact(rows * rows, -6)
        _, outs = device(nsg, data, bb, tmp_path, BATCHES)
        same_in_every_batch(outs)
        got = shown(outs[-1][1][0], kind)
        assert np.isfinite(got).all()
        for i, (op, _, C) in enumerate(items):
            ref = nm.reduce64(op, rows[..., :C], (-1,))[..., 0]
            if op == "ReduceLogSumExp":
                lse_check(got[:, i], ref, (kind, off, C))
            else:
                np.testing.assert_array_equal(got[:, i], ref.astype(np.float32), err_msg=f"{op} {kind} off {off} C {C}")
        heads_close(outs, net.run(x, rounded=False))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["spatial", "flat"])
def test_exact_cases_of_the_reductions(nsg, boards, tmp_path, kind):
    """Rows that are the same on every square (zero stem weights): one non-zero element v = -2.75 among zeros, v among
    -inf, all zeros, all -inf, one +inf, and C copies of 1e4; C = 17 at offsets of every residue of 4.  Bit for bit.  (Flat
    rows are shown through a 0/1 selection Gemm, where an infinite result would turn its neighbours into NaN: the two
    cases whose result is infinite run on the spatial rows only.)"""
    bb, _ = boards
    C, v = 17, -2.75
    blocks = {"one": {7: v}, "ninf": {j: -np.inf for j in range(C) if j != 7} | {7: v}, "zero": {}, "allninf": {j: -np.inf for j in range(C)},
              "pinf": {j: 0.5 for j in range(C)} | {11: np.inf}, "big": {j: 1e4 for j in range(C)}}
    chans, items, want = {}, [], []
    base = 3
    for name, vals in blocks.items():
        if kind == "flat" and name in ("allninf", "pinf"):
            continue
        for j in range(C):
            chans[base + j] = vals.get(j, 0.0)
        row = np.array([vals.get(j, 0.0) for j in range(C)])
        for op in nm.REDUCE if name in ("one", "zero") else ["ReduceLogSumExp"]:  # the infinities and 1e4 are the log-sum-exp's cases
            items.append((op, base, C))
            want.append((name, op, row))
        base += C + 2  # offsets 3, 22, 41, ...: every residue of 4
    assert len(items) <= F
    net, data = nm.pack_model(nsg, kind, items, base + F, channels=chans)
    _, outs = device(nsg, data, bb, tmp_path, BATCHES)
    same_in_every_batch(outs)
    got = shown(outs[-1][1][0], kind)
    logC = np.log(np.float64(C))
    # fl(1e4 + logf(C)) is the same float32 for every logf within 4 ulps: 1e4's ulp is 2^-10, far above logf's error
    big = np.float32(1e4 + logC)
    assert np.float32(1e4 + logC * (1 + 2.0 ** -21)) == big == np.float32(1e4 + logC * (1 - 2.0 ** -21)) and np.isfinite(big)
    for i, (name, op, row) in enumerate(want):
        g = got[:, i]
        if op == "ReduceLogSumExp" and name == "big":
            expect = big
        elif op == "ReduceLogSumExp" and name in ("one", "zero"):
            ref = np.full(g.shape, nm.reduce64(op, row[None], (-1,))[0, 0])
            lse_check(g, ref, name)
            continue
        else:
            expect = np.float32(nm.reduce64(op, row[None], (-1,))[0, 0])
        assert expect == {"one": {"ReduceL1": 2.75, "ReduceL2": 2.75, "ReduceSumSquare": 7.5625}.get(op, expect), "ninf": v,
                          "zero": 0.0, "allninf": -np.inf, "pinf": np.inf, "big": big}[name]
        np.testing.assert_array_equal(g, np.full(g.shape, expect, np.float32), err_msg=f"{name} {op}")


# ---- 3: the fused launch equals the two-launch path, and float64 rounded once -----------------------------------------
def both_paths(nsg, bb, tmp_path, **kw):
    kind = kw.pop("kind")
    res = []
    for twin in (False, True):
        net, data, ch = nm.normalize_model(nsg, kind, twin=twin, **kw)
        info, outs = device(nsg, data, bb, tmp_path, BATCHES)
        same_in_every_batch(outs)
        res.append((net, info, outs, ch))
    (net, fused_info, fused, ch), (_, twin_info, twin, _) = res
    assert twin_info["launches"] >= fused_info["launches"] + 1
    for (_, a), (_, b) in zip(fused, twin):
        np.testing.assert_array_equal(a[0], b[0])
    return net, fused, ch


@pytest.mark.gpu
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("off", nm.OFFSETS)
def test_normalize_at_every_lane_split_fused_and_unfused(nsg, boards, tmp_path, off, p):
    """Flat rows show every channel: all twelve widths at the offset, kLaunchNormalize against the twin whose norm has a
    second reader (kLaunchChanReduce, then Clip and Div in an elementwise launch), bit for bit; and both against the one
    right float32 answer of the exact grid.  A selection Gemm reads the pad channels against zero weights."""
    bb, x = boards
    for C in nm.WIDTHS:
        net, outs, ch = both_paths(nsg, bb, tmp_path, kind="flat", off=off, C=C, p=p, eps=1e-6, seed=C, width=off + C + 1,
                                   channels={off + C: gm.POISON, **({off - 1: gm.POISON} if off else {})})
        rows = nm.rows64(net, x, "flat")[..., off:off + C]
        assert gm.sums_exact(rows, -3) and gm.sums_exact(rows * rows, -6)
        ref = em.f32(rows / np.maximum(em.f32(nm.reduce64("ReduceL1" if p == 1 else "ReduceL2", rows, (-1,))), np.float64(np.float32(1e-6))))
        np.testing.assert_array_equal(outs[-1][1][0], nm.shown_normalize(ref, "flat", ch).astype(np.float32), err_msg=f"C {C}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["spatial", "token"])
def test_normalize_on_real_positions_fused_and_unfused(nsg, real_boards, tmp_path, kind):
    """Board and token rows of the golden positions: C = 27 at offsets 0 .. 4 (every channel shown), and C = 100 at offset 3
    through a window of 27 behind a selection that reads the pads.  Fused = unfused = float64 rounded once."""
    bb, x = real_boards
    for off, C, p, start in [(o, F, 2, 0) for o in nm.OFFSETS] + [(1, F, 1, 0), (3, 100, 2, 0), (3, 100, 1, 81)]:
        net, outs, ch = both_paths(nsg, bb, tmp_path, kind=kind, off=off, C=C, p=p, seed=off, start=start)
        rows = nm.rows64(net, x, kind)[..., off:off + C]
        assert gm.sums_exact(rows, -3) and gm.sums_exact(rows * rows, -6)
        n = em.f32(nm.reduce64("ReduceL1" if p == 1 else "ReduceL2", rows, (-1,)))
        ref = em.f32(rows / np.maximum(n, np.float64(np.float32(1e-12))))
        np.testing.assert_array_equal(outs[-1][1][0], nm.shown_normalize(ref, kind, ch).astype(np.float32), err_msg=f"{off} {C} {p}")
        heads_close(outs, net.run(x, rounded=False))


@pytest.mark.gpu
def test_exact_cases_of_normalize(nsg, boards, tmp_path):
    """A row with one non-zero element gives -1 there and 0 elsewhere (L1 and L2); an all-zero row gives zeros, 0 / eps."""
    bb, _ = boards
    for p in (1, 2):
        for vals in ({5: -2.75}, {}):
            chans = {j: vals.get(j - 3, 0.0) for j in range(3, 3 + 17)}
            _, data, ch = nm.normalize_model(nsg, "spatial", 3, 17, p=p, channels=chans, width=40)
            _, outs = device(nsg, data, bb, tmp_path, BATCHES)
            want = np.zeros(17)
            for j in vals:
                want[j] = -1.0
            for n, o in outs:
                np.testing.assert_array_equal(o[0], np.broadcast_to(want[ch][None, :, None], (n, F, 81)).reshape(n, -1).astype(np.float32))


# ---- 4: against float64 where the sums round ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("scale_exp", [-11, -1])
@pytest.mark.parametrize("kind", KINDS)
def test_rounding_sums_are_inside_their_bounds(nsg, boards, tmp_path, kind, scale_exp):
    """The 2^-11 grid with channel offsets of 4096 and -1024 (partial sums leave float32), and that grid times 2^10.
    L1, SumSquare: |err| <= C u sum t_i + u |ref|.  L2: relative C 2^-25 + 2^-24."""
    bb, x = boards
    off = 1
    items = [(op, off, C) for op in ("ReduceL1", "ReduceSumSquare", "ReduceL2") for C in (3, 16, 17, 24, 63, 64, 65, 100)]
    net, data = nm.pack_model(nsg, kind, items, off + 100 + F, exp=-11, fine=True)
    if scale_exp != -11:  # the same grid times 2^10
        for k in ("s_w", "s_b"):
            net.consts[k][:] = net.consts[k] * np.float32(2.0 ** (scale_exp + 11))
        data = net.data()
    rows = nm.rows64(net, x, kind)[..., off:off + 100]
    assert not gm.sums_exact(rows * rows, 2 * scale_exp)
    _, outs = device(nsg, data, bb, tmp_path, BATCHES)
    same_in_every_batch(outs)
    got = shown(outs[-1][1][0], kind).astype(np.float64)
    for i, (op, _, C) in enumerate(items):
        v = rows[..., :C]
        ref = nm.reduce64(op, v, (-1,))[..., 0]
        t = np.abs(v) if op == "ReduceL1" else v * v
        if op == "ReduceL2":
            bound = (C * 2.0 ** -25 + 2.0 ** -24) * ref
        else:
            bound = C * U * t.sum(axis=-1) + U * np.abs(ref)
        err = np.abs(got[:, i] - ref)
        print(kind, op, C, "error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (op, C, float((err / bound).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_rounding_normalize_is_inside_its_bound(nsg, boards, tmp_path, kind):
    """The same fine grid: every element within relative C 2^-25 + 2^-23 of float64, L1 and L2."""
    bb, x = boards
    for p in (1, 2):
        for off, C in ((1, F), (2, 100)):
            net, data, ch = nm.normalize_model(nsg, kind, off, C, p=p, exp=-11, fine=True, start=40)
            rows = nm.rows64(net, x, kind)[..., off:off + C]
            ref = nm.shown_normalize(nm.normalize64(rows, p, 1e-12), kind, ch)
            _, outs = device(nsg, data, bb, tmp_path, BATCHES)
            same_in_every_batch(outs)
            err = np.abs(outs[-1][1][0].astype(np.float64) - ref)
            bound = (C * 2.0 ** -25 + 2.0 ** -23) * np.abs(ref)
            print(kind, p, off, C, "error / bound", float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_the_log_sum_exp_against_float64(nsg, boards, tmp_path, kind):
    """The grid of 1/8 and that grid times 2^10 (rows whose max dwarfs the rest), and rows with constant channels of +-20,
    +-90 and +-1e4 beside the grid: within twice the measured ulps of the float64 reference."""
    bb, x = boards
    worst = 0.0
    consts = [20.0, -20.0, 90.0, -90.0, 1e4, -1e4]
    for exp, chans in ((-3, {}), (7, {}), (-3, {2 + 5 * i: c for i, c in enumerate(consts)})):
        views = [(0, 3), (1, 5), (2, 17), (3, 24), (4, 27), (0, 33), (1, 64), (2, 100)]
        if chans:  # views that hold one of the constants, pairs of opposite sign, all of them
            views = [(0, 4), (4, 6), (10, 6), (16, 4), (20, 6), (26, 6), (0, 16), (8, 20), (0, 40), (20, 17), (1, 100)]
        items = [("ReduceLogSumExp", o, C) for o, C in views]
        net, data = nm.pack_model(nsg, kind, items, 102 + F, exp=exp, channels=chans, seed=exp + 20)
        rows = nm.rows64(net, x, kind)
        _, outs = device(nsg, data, bb, tmp_path, BATCHES)
        same_in_every_batch(outs)
        got = shown(outs[-1][1][0], kind)
        for i, (_, o, C) in enumerate(items):
            ref = nm.reduce64("ReduceLogSumExp", rows[..., o:o + C], (-1,))[..., 0]
            assert np.isfinite(ref).all()
            worst = max(worst, lse_check(got[:, i], ref, (kind, exp, bool(chans), o, C)))
    print("LSE worst ulps", kind, worst)


# ---- 5: batch independence and containment --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("what", ["normalize", "ReduceLogSumExp", "ReduceL2"])
def test_a_board_between_neighbours_at_1e30(nsg, tmp_path, what):
    """A board alone, and as the first, middle and last of three whose other boards hold 1e30 in every stem channel: equal bits."""
    from test_gpu_onnx_gate import lone_board
    bb, plane, me, others = lone_board(nsg)
    net = nm.NNet(nsg)
    net.stem(F + 4)
    net.consts["s_w"][:, plane, 1, 1] = gm.POISON
    v = net.slice("s", 1, 1 + F, 1, "v")
    if what == "normalize":
        y = net.normalize(v, 1, "y", eps=1e-6, expand_to=[1, F, 9, 9])
    else:
        y = net.node("Sub", [v, net.reduce(what, v, "r", 1)], "y")
    net.show(y, "spatial")
    net.heads_of("s", F + 4)
    path = tmp_path / "m.onnx"
    path.write_bytes(net.data())
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    alone = ev.compute_blocking(bb[[me]])[0][0].copy()
    assert np.isfinite(alone).all() and float(np.abs(alone).max()) < 1e6
    for pos in range(3):
        order = others[:pos] + [me] + others[pos:]
        whole = ev.compute_blocking(bb[order])[0].copy()
        np.testing.assert_array_equal(whole[pos], alone)
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_infinities_outside_the_view_change_nothing(nsg, boards, tmp_path, kind):
    """+inf in the channels just outside [offset, offset + C) of the source rows: every reduction and the normalised rows
    keep their bits.  (offset, C) = (1, 3), (3, 17), (5, 63), (4, 64): ragged and aligned ends."""
    bb, _ = boards
    views = [(1, 3), (3, 17), (5, 63), (4, 64)]
    res = []
    for planted in (False, True):
        outs_all = []
        for off, C in views:
            chans = {off - 1: np.inf, off + C: np.inf} if planted else {}
            items = [(op, off, C) for op in nm.REDUCE]
            _, data = nm.pack_model(nsg, kind, items, off + C + 1 + F, channels=chans, seed=C)
            outs_all.append(device(nsg, data, bb, tmp_path, (3,))[1][0][1][0][:, :4 * 81 if kind != "flat" else 4])
            for p in (1, 2):
                _, data, _ = nm.normalize_model(nsg, kind, off, C, p=p, channels=chans, seed=C, width=off + C + 1 + F)
                outs_all.append(device(nsg, data, bb, tmp_path, (3,))[1][0][1][0])
        res.append(outs_all)
    for a, b in zip(*res):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_the_pad_channels_of_the_new_rows_are_zero(nsg, boards, tmp_path):
    """A 1x1 conv of ones reads the reduced row's whole 16-channel chunk against zero pad weights: a NaN or an infinity in
    a pad would come out as NaN.  The last case makes the result itself +inf (two elements at 3e38: x^2 overflows, which
    the L2 norm does not rescale away): a kernel that wrote its result to every channel would turn inf * 0 into NaN."""
    bb, x = boards
    for op, overflow in [(op, False) for op in nm.REDUCE] + [("ReduceL2", True), ("ReduceL1", True)]:
        net = nm.NNet(nsg)
        net.stem(F + 1)
        nm.set_channels(net, {F: gm.POISON, **({0: 3e38, 1: 3e38} if overflow else {})})
        r = net.reduce(op, net.slice("s", 0, F, 1, "v"), "r", 1)
        net.node("Conv", [r, net.const("ones", np.ones((F, 1, 1, 1)))], "y", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
        net.show("y", "spatial")
        net.heads_of("s", F + 1)
        _, outs = device(nsg, net.data(), bb, tmp_path, BATCHES)
        for n, o in outs:
            assert np.isposinf(o[0]).all() if overflow else np.isfinite(o[0]).all(), op


# ---- 6: end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_exported_cosine_policy_model_against_torch_float64(nsg, real_boards, tmp_path):
    """Stem, F.normalize over the tokens of two embeddings, their cosine similarity (kLaunchBmm), a value head on
    x - logsumexp(x): loaded from memory, within the 1e-4 of the other exported models, opsets 13 and 17 bit for bit."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_onnx_norm_golden as gen
    import torch
    bb, x = real_boards
    net = gm.randomize(nm.cosine_net(), 3)
    with torch.no_grad():
        want = [t.numpy() for t in net.double()(torch.from_numpy(x))]
    net.float()
    res = {}
    for opset in (13, 17):
        torch.manual_seed(1)
        data = gen.export_model(net.eval(), str(tmp_path / f"e{opset}.onnx"), fold=True, opset=opset)  # (a Linear's weight Transpose folds)
        ev = nsg.Evaluator(0, 32, 86)
        ev.load_memory(data)
        info = ev.graph_info()
        assert info["path"] == "graph"
        res[opset] = [o.copy() for o in ev.compute_blocking(bb)]
        ev.close()
        for got, ref in zip(res[opset], want):
            assert float(np.abs(got.reshape(ref.shape).astype(np.float64) - ref).max()) < 1e-4
    for a, b in zip(res[13], res[17]):
        np.testing.assert_array_equal(a, b)
