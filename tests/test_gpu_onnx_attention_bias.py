"""Attention with a bias computed at run time on the device (DESIGN.md sections 13.3, 13.4).

Whole models: the generator forms A, B and C of tests/attention_bias_models.py at F = 32, H = 4 (d = 8, D16 = 1) and
form C at F = 64, H = 1 (d = 64, D16 = 4), against the same module in float64 at the general-graph attention tests'
tolerance (max_err < 1e-4).  The generator's last layer is scaled until the bias has a standard deviation between 1 and
4 across the keys (asserted): a near-zero bias would hide a dropped or mis-indexed one.

Near-direct (`RtAttCase`): an exact stem, exact q / k / v and an exact run-time bias through each of the kernel's three
head strides (0, 6561, 6576), against the float64 definition inside the bound derived from the same inputs.  On these
cases acc scale, + bias, + rtScale rt are all exactly representable (asserted in `inputs`), so the terms of the two
added roundings are zero and the bound is section 13.6's with exact scores; the cases at d = 32 and 48 (D16 = 2 and
3) are not exact and carry the full score error with the two added terms.  With the -inf mask every (head, query)
keeps one key and the output equals that key's V row bit for bit; the one-board cases mask a single board of the
batch from run-time data (Log of a 0/1 tensor), and the others stay open.  The host half (`test_the_bound_is_honest`, no
device) holds a float32 numpy evaluation inside the bound and each run-time-bias fault outside it.

Batches 1, 19 and 21 agree bit for bit on the boards they share: with H = 4 the dense launch over the head rows runs
over 4, 76 and 84 rows -- a partial 81-row group, and one group plus three rows."""
import numpy as np
import pytest

import attention_bias_models as abm
import reduction_models as rm
from reduction_models import ratio
from test_gpu_onnx_elementwise import heads_close

gen = abm.gen


@pytest.fixture(scope="module")
def boards(nsg):
    """21 seeded positions (the first 19 are the sibling files') and their planes in float64."""
    bb = nsg.synth.random_batch(21, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def max_err(out, ref):
    return max(float(np.abs(np.asarray(o, np.float64).reshape(-1) - np.asarray(r).reshape(-1)).max()) for o, r in zip(out, ref))


def run_batches(nsg, path, bb, batches=(1, 19, 21)):
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 1
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    ev.close()
    # a board does not depend on its batch
    whole = outs[-1][1]
    for n, o in outs[:-1]:
        for a, b in zip(o, whole):
            np.testing.assert_array_equal(a, b[:n])
    return info, outs


MODELS = [("A", 32, 4, dict()), ("A", 32, 4, dict(bias=True, rt_first=True, swap=True, mul_behind=0.5)),
          ("B", 32, 4, dict(bias=True, scale_on="q")), ("C", 32, 4, dict(bias=True, scale_on="k")),
          ("C", 32, 4, dict(mul_behind=0.5)), ("C", 64, 1, dict(bias=True))]


@pytest.mark.gpu
@pytest.mark.parametrize("form,F,H,kw", MODELS, ids=[f"{f}-{F}-{H}-" + "-".join(kw) for f, F, H, kw in MODELS])
def test_whole_models_match_float64(nsg, boards, tmp_path, form, F, H, kw):
    import torch
    bb, x64 = boards
    x = torch.from_numpy(x64)
    net = abm.build(F, H, 11 + F + H, form=form, **kw)
    sds = gen.sharpen(net, x.float())
    sd = abm.sharpen_bias(net, x.float())
    assert 1.0 < sd < 4.0, sd
    assert all(0.5 < s < 8.0 for s in sds), sds
    path = tmp_path / "m.onnx"
    gen.export_model(net, str(path))
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(x)]
    info, outs = run_batches(nsg, path, bb)
    err = max(max_err(o, [r[:n] for r in ref]) for n, o in outs)
    print(form, F, H, kw, "bias std across keys", sd, "max abs err", err)
    assert err < 1e-4, err


CASES = {"rows": dict(kind="rows"), "flat": dict(kind="flat"), "broadcast": dict(kind="broadcast"),
         "rows_scaled": dict(kind="rows", rt_scale=0.5), "flat_no_constant_bias": dict(kind="flat", bias=None, rt_scale=2.0),
         "flat_masked": dict(kind="flat", mask=True), "broadcast_masked": dict(kind="broadcast", mask=True, rt_scale=0.5),
         "rows_d64": dict(kind="rows", H=1), "rows_masked": dict(kind="rows", mask=True),
         # -inf on one board only, made from run-time data: it must stay with its board
         "flat_one_board": dict(kind="flat", one_board=True), "broadcast_one_board": dict(kind="broadcast", one_board=True),
         # d = 32 and 48: graphAttention<2, true> and <3, true>; the scale is no power of two, the bound carries delta
         "rows_d32": dict(kind="rows", H=2, exact=False), "flat_d48": dict(kind="flat", F=48, H=1, exact=False, rt_scale=0.5)}


def make_case(nsg, name, x):
    kw = dict(CASES[name])
    if kw.pop("one_board", False):
        kw["mask_board"] = x
    return abm.RtAttCase(nsg, kw.pop("F", 64), kw.pop("H", 4), **kw)


def check_single_rows(case, inp, got):
    """Where a (head, query) keeps one key the output is that key's V row, bit for bit."""
    one, key = case.single_rows()
    vk = inp["v"].reshape(len(got), 81, case.F)[:, :, case.ch]
    exp = vk[:, key.reshape(rm.WIN, 81), np.arange(rm.WIN)[:, None]].reshape(len(got), -1)
    rows = slice(None) if case.mask else [case.masked_board(inp["env"])]
    np.testing.assert_array_equal(got[rows][:, one], exp[rows][:, one].astype(np.float32))
    if not case.mask:  # the other boards are open: their rows mix many keys
        others = np.delete(np.arange(len(got)), rows)
        assert (got[others] != exp[others].astype(np.float32)).mean() > 0.9


def fault_case(nsg, fault, x):
    """The case each fault is shown on: the scale needs a factor other than 1, the head fault a bias per head."""
    return make_case(nsg, "rows_scaled" if fault == "rt_scale_dropped" else "flat", x)


def test_the_bound_is_honest(nsg):
    """Host only.  A plain float32 evaluation lies inside the bound on every case; with the bias indexed [key][query],
    head h reading head h-1's bias, board b reading board 0's, or rtScale dropped, it falls outside."""
    bb = nsg.synth.random_batch(5, 86, seed=31)
    x = nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)
    for name in CASES:
        case = make_case(nsg, name, x)
        inp, ref, bound = case.expected(x)
        rt = inp["rt"][np.isfinite(inp["rt"])]
        assert float(rt.std()) > 0.5, (name, float(rt.std()))  # a bias that matters
        if case.thr is not None:  # exactly one board is masked
            assert [int(np.isneginf(r).any()) for r in inp["rt"]].count(1) == 1
            check_single_rows(case, inp, case.select(case.emulate(inp)))
        elif not case.mask:  # it differs per board, per head (where it has heads), per query and per key
            r = inp["rt"]
            assert (r[0] != r[1]).any() and (r[:, :, 0] != r[:, :, 1]).any() and (r[..., 0] != r[..., 1]).any()
            assert r.shape[1] == 1 or (r[:, 0] != r[:, 1]).any()
        got = case.select(case.emulate(inp))
        assert ratio(got, ref, bound) <= 1.0, (name, ratio(got, ref, bound))
    for fault in abm.RT_FAULTS:
        case = fault_case(nsg, fault, x)
        inp, ref, bound = case.expected(x)
        r = ratio(case.select(case.emulate(inp, fault)), ref, bound)
        assert r > 1.0, (fault, r)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_near_direct(nsg, boards, tmp_path, name):
    bb, x = boards
    case = make_case(nsg, name, x)
    inp, ref, bound = case.expected(x)
    path = tmp_path / "m.onnx"
    path.write_bytes(case.data)
    info, outs = run_batches(nsg, path, bb)
    heads_close(outs, inp["env"])
    got = outs[-1][1][0]
    assert np.isfinite(got).all()
    if case.mask or case.thr is not None:
        check_single_rows(case, inp, got)
    r = ratio(got, ref, bound)
    print("run-time bias", name, "error / bound", r, "largest bound", float(bound.max()))
    assert r <= 1.0, r
