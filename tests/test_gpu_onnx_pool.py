"""Pooling, the global max, Split and the clamp activations on the device: the pooling fixture against its float64
PyTorch outputs, batch independence, max pooling exact on integers for every window shape, the two average divisors, a
sweep of widths and view offsets, both export forms of the global max, every new activation in a conv epilogue and in an
elementwise chain, and the evaluator contract on the fixture."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

NAME = "net_graph_pool"


def gid(v):
    return str(v).replace(" ", "")


@pytest.fixture(scope="module")
def gen():
    import make_onnx_pool_golden
    return make_onnx_pool_golden


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(f"{golden_dir}/net_pool.npz"))
    g["bitboards"] = np.load(f"{golden_dir}/net_graph.npz")["bitboards86"]
    g[f"{NAME}_policy"] = np.concatenate([np.load(f"{golden_dir}/{NAME}_policy_{h}.npz")["policy"] for h in range(2)])
    return g


@pytest.fixture(scope="module")
def boards(nsg):
    """19 seeded positions and their planes as a float64 tensor, shared by the test-time models."""
    import torch
    bb = nsg.synth.random_batch(19, 86, seed=31)
    x = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64))
    return bb, x


def max_err(out, ref):
    return max(float(np.abs(np.asarray(o, np.float64).reshape(-1) - np.asarray(r).reshape(-1)).max()) for o, r in zip(out, ref))


def run(nsg, gen, net, boards, path, batches=(1, 19)):
    """Exports `net`, runs it on the device for each batch and returns [(n, outputs)] and the float64 reference of the
    same module on the CPU."""
    import torch
    bb, x = boards
    gen.export_model(net.float(), str(path))
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(x)]
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    assert ev.graph_info()["path"] == "graph"
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    ev.close()
    return outs, ref


def err_against_float64(nsg, gen, net, boards, path):
    outs, ref = run(nsg, gen, net, boards, path)
    return max(max_err(o, [r[:n] for r in ref]) for n, o in outs)


@pytest.mark.gpu
def test_pool_fixture_matches_pytorch(nsg, golden_dir, golden):
    ref = [golden[f"{NAME}_policy"], golden[f"{NAME}_value"], golden[f"{NAME}_draw"]]
    ev = nsg.Evaluator(0, 64, 86, precision="fp32")
    ev.load(f"{golden_dir}/{NAME}.onnx")
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    for n in (1, 6, 17, 64):
        out = ev.compute_blocking(golden["bitboards"][:n])
        err = max_err(out, [r[:n] for r in ref])
        print(NAME, n, "max abs err", err)
        assert err < 1e-4, (n, err)
    assert ev.last_plan()["trunk_precision"] == "fp32"
    ev.close()


@pytest.mark.gpu
def test_a_board_does_not_depend_on_its_batch(nsg, golden_dir, golden):
    ev = nsg.Evaluator(0, 64, 86)
    ev.load(f"{golden_dir}/{NAME}.onnx")
    bb = golden["bitboards"][:37]
    whole = [x.copy() for x in ev.compute_blocking(bb)]
    for b in range(37):
        one = ev.compute_blocking(bb[b:b + 1])
        for x, y in zip(one, whole):
            np.testing.assert_array_equal(x[0], y[b])
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("k,d", [(3, 1), (5, 1), (9, 1), ((1, 9), 1), ((9, 1), 1), (3, 2), (3, 4)], ids=gid)
def test_max_pooling_is_exact(nsg, gen, boards, tmp_path, k, d):
    """The max of 0/1 planes is 0 or 1, and the integer 1x1 conv behind it sums at most 86 of them times 2, plus 3:
    integers far below 2^24, so the policy equals the float64 reference bit for bit.  A window cut to its centre row
    and column (a 1-D window: to all but its two ends) changes the policy at a corner and at the centre, so a kernel
    that dropped the outer taps or read a wrong halo cannot pass."""
    import torch
    net = gen.PoolTapNet("max", k, d, seed=7).eval()
    x = boards[1]
    with torch.no_grad():
        full = net.double()(x)[0].reshape(-1, 27, 81)
        net.cut = True
        cut = net(x)[0].reshape(-1, 27, 81)
        net.cut = False
    assert float(full.abs().max()) < 2 ** 24 and bool((full == full.round()).all())
    for sq in (0, 40):
        assert bool((full[:, :, sq] != cut[:, :, sq]).any()), sq
    outs, ref = run(nsg, gen, net, boards, tmp_path / "max.onnx")
    for n, o in outs:
        np.testing.assert_array_equal(o[0], ref[0][:n])
        assert max_err(o[1:], [r[:n] for r in ref[1:]]) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("include", [0, 1], ids=["exclude_pad", "include_pad"])
@pytest.mark.parametrize("k", [3, 5, (3, 1), (1, 9)], ids=gid)
def test_average_divisors(nsg, gen, boards, tmp_path, k, include):
    """count_include_pad 0 and 1 differ at a corner (a 3x3 window there holds 4 squares, not 9) and agree at the
    centre: a wrong divisor is an error of the order of the policy itself, far above the bar."""
    import torch
    net = gen.PoolTapNet("avg", k, include, seed=9).eval()
    if k == 3:
        other = gen.PoolTapNet("avg", k, 1 - include, seed=9).eval()
        with torch.no_grad():
            a = net.double()(boards[1])[0].reshape(-1, 27, 81)
            b = other.double()(boards[1])[0].reshape(-1, 27, 81)
        assert float((a[:, :, 0] - b[:, :, 0]).abs().max()) > 1e-2
        assert float((a[:, :, 40] - b[:, :, 40]).abs().max()) < 1e-12
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "avg.onnx")
    print(k, include, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
@pytest.mark.parametrize("kind,k", [("max", 3), ("avg", 3), ("max", 5)], ids=["max3", "avg_exclude3", "max5"])
@pytest.mark.parametrize("split", [6, 8, 16])
@pytest.mark.parametrize("C", [24, 40, 64])
def test_widths_and_view_offsets(nsg, gen, boards, tmp_path, C, split, kind, k):
    """The pooled part is a view at channel `split` of the stem's rows: 6 is no multiple of 4 (scalar loads), 8 a
    multiple of 4 but not of 16, 16 a chunk.  Its width C - split is 18, 16, 8, 34, 32, 24, 58, 56 or 48: last chunks
    with 2, 8 and 10 channels beside full ones, widths that 4 does not divide (18, 34, 58: a last piece of 2
    channels read with scalar loads whatever the offset), and one to four chunks, the grid's second axis."""
    import torch
    torch.manual_seed(C * 5 + split)
    net = gen.randomize(gen.PoolBlockNet(C, split, kind, k), C + split).eval()
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "b.onnx")
    print(C, split, kind, k, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
def test_global_max_is_exact(nsg, gen, boards, tmp_path):
    """An integer stem on 0/1 planes, the max over the squares both ways the exporter writes it, an integer Linear:
    integers below 2^24 throughout, so the policy equals the float64 reference."""
    import torch
    net = gen.GlobalMaxNet(seed=5).eval()
    with torch.no_grad():
        full = net.double()(boards[1])[0]
    assert float(full.abs().max()) < 2 ** 24 and bool((full == full.round()).all()) and float(full.std()) > 1
    outs, ref = run(nsg, gen, net, boards, tmp_path / "gmax.onnx")
    for n, o in outs:
        np.testing.assert_array_equal(o[0], ref[0][:n])


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["epilogue", "chain"])
@pytest.mark.parametrize("act", ["relu6", "hardswish", "hardsigmoid", "hardtanh", "clamp_min", "leaky_relu", "prelu",
                                 "maximum", "minimum", "abs", "neg"])
def test_activations(nsg, gen, boards, tmp_path, act, where):
    import torch
    torch.manual_seed(11)
    net = gen.ActNet(act, where, boards[1], seed=13).eval()
    # a condition on the inputs, checked on the CPU reference: the pre-activations fall on both sides of every kink
    with torch.no_grad():
        pre = net.double().pre(boards[1]).reshape(-1)
    kinks = gen.ACTS[act][1]
    for kink in ((0.0,) if kinks is None else kinks):
        below = float((pre < kink).double().mean())
        assert 0.05 <= below <= 0.95, (act, kink, below)
    if act == "prelu":
        assert float(net.prelu.weight.min()) < 0 and float(net.prelu.weight.max()) > 1
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "act.onnx")
    print(act, where, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
def test_evaluator_contract_on_the_pool_fixture(nsg, golden_dir, golden):
    path = f"{golden_dir}/{NAME}.onnx"
    ref = [golden[f"{NAME}_policy"], golden[f"{NAME}_value"], golden[f"{NAME}_draw"]]
    bb = golden["bitboards"][:16]
    ev = nsg.Evaluator(0, 16, 86)
    ev.load(path)
    p, v, d = [x.copy() for x in ev.compute_blocking(bb)]
    # gather
    rng = np.random.default_rng(4)
    counts = rng.integers(1, 40, size=16)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    idx = np.concatenate([rng.choice(2187, c, replace=False) for c in counts]).astype(np.uint16)
    vals, v2, d2 = ev.compute_gather_blocking(bb, idx, off)
    np.testing.assert_array_equal(vals, np.concatenate([p[b, idx[off[b]:off[b + 1]]] for b in range(16)]))
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(d2, d)
    # nsg_load_shared on the same device: identical outputs
    sh = nsg.Evaluator(0, 16, 86)
    sh.load_shared(ev)
    assert sh.graph_info()["path"] == "graph" and sh.graph_info()["conv_launches"] == 16
    for x, y in zip(sh.compute_blocking(bb), (p, v, d)):
        np.testing.assert_array_equal(x, y)
    # an f16m6 evaluator runs the general graph in fp32
    m6 = nsg.Evaluator(0, 16, 86, precision="f16m6")
    m6.load(path)
    info = m6.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    o6 = m6.compute_blocking(bb)
    assert m6.last_plan()["trunk_precision"] == "fp32"
    assert max_err(o6, [r[:16] for r in ref]) < 1e-4
    for x in (ev, sh, m6):
        x.close()
