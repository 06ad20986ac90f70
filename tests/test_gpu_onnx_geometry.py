"""Convolution geometries on the device: the geometry fixture against its float64 PyTorch outputs, batch independence,
exact integer taps for every kernel shape, a zero-ringed 5x5 net that must give the bits of its 3x3 centre, width
sweeps of the dense and the depthwise kernel, and the evaluator contract on the fixture."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

NAME = "net_graph_geom"
# kernel, dilation
GEOMETRIES = [(5, 1), (7, 1), (9, 1), ((1, 9), 1), ((9, 1), 1), ((3, 1), 1), (3, 2), (3, 4), (5, 2)]


def gid(v):
    return str(v).replace(" ", "")


@pytest.fixture(scope="module")
def gen():
    import make_onnx_geometry_golden
    return make_onnx_geometry_golden


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(f"{golden_dir}/net_geom.npz"))
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
def test_geometry_fixture_matches_pytorch(nsg, golden_dir, golden):
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


def outermost_zeroed(w):
    """The weight with its outermost taps (first and last row and column of the kernel, where there is more than one)
    set to zero."""
    w = w.clone()
    if w.shape[2] > 1:
        w[:, :, 0, :] = 0
        w[:, :, -1, :] = 0
    if w.shape[3] > 1:
        w[:, :, :, 0] = 0
        w[:, :, :, -1] = 0
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("k,d", GEOMETRIES, ids=gid)
def test_exact_taps(nsg, gen, boards, tmp_path, k, d):
    """Integer weights on 0/1 planes (zero on the four planes that hold fractions): every partial sum is an integer far
    below 2^24 (at most 2 * 81 taps * 86 planes), so the policy equals the float64 reference.  86 planes pad to 96: six chunks, the last one partly empty; 9x9 has 81
    taps, eleven weight groups."""
    import torch
    net = gen.TapNet(k, d, seed=7).eval()
    x = boards[1]
    # the outermost taps matter at a corner and at the centre: a kernel that dropped them, or read a wrong halo,
    # cannot pass
    with torch.no_grad():
        full = net.double()(x)[0].reshape(-1, 27, 81)
        w = net.p.weight.clone()
        net.p.weight.copy_(outermost_zeroed(w))
        cut = net(x)[0].reshape(-1, 27, 81)
        net.p.weight.copy_(w)
    assert float(full.abs().max()) < 2 ** 24 and bool((full == full.round()).all())
    for sq in (0, 40):
        assert bool((full[:, :, sq] != cut[:, :, sq]).any()), sq
    outs, ref = run(nsg, gen, net, boards, tmp_path / "taps.onnx")
    for n, o in outs:
        np.testing.assert_array_equal(o[0], ref[0][:n])
        assert max_err(o[1:], [r[:n] for r in ref[1:]]) < 1e-4


@pytest.mark.gpu
def test_a_zero_ring_is_bit_identical(nsg, gen, boards, tmp_path):
    """A 5x5 kernel whose outer ring is zero adds 0 * x to a finite chain -- an exact no-op -- in the 3x3 kernel's
    order (chunk, tap, channel): the 5x5 net on the new kernel gives the bits of the 3x3 net on graphConv<9>."""
    import torch
    torch.manual_seed(24)
    small = gen.randomize(gen.RingNet(3, F=24), 25).eval()
    big = gen.zero_ring_copy(small, 5).eval()
    with torch.no_grad():
        for a, b in zip(small(boards[1].float()), big(boards[1].float())):
            assert float((a - b).abs().max()) < 1e-5  # the same function
    o3, _ = run(nsg, gen, small, boards, tmp_path / "k3.onnx")
    o5, _ = run(nsg, gen, big, boards, tmp_path / "k5.onnx")
    for (n, a), (_, b) in zip(o3, o5):
        assert float(np.abs(a[0]).max()) > 1e-3
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", [(24, 40), (40, 72), (64, 64)])
@pytest.mark.parametrize("k,d", [(5, 1), ((1, 9), 1), (3, 2)], ids=gid)
def test_width_sweep(nsg, gen, boards, tmp_path, cin, cout, k, d):
    """Pad channels (24, 40), a partial 64-tile (40) and two tiles (72), with BatchNorm, a residual and ReLU fused."""
    import torch
    torch.manual_seed(cin * 7 + cout)
    net = gen.randomize(gen.BlockNet(cin, cout, k, d), cin + cout).eval()
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "w.onnx")
    print(cin, cout, k, d, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["bare", "bn_res_swish"])
@pytest.mark.parametrize("C", [24, 40, 64])
@pytest.mark.parametrize("k,d", [(3, 1), (5, 1), (7, 1), ((1, 9), 1), (3, 2)], ids=gid)
def test_depthwise_sweep(nsg, gen, boards, tmp_path, k, d, C, full):
    import torch
    torch.manual_seed(C * 3 + full)
    net = gen.randomize(gen.DwNet(C, k, d, full=full), C + 2 * full).eval()
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "dw.onnx")
    print(C, k, d, full, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
def test_depthwise_exact_taps(nsg, gen, boards, tmp_path):
    """Integer per-channel 7x7 taps over the 0/1 planes (at most 2 * 49 + 3 per channel), then an integer 1x1 to 27
    channels: integers below 2^24 throughout, so the policy equals the float64 reference."""
    import torch
    net = gen.DwTapNet(7, seed=3).eval()
    with torch.no_grad():
        full = net.double()(boards[1])[0].reshape(-1, 27, 81)
        w = net.dw.weight.clone()
        net.dw.weight.copy_(outermost_zeroed(w))
        cut = net(boards[1])[0].reshape(-1, 27, 81)
        net.dw.weight.copy_(w)
    assert float(full.abs().max()) < 2 ** 24 and bool((full == full.round()).all())
    for sq in (0, 40):
        assert bool((full[:, :, sq] != cut[:, :, sq]).any()), sq
    outs, ref = run(nsg, gen, net, boards, tmp_path / "dwtaps.onnx")
    for n, o in outs:
        np.testing.assert_array_equal(o[0], ref[0][:n])


@pytest.mark.gpu
def test_evaluator_contract_on_the_geometry_fixture(nsg, golden_dir, golden):
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
    assert sh.graph_info()["path"] == "graph" and sh.graph_info()["conv_launches"] == 12
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
