"""Grouped convolutions on the device (graphConvGrouped): exact integers for every shape of
group_models.SHAPES and every geometry class, the bits of the dense kernels on a Split / Concat twin, a ResNeXt-style
net against float64 PyTorch, batch independence, isolation of a group from a non-finite value in another group's
chunk, and pad channels that are zeros for the next reader."""
import numpy as np
import pytest

import group_models as gm

BAR = 1e-4  # what test_geometry_fixture_matches_pytorch holds the dense kernels of the same width to


@pytest.fixture(scope="module")
def boards(nsg):
    """19 seeded positions and their planes as a float64 tensor, shared by the test-time models."""
    import torch
    bb = nsg.synth.random_batch(19, 86, seed=31)
    x = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64))
    return bb, x


@pytest.fixture(scope="module")
def positions(nsg, golden_dir):
    """The 64 positions of the general-graph fixtures, as bitboards and as float64 planes."""
    import torch
    bb = np.load(f"{golden_dir}/net_graph.npz")["bitboards86"]
    x = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64))
    return bb, x


def max_err(out, ref):
    return max(float(np.abs(np.asarray(o, np.float64).reshape(-1) - np.asarray(r).reshape(-1)).max()) for o, r in zip(out, ref))


def device(nsg, net, path, bb, batches, size=32):
    """Exports `net` and runs it on the device for each batch: [(n, outputs)]."""
    gm.export(net, path)
    ev = nsg.Evaluator(0, size, 86)
    ev.load(str(path))
    assert ev.graph_info()["path"] == "graph"
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    ev.close()
    return outs


def reference(net, x):
    import torch
    with torch.no_grad():
        return [t.numpy() for t in net.double()(x)]


# ---- 1. exact integers -----------------------------------------------------------------------------------------------
EXACT = [(s, 3, 1) for s in gm.SHAPES] + [(s, k, d) for s in ((72, 48, 3), (64, 128, 4)) for k, d in gm.GEOMETRIES]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,k,d", EXACT, ids=gm.sid)
def test_exact_integers(nsg, boards, tmp_path, shape, k, d):
    """Integer stem on the 0/1 planes, integer grouped weights and bias: every partial sum of the grouped conv, in any
    order, is an integer below 2^24 (asserted on the float64 side from the weights), so the policy -- a 0/1 selection of
    27 of its channels, one model per window -- equals the float64 reference.  A wrong chunk range, a wrong weight
    offset, a group read by the wrong wave or a dropped tap cannot pass."""
    import torch
    cin, cout, G = shape
    bb, x = boards
    net = gm.GroupTapNet(cin, cout, G, k, d, seed=cin + cout).eval()
    stem_bound, bound = net.bound()
    assert stem_bound < 2 ** 24 and bound < 2 ** 24, (stem_bound, bound)
    with torch.no_grad():
        y = net.double().grouped(x)
    assert float(y.abs().max()) <= bound and bool((y == y.round()).all())
    assert all(bool((y[:, c] != 0).any()) for c in range(cout))  # every output channel shows something
    for start in gm.windows(cout):
        net.show(start)
        ref = reference(net, x)
        assert np.array_equal(ref[0].reshape(-1, gm.WIN, 81)[:, :min(gm.WIN, cout - start)],
                              y[:, start:start + gm.WIN].reshape(len(bb), -1, 81).numpy())
        for n, o in device(nsg, net, tmp_path / f"exact{start}.onnx", bb, (1, 19)):
            np.testing.assert_array_equal(o[0], ref[0][:n])
            assert max_err(o[1:], [r[:n] for r in ref[1:]]) < BAR


# ---- 2. the bits of the dense kernels ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("shape", [(64, 128, 4), (128, 64, 4), (160, 160, 2)], ids=gm.sid)
def test_same_numbers_as_the_dense_kernel(nsg, boards, tmp_path, shape, k):
    """Cin / group is a multiple of 16 here, so a group's inputs are whole chunks and the grouped chain -- chunks
    ascending, taps row-major, k-steps ascending -- is the chain of a group-1 conv on the group's channel slice.  The twin
    is Split -> one group-1 Conv per group -> Concat: each part is copied into rows of its own (chunks from 0), runs on
    graphConv<9> (3x3) or graphConvGeo (5x5) with the same f32 weights and bias, and is copied back.  All three
    outputs agree bit for bit."""
    import torch
    bb, x = boards
    torch.manual_seed(sum(shape) + k)
    net = gm.randomize(gm.GroupNet(*shape, k), 5).eval()
    twin = gm.twin_of(net).eval()
    with torch.no_grad():
        for a, b in zip(net(x.float()), twin(x.float())):
            assert float((a - b).abs().max()) < 1e-5  # the same function
    ref = reference(net, x)
    og = device(nsg, net, tmp_path / "g.onnx", bb, (1, 19))
    ot = device(nsg, twin, tmp_path / "t.onnx", bb, (1, 19))
    for (n, a), (_, b) in zip(og, ot):
        assert float(np.abs(a[0]).max()) > 1e-3
        err = max_err(a, [r[:n] for r in ref])
        print(shape, k, n, "max abs err against float64", err)
        assert err < BAR
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)


# ---- 3. and 4. a ResNeXt-style net ---------------------------------------------------------------------------------------
_nets = {}


def resnext(G):
    import torch
    if G not in _nets:
        torch.manual_seed(500 + G)
        _nets[G] = gm.randomize(gm.ResNeXtNet(32, G, blocks=3), 60 + G).eval()
    return _nets[G]


@pytest.fixture(scope="module")
def resnext_ref(positions):
    """The float64 outputs of the two nets on the 64 positions, computed once."""
    return {G: reference(resnext(G), positions[1]) for G in (4, 8)}


@pytest.mark.gpu
@pytest.mark.parametrize("G", [4, 8])
def test_resnext_net_matches_pytorch_float64(nsg, positions, resnext_ref, tmp_path, G):
    """Three blocks of 1x1 -> 3x3 grouped -> 1x1 at width 32 with BatchNorm of non-trivial running statistics, residuals,
    ReLU and swish, against float64 PyTorch at the bar of the dense kernels of the same width."""
    ref = resnext_ref[G]
    data = gm.export(resnext(G), tmp_path / "rx.onnx")
    assert b"BatchNormalization" in data
    for n, o in device(nsg, resnext(G), tmp_path / "rx.onnx", positions[0], (1, 6, 17, 64), size=64):
        err = max_err(o, [r[:n] for r in ref])
        print("resnext G", G, "batch", n, "max abs err", err)
        assert float(np.abs(o[0]).max()) > 1e-2
        assert err < BAR, (n, err)


@pytest.mark.gpu
def test_a_board_does_not_depend_on_its_batch(nsg, positions, tmp_path):
    gm.export(resnext(8), tmp_path / "rx.onnx")
    ev = nsg.Evaluator(0, 64, 86)
    ev.load(str(tmp_path / "rx.onnx"))
    bb = positions[0][:37]
    whole = [x.copy() for x in ev.compute_blocking(bb)]
    for b in range(37):
        one = ev.compute_blocking(bb[b:b + 1])
        for x, y in zip(one, whole):
            np.testing.assert_array_equal(x[0], y[b])
    ev.close()


# ---- 5. isolation ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_group_does_not_read_another_groups_chunk(nsg, boards, tmp_path):
    """(64 -> 64, group 4): 16 channels per group, one chunk each.  A constant Add in front of the conv is inf in
    channels 48..63 -- group 3, chunk 3 -- and the policy reads output channels 0..47 only; value and draw read the
    stem in front of the Add.  A wave whose sub-range is its own group's chunk never multiplies an inf: all three
    outputs are finite and have the bits of the model with a zero constant.  A block-diagonal dense lowering, or waves
    that run the whole tile range, give 0 * inf = NaN."""
    import torch
    bb, x = boards
    torch.manual_seed(77)
    clean = gm.randomize(gm.IsolationNet(False), 9).eval()
    poisoned = gm.IsolationNet(True).eval()
    poisoned.load_state_dict({k: v for k, v in clean.state_dict().items() if k != "c"}, strict=False)
    assert bool(torch.isinf(poisoned.c[0, 48:]).all()) and float(poisoned.c[0, :48].abs().max()) == 0.0
    data = gm.export(poisoned, tmp_path / "inf.onnx")
    info = nsg.inspect_onnx(data, 86)
    oc = device(nsg, clean, tmp_path / "zero.onnx", bb, (1, 19))
    op = device(nsg, poisoned, tmp_path / "inf.onnx", bb, (1, 19))
    assert info["path"] == "graph"
    ref = reference(clean, x)
    for (n, a), (_, b) in zip(oc, op):
        assert max_err(a, [r[:n] for r in ref]) < BAR
        for u, v in zip(a, b):
            assert np.isfinite(v).all()
            np.testing.assert_array_equal(u, v)


# ---- 6. pad channels -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("act", ["exp", "recip"])
def test_pad_channels_are_zeros_for_the_next_reader(nsg, boards, tmp_path, act):
    """(24 -> 24, group 3) with an activation fused, read by a dense 3x3 conv whose second chunk holds the pad channels
    24..31.  With Exp a pad that went through applyAct would be 1; with Reciprocal (outputs of the grouped conv kept at 1
    or above by its weights, see PadNet) it would be inf, and inf times the dense conv's zero weight is NaN."""
    import torch
    bb, x = boards
    torch.manual_seed(12)
    net = gm.PadNet(act)
    if act == "exp":
        net = gm.randomize(net, 13)
    net = net.eval()
    ref = reference(net, x)
    if act == "recip":
        with torch.no_grad():
            assert float(net.double().g(torch.relu(net.stem(x))).min()) >= 1.0
    for n, o in device(nsg, net, tmp_path / "pad.onnx", bb, (1, 19)):
        err = max_err(o, [r[:n] for r in ref])
        print("pad channels", act, n, "max abs err", err)
        assert all(np.isfinite(t).all() for t in o)
        assert err < BAR, err
