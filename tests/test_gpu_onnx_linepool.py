"""Rank and file pooling (graphLinePool) and the line tensors behind it on the device, almost directly: an exact stem
(elt_models.Net.stem: small integers times 2^-3, so its float32 output is known bit for bit), the ops under test, and
policy = Flatten(result) with 27 channels, so every element reaches the test unmixed.  A line is shown by broadcasting
it back onto the board: result = 0 * s + line (exact for finite s).  Batches of 1, 3 and 19 boards.

The mean's reference is the order contract itself: the float64 sum of the line's nine elements rounded to float32 (the
sum is exact, so the order cannot show), divided by float32 9 and rounded once.  The max is exact."""
import numpy as np
import pytest

import elt_models as em
import line_models as lm

F = em.F
BATCHES = (1, 3, 19)


@pytest.fixture(scope="module")
def boards(nsg):
    bb = nsg.synth.random_batch(19, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def device(nsg, data, bb, tmp_path, batches=BATCHES, alone=None):
    path = tmp_path / "m.onnx"
    path.write_bytes(data)
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    single = None if alone is None else [o.copy() for o in ev.compute_blocking(bb[alone:alone + 1])]
    ev.close()
    return info, outs, single


def exact_stem(s, exp=-3):
    g = s * 2.0 ** -exp
    assert bool((g == np.round(g)).all()) and float(np.abs(g).max()) < 2 ** 20


def ulps(got, ref):
    ref = np.asarray(ref, np.float64)
    step = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(step, 2.0 ** -149)


def shown(net, s, line):
    """[N,C,9,9] = 0 * s + line: the line broadcast back onto the board, exactly."""
    zero = net.node("Mul", [s, net.const("zero", [0.0])], "zeros")
    return net.node("Add", [zero, line], "shown")


# ---- 1. bit for bit: orientations, modes, forms, pad channels, Split parts, broadcast through Mul and Add ----------------
SHAPES = {"c24_pad": (27, 0, 24), "c40_off20_scalar": (40, 20, 20), "c40_off16_vector": (40, 16, 24)}
COMBINE = [("Mul", False), ("Add", True), ("Mul", True), ("Add", False)]  # (op, line first)


def pooled_model(nsg, shape, how, files, k):
    W, off, cp = SHAPES[shape]
    net = lm.LNet(nsg)
    s = net.stem(W)
    sizes = [z for z in (off, cp, W - off - cp) if z > 0]
    outs = [f"part{i}" for i in range(len(sizes))]
    net.const("sizes", sizes, np.int64)
    net.node("Split", [s, "sizes"], outs, name="split", axis=1)
    b = outs[1 if off > 0 else 0]
    net.const("fill_sizes", [F - cp, W - F + cp], np.int64)
    net.node("Split", [s, "fill_sizes"], ["fill", "rest"], name="fill_split", axis=1)
    line = net.line(b, "line", how, files)
    op, first = COMBINE[k % 4]
    y = net.node(op, [line, b] if first else [b, line], "y")
    cat = net.node("Concat", [y, "fill"], "cat", axis=1)
    net.node("Flatten", [cat], "policy", name="pflat", axis=1)
    net.heads(cat)  # (value and draw need 27 channels; they are not what this model is about)
    return net, net.data()


CASES = [(sh, how, files) for sh in SHAPES for how in ("mean", "max", "avgpool", "maxpool") for files in (False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{sh}-{how}-{'files' if f else 'ranks'}" for sh, how, f in CASES])
def test_lines_equal_the_order_contract_bit_for_bit(nsg, boards, tmp_path, k):
    shape, how, files = CASES[k]
    net, data = pooled_model(nsg, shape, how, files, k)
    bb, x = boards
    exact_stem(net.run(x, rounded=False)["s"])
    ref = net.run(x, rounded=True)["policy"].astype(np.float32)
    assert np.isfinite(ref).all()
    info, outs, single = device(nsg, data, bb, tmp_path, alone=7)
    for n, o in outs:
        np.testing.assert_array_equal(o[0], ref[:n])
    # board 7 of 19 and the same board run alone: the same bits
    np.testing.assert_array_equal(single[0][0], outs[-1][1][0][7])


# ---- 2. against graphPool: a 1x9 window with pads 4 holds the whole rank at file 4 -------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("files", [False, True])
def test_the_line_max_equals_graphpool_where_its_window_holds_the_line(nsg, boards, tmp_path, files):
    net = lm.LNet(nsg)
    s = net.stem()
    ks, pads = ([9, 1], [4, 0, 4, 0]) if files else ([1, 9], [0, 4, 0, 4])
    p = net.node("MaxPool", [s], "p", kernel_shape=ks, pads=pads, strides=[1, 1])
    m = net.line(s, "m", "max", files)
    data = net.finish(net.node("Sub", [p, m], "d"), s)
    bb, x = boards
    ref = net.run(x, rounded=True)["policy"].astype(np.float32)
    info, outs, _ = device(nsg, data, bb, tmp_path)
    for n, o in outs:
        d = o[0].reshape(n, F, 9, 9)
        centre = d[:, :, 4, :] if files else d[:, :, :, 4]
        assert (centre == 0).all() and (d <= 0).all() and (d < 0).any()
        np.testing.assert_array_equal(o[0], ref[:n])


# ---- 3. values that expose a wrong neighbour or a wrong pad ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("how", ["mean", "max"])
@pytest.mark.parametrize("files", [False, True])
def test_infinities_stay_in_their_own_line(nsg, boards, tmp_path, how, files):
    """Channel 5 is -inf except on square (3, 6); channel 10 is +inf on the last rank; channel 26, the last one before
    the pad channels, is -inf on the last file."""
    k = np.zeros((F, 9, 9))
    k[5] = -np.inf
    k[5, 3, 6] = 0.0
    k[10, 8, :] = np.inf
    k[26, :, 8] = -np.inf
    net = lm.LNet(nsg)
    s = net.stem()
    t = net.node("Add", [s, net.const("k", k)], "t")
    data = net.finish(shown(net, s, net.line(t, "line", how, files)), s)
    bb, x = boards
    ref = net.run(x, rounded=True)["policy"].astype(np.float32)
    assert not np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).any()
    r = ref.reshape(-1, F, 9, 9)
    assert np.isfinite(r[:, 5, 3, :] if not files else r[:, 5, :, 6]).all() == (how == "max")  # the one open square
    info, outs, _ = device(nsg, data, bb, tmp_path)
    for n, o in outs:
        np.testing.assert_array_equal(o[0], ref[:n])


# ---- 4. Exp and Reciprocal on a line tensor; pad channels stay zero in front of a conv ---------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("act", ["Reciprocal", "Exp"])
def test_activations_on_a_line_tensor_and_its_pad_channels(nsg, boards, tmp_path, act):
    """27 channels in rows of 32: a pad channel holding 1 / 0 = inf would meet the next conv's zero weights as NaN."""
    net = lm.LNet(nsg)
    s = net.stem()
    m = net.line(s, "m", "mean")
    if act == "Reciprocal":
        a = net.node("Reciprocal", [net.node("Add", [net.node("Abs", [m], "ab"), net.const("one", [1.0])], "den")], "a")
    else:
        a = net.node("Exp", [m], "a")
    net.const("eye", np.eye(F).reshape(F, F, 1, 1))
    c = net.node("Conv", [a, "eye"], "c", kernel_shape=[1, 1])
    data = net.finish(shown(net, s, c), s)
    bb, x = boards
    # arithmetic rounded per op as the kernels round it, the activation itself in float64: the conv behind it rounds once
    ref = net.run(x, rounded=True)["policy"]
    info, outs, _ = device(nsg, data, bb, tmp_path)
    assert info["conv_launches"] == 4  # the stem, the conv on the line tensor, value and draw
    for n, o in outs:
        assert np.isfinite(o[0]).all()
        worst = float(ulps(o[0], ref[:n]).max())
        print(f"{act} on a line tensor, {n} boards: {worst:.2f} ulps")
        # Reciprocal is the correctly rounded division (0.5 ulp of the float64 value); Exp is held to twice its measured 0.58
        assert worst <= (0.5 if act == "Reciprocal" else 1.16), worst


# ---- 5. the 18-line path ----------------------------------------------------------------------------------------------
def eighteen(nsg, which):
    rng = np.random.default_rng(5)
    net = lm.LNet(nsg)
    s = net.stem()
    xh = net.line(s, "xh", "max", False)
    xw = net.node("Transpose", [net.line(s, "xw", "max", True)], "xwt", perm=[0, 1, 3, 2])
    cat = net.node("Concat", [xh, xw], "cat", axis=2)
    net.const("w1", rng.integers(-1, 2, size=(8, F, 1, 1)))
    net.const("b1", rng.integers(-8, 9, size=8) / 8.0)
    z = net.node("Conv", [cat, "w1", "b1"], "z", kernel_shape=[1, 1])
    # var + eps = 1 exactly: the folded scale is gamma, a power of two
    for name, v in (("gm", 2.0 ** rng.integers(-1, 2, size=8)), ("bt", rng.integers(-8, 9, size=8) / 8.0),
                    ("mn", rng.integers(-8, 9, size=8) / 8.0), ("vr", np.full(8, 1.0 - 2.0 ** -10))):
        net.const(name, v)
    bn = net.node("BatchNormalization", [z, "gm", "bt", "mn", "vr"], "bn", epsilon=2.0 ** -10)
    h = net.node("HardSwish", [bn], "h")
    net.const("nine", [9, 9], np.int64)
    yh, yw = net.node("Split", [h, "nine"], ["yh", "yw"], name="split", axis=2)
    # selections with a factor of +-1 or +-2: one term per output, so the gate conv's sum is exact
    sel = np.zeros((2, F, 8, 1, 1))
    for j in range(2):
        sel[j, np.arange(F), rng.integers(0, 8, size=F), 0, 0] = rng.choice([-2.0, -1.0, 1.0, 2.0], size=F)
    net.const("wh", sel[0])
    net.const("ww", sel[1])
    ah = net.node("Sigmoid", [net.node("Conv", [yh, "wh"], "ch", kernel_shape=[1, 1])], "ah")
    ywt = net.node("Transpose", [yw], "ywt", perm=[0, 1, 3, 2])
    aw = net.node("Sigmoid", [net.node("Conv", [ywt, "ww"], "cw", kernel_shape=[1, 1])], "aw")
    return net, net.finish(shown(net, s, ah if which == "h" else aw), s), sel[0 if which == "h" else 1]


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["h", "w"])
def test_the_eighteen_line_path(nsg, boards, tmp_path, which):
    """Concat, shared conv + BatchNorm + hardswish, Split, gate conv + sigmoid.  The shared conv's sums are exact
    (maxima on the stem's grid, integer weights, a power-of-two BatchNorm), so hardswish meets its exact argument and
    is held to 1 ulp; the gate conv multiplies one such value by +-1 or +-2, so the sigmoid's argument is off by at most
    |w| ulp(h), which its slope (at most 1/4) carries into the result beside its own 2 x 1.28 ulps."""
    net, data, sel = eighteen(nsg, which)
    bb, x = boards
    env = net.run(x, rounded=False)
    exact_stem(env["bn"], exp=-4)  # gamma = 1/2 halves the grid of 1/8
    ref = env["policy"]
    half = env["yh"] if which == "h" else env["ywt"]  # [N,8,9,1] or [N,8,1,9]
    w = np.abs(sel[:, :, 0, 0])                      # [27,8]
    arg_err = np.einsum("oc,ncyx->noyx", w, np.spacing(np.abs(half).astype(np.float32)).astype(np.float64))
    bound = np.broadcast_to(0.25 * arg_err, (len(x), F, 9, 9)).reshape(len(x), -1) + 2.56 * np.spacing(ref.astype(np.float32)).astype(np.float64)
    info, outs, _ = device(nsg, data, bb, tmp_path)
    # the stem, the shared conv, the two gate convs, value, draw; beside them the two poolings (the Concat is theirs),
    # the copies of the two 9-line views, the broadcast, the mean, planes and outputs
    assert info["conv_launches"] == 6 and info["launches"] == 6 + 2 + 2 + 1 + 1 + 2
    for n, o in outs:
        err = np.abs(o[0].astype(np.float64) - ref[:n])
        share = float((err / bound[:n]).max())
        print(f"18-line path, gate {which}, {n} boards: {share:.3f} of the bound")
        assert share <= 1.0, share


# ---- 6. the whole coordinate-attention net, random weights, against float64 torch -------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["reduce", "max"])
def test_a_coordinate_attention_net_against_float64(nsg, boards, tmp_path, form):
    import os
    import sys
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_onnx_norm_golden as gen
    net = lm.randomize(lm.coord_att_net(form), 11)
    data = gen.export_model(net, str(tmp_path / "ca.onnx"), fold=False, opset=17)
    bb, x = boards
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(torch.from_numpy(x))]
    net.float()
    vals, errs = lm.ca_forward(net.double(), x)
    for a, b in zip(vals, ref):  # the numpy restatement that carries the bound is the torch module
        np.testing.assert_allclose(a.reshape(b.shape), b, rtol=0, atol=1e-12)
    info, outs, _ = device(nsg, data, bb, tmp_path)
    for n, o in outs:
        for got, r, e, name in zip(o, ref, errs, ("policy", "value", "draw")):
            err = np.abs(got.reshape(n, -1).astype(np.float64) - r[:n].reshape(n, -1))
            # the evaluator's own float32 store of the result: half an ulp more
            bound = e[:n].reshape(n, -1) + 0.5 * np.spacing(np.abs(r[:n]).astype(np.float32)).astype(np.float64).reshape(n, -1)
            share = float((err / bound).max())
            print(f"coordinate attention ({form}), {name}, {n} boards: {share:.2e} of the derived bound")
            assert share <= 1.0, (name, share)
