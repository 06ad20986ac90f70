"""The fused elementwise launch (graphElt) and the shared activation (applyAct) on the device, almost directly: every
model is an exact stem, the ops under test and policy = Flatten(result) with 27 channels, so every element the kernel
writes reaches the test unmixed.  The stem's weights are small integers times a power of two (zero on the four planes
that hold fractions), so its float32 output is exact and the kernel's input is known bit for bit.

Arithmetic is compared bit for bit with the same op sequence in float64 rounded to float32 after every op
(elt_models.Net.run); activations are compared with their float64 definitions in float32 ulps of the reference."""
import numpy as np
import pytest

import elt_models as em

F = em.F


@pytest.fixture(scope="module")
def boards(nsg):
    """The 19 seeded positions of the sibling test files and their planes in float64."""
    bb = nsg.synth.random_batch(19, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def device(nsg, data, bb, tmp_path, batches=(1, 19)):
    path = tmp_path / "m.onnx"
    path.write_bytes(data)
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    ev.close()
    return info, outs


def exact_stem(env, names=("s",), exp=-3):
    """The stem's float64 result is a multiple of 2^exp below 2^24 steps: float32 holds it, in any order of summation;
    and every board has negative, zero and positive values, so the kinks at 0 are hit."""
    for name in names:
        s = env[name] * 2.0 ** -exp
        assert bool((s == np.round(s)).all()) and float(np.abs(s).max()) < 2 ** 24
        for b in range(s.shape[0]):
            assert (s[b] < 0).any() and (s[b] == 0).any() and (s[b] > 0).any(), (name, b)


def heads_close(outs, env64):
    for n, o in outs:
        for got, name in ((o[1], "value"), (o[2], "draw")):
            err = float(np.abs(got.reshape(-1).astype(np.float64) - env64[name][:n].reshape(-1)).max())
            assert err < 1e-4, (name, n, err)


def check_exact(nsg, net, data, boards, tmp_path, stems=("s",)):
    """The policy equals the rounded-per-op reference bit for bit; value and draw are within 1e-4 of float64."""
    bb, x = boards
    ref = net.run(x, rounded=True)
    exact_stem(net.run(x, rounded=False), stems)
    assert np.isfinite(ref["policy"]).all()
    info, outs = device(nsg, data, bb, tmp_path)
    for n, o in outs:
        np.testing.assert_array_equal(o[0], ref["policy"][:n].astype(np.float32))
    heads_close(outs, net.run(x, rounded=False))
    return info, outs


def ulps(got, ref):
    """|got - ref| in float32 ulps of the reference, with one denormal step as the floor of an ulp."""
    ref = np.asarray(ref, np.float64)
    with np.errstate(over="ignore"):
        step = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(step, 2.0 ** -149)


# ---- 1. arithmetic, bit for bit ------------------------------------------------------------------------------------
BINARY = ["Add", "Sub", "Mul", "Div", "Max", "Min"]
SCALAR = [1.37]
CHANNEL = (np.linspace(0.3, 2.9, F) * np.where(np.arange(F) % 3 == 0, -1.0, 1.0)).reshape(F, 1, 1)


def denominator(net, x, tag):
    """abs(x) + 1: never zero."""
    return net.node("Add", [net.node("Abs", [x], tag + "_abs"), net.const(tag + "_one", [1.0])], tag + "_den")


@pytest.mark.gpu
@pytest.mark.parametrize("op", BINARY)
def test_binary_ops_of_two_runtime_tensors(nsg, boards, tmp_path, op):
    """The two halves of the Split: the second operand is read at channel offset 27 of rows of stride 64."""
    net = em.Net(nsg)
    a, b = net.split_stem()
    y = net.node(op, [a, denominator(net, b, "d") if op == "Div" else b], "y")
    check_exact(nsg, net, net.finish(y, a), boards, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("const", ["scalar", "channel"])
@pytest.mark.parametrize("op", BINARY)
def test_binary_ops_with_a_constant(nsg, boards, tmp_path, op, const, side):
    """c - x and x - c, c / x and x / c: the operand order is the node's."""
    net = em.Net(nsg)
    a, b = net.split_stem()
    c = net.const("c", SCALAR if const == "scalar" else CHANNEL)
    x = denominator(net, b, "d") if op == "Div" and side == "left" else b
    y = net.node(op, [c, x] if side == "left" else [x, c], "y")
    check_exact(nsg, net, net.finish(y, a), boards, tmp_path)


def unary_case(net, x, case):
    if case in ("Neg", "Abs"):
        return net.node(case, [x], "y")
    if case == "clip_both":
        return net.node("Clip", [x, net.const("lo", [-1.375]), net.const("hi", [2.125])], "y")
    if case == "clip_lower":
        return net.node("Clip", [x, net.const("lo", [-1.375])], "y")
    if case == "clip_upper":
        return net.node("Clip", [x, "", net.const("hi", [2.125])], "y")
    if case == "leaky_relu":
        return net.node("LeakyRelu", [x], "y", alpha=0.1)
    if case == "prelu_scalar":
        return net.node("PRelu", [x, net.const("slope", [0.3])], "y")
    if case == "prelu_channel":
        return net.node("PRelu", [x, net.const("slope", np.linspace(-0.5, 1.5, F).reshape(F, 1, 1))], "y")
    assert case == "batchnorm"  # on a Split half: no conv to fold it into
    rng = np.random.default_rng(3)
    for name, v in (("gm", rng.uniform(0.5, 2.0, F)), ("bt", rng.normal(size=F)), ("mn", rng.normal(size=F)), ("vr", rng.uniform(0.5, 2.0, F))):
        net.const(name, v)
    return net.node("BatchNormalization", [x, "gm", "bt", "mn", "vr"], "y", epsilon=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["Neg", "Abs", "clip_both", "clip_lower", "clip_upper", "leaky_relu", "prelu_scalar",
                                  "prelu_channel", "batchnorm"])
def test_unary_ops_and_the_clamp_family(nsg, boards, tmp_path, case):
    """On the second half of the Split (kSrcSame at channel offset 27).  The stem has zeros and both signs on every
    board (asserted), and the bounds lie on its grid of 1/8: x == 0 and x == a bound occur."""
    net = em.Net(nsg)
    a, b = net.split_stem()
    y = unary_case(net, b, case)
    bb, x = boards
    s = net.run(x)["b"]
    assert (s == -1.375).any() and (s == 2.125).any() and (s == 0).any()
    check_exact(nsg, net, net.finish(y, a), boards, tmp_path)


# ---- 2. source modes ---------------------------------------------------------------------------------------------
def board_vector(net, a):
    """[N,27,1,1] from mean -> Gemm with a signed permutation matrix times 2^-1: exact given the mean, whatever the
    order of the dense kernel's sum.  The mean itself is the exact sum of 81 multiples of 1/8 divided by 81 once."""
    perm = np.random.default_rng(5).permutation(F)
    w = np.zeros((F, F))
    w[np.arange(F), perm] = np.where(np.arange(F) % 2 == 0, 0.5, -0.5)
    net.node("GlobalAveragePool", [a], "se_gp")
    net.node("Flatten", ["se_gp"], "se_flat", axis=1)
    net.node("Gemm", ["se_flat", net.const("se_w", w)], "se_fc", transB=1)
    return net.node("Unsqueeze", ["se_fc", net.const("se_axes", [2, 3], np.int64)], "g4")


@pytest.mark.gpu
def test_a_flat_tensor_broadcast_over_the_squares(nsg, boards, tmp_path):
    """kSrcBoard: x[n, c, sq] * g[n, c].  The reference indexes g by board and channel on its own."""
    net = em.Net(nsg)
    a, b = net.split_stem()
    y = net.node("Mul", [b, board_vector(net, a)], "y")
    bb, x = boards
    env = net.run(x)
    want = em.f32(env["b"] * env["se_fc"][:, :, None, None]).reshape(len(bb), -1)
    assert np.array_equal(want, env["y"].reshape(len(bb), -1)) and len(np.unique(env["se_fc"])) > 100
    check_exact(nsg, net, net.finish(y, a), boards, tmp_path)


@pytest.mark.gpu
def test_an_open_flat_group_inlined_into_a_spatial_one(nsg, boards, tmp_path):
    """sigmoid(fc(mean) * 0.5) * x: the flat group's sources become kSrcBoard inside the spatial launch.  The
    sigmoid's argument is exact; its result is within SIGMOID ulps, which is at most 2 SIGMOID half-ulps of the
    product's relative error, and the product is rounded once more: 2 * bound + 1 ulps of the float64 product."""
    net = em.Net(nsg)
    a, b = net.split_stem()
    t = net.node("Mul", [board_vector(net, a), net.const("half", [0.5])], "t")
    y = net.node("Mul", [net.node("Sigmoid", [t], "h"), b], "y")
    bb, x = boards
    env = net.run(x)
    want = (em.ACT64["sigmoid"](env["t"]) * env["b"]).reshape(len(bb), -1)
    info, outs = device(nsg, net.finish(y, a), bb, tmp_path)
    heads_close(outs, net.run(x, rounded=False))
    worst = max(float(ulps(o[0], want[:n]).max()) for n, o in outs)
    print("inlined flat group: max ulps", worst)
    assert worst <= 2 * ACT_ULPS["sigmoid"] + 1, worst


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["spatial", "token"])
def test_a_constant_per_square_and_channel(nsg, boards, tmp_path, kind):
    """kSrcSquareChannel: a [27,9,9] constant on a spatial tensor (the Split half at offset 27) and an [81,27] constant
    on a token tensor.  Every entry differs, so a transposed or shifted index cannot pass."""
    net = em.Net(nsg)
    a, b = net.split_stem()
    if kind == "spatial":
        pos = (np.arange(F)[:, None] * 81 + np.arange(81)[None, :]).reshape(F, 9, 9) * 2.0 ** -4
        y = net.node("Add", [b, net.const("pos", pos)], "y")
    else:
        pos = (np.arange(81)[:, None] * F + np.arange(F)[None, :]) * 2.0 ** -4
        net.node("Reshape", [b, net.const("to3", [-1, F, 81], np.int64)], "b3")
        net.node("Transpose", ["b3"], "tok", perm=[0, 2, 1])
        net.node("Add", ["tok", net.const("pos", pos)], "tok2")
        y = net.node("Transpose", ["tok2"], "y", perm=[0, 2, 1])
    bb, x = boards
    env = net.run(x)
    table = pos.reshape(F, 81) if kind == "spatial" else pos.T  # [channel][square]
    want = em.f32(env["b"].reshape(len(bb), F, 81) + table[None]).reshape(len(bb), -1)
    assert np.array_equal(want, env["y"].reshape(len(bb), -1))
    check_exact(nsg, net, net.finish(y, a), boards, tmp_path)


# ---- 3. every Act code, body and tails ---------------------------------------------------------------------------
# The largest error measured on an MI355X against the float64 definitions, in float32 ulps of the reference, the same
# in both placements (body: about +-8 in steps of 1/8; the tails, the same grid times 2^10, stay below 0.04 ulps
# everywhere).  The tests assert twice these, for compiler drift in expf / erff / erfcf / tanhf / log1pf; the
# piecewise-linear ones are held to 1 ulp (measured: relu and relu6 0, hardswish and hardsigmoid 0.67).
#   sigmoid 1.28   tanh 0.67   swish 0.99   softplus 1.02   erf 0.66   gelu 35.93
# GELU's error is its argument's: v / sqrt(2) is rounded once, and erfc(x) far out changes by 2 x^2 ulps per ulp of
# x (x = 4.4 at v = -6.25).  Computed as 0.5 v (1 + erff(x)) it was 1.5e7 ulps: zero from v = -5.7 on.  Computed as
# v / 6 + 0.5 the hard sigmoid was 8 to 11 ulps off around its knee at -3, the hard swish 11 to 15.
MEASURED_ULPS = {"sigmoid": 1.28, "tanh": 0.67, "swish": 0.99, "softplus": 1.02, "erf": 0.66, "gelu": 35.93}
ACT_ULPS = {k: 2 * v for k, v in MEASURED_ULPS.items()}
ACT_ULPS.update(relu=1, relu6=1, hardswish=1, hardsigmoid=1)


def act_nodes(net, x, act):
    if act in ("relu", "sigmoid", "tanh", "softplus", "erf"):
        return net.node({"relu": "Relu", "sigmoid": "Sigmoid", "tanh": "Tanh", "softplus": "Softplus", "erf": "Erf"}[act], [x], "y")
    if act == "swish":
        return net.node("Mul", [x, net.node("Sigmoid", [x], "sg")], "y")
    if act == "gelu":  # the exporter's exact GELU
        e = net.node("Erf", [net.node("Div", [x, net.const("sqrt2", [np.sqrt(2.0)])], "xd")], "xe")
        return net.node("Mul", [net.node("Mul", [x, net.node("Add", [e, net.const("one", [1.0])], "e1")], "xm"), net.const("half", [0.5])], "y")
    if act == "relu6":
        return net.node("Clip", [x, net.const("zero", [0.0]), net.const("six", [6.0])], "y")
    if act == "hardswish":
        return net.node("HardSwish", [x], "y")
    assert act == "hardsigmoid"
    return net.node("HardSigmoid", [x], "y", alpha=1.0 / 6.0, beta=0.5)


def act_model(nsg, act, where):
    """Channels 0-13 of the stem span about +-8 in steps of 1/8, channels 14-26 are the same grid times 2^10 (the
    tails).  where = "epilogue": the activation is the conv's only consumer; "chain": behind -(-s), which no conv
    absorbs, so it is an instruction of the elementwise program on the same exact input.  The heads read a stem of
    their own."""
    net = em.Net(nsg)
    net.stem(seed=2, span=4)
    net.consts["s_w"][14:] *= 2.0 ** 10
    net.consts["s_b"][14:] *= 2.0 ** 10
    x = "s" if where == "epilogue" else net.node("Neg", [net.node("Neg", ["s"], "n1")], "n2")
    y = act_nodes(net, x, act)
    net.stem(seed=4, out="hs")
    return net, net.finish(y, "hs")


def measure_act(nsg, boards, tmp_path, act, where):
    bb, x = boards
    net, data = act_model(nsg, act, where)
    s = net.run(x, rounded=False)["s"]
    g = s * 8
    assert bool((g == np.round(g)).all()) and float(np.abs(g).max()) < 2 ** 24
    body, tail = s[:, :14], s[:, 14:]
    assert body.min() <= -6 and body.max() >= 6 and np.abs(body).max() <= 16 and np.abs(tail).max() >= 4096
    want = em.ACT64[act](s).reshape(len(bb), -1)
    info, outs = device(nsg, data, bb, tmp_path)
    worst = {"body": 0.0, "tail": 0.0}
    for n, o in outs:
        assert np.isfinite(o[0][np.isfinite(want[:n])]).all()
        u = ulps(o[0], want[:n]).reshape(n, F, 81)
        worst = {"body": max(worst["body"], float(u[:, :14].max())), "tail": max(worst["tail"], float(u[:, 14:].max()))}
    heads_close(outs, net.run(x, rounded=False))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["epilogue", "chain"])
@pytest.mark.parametrize("act", list(ACT_ULPS))
def test_activations_in_ulps(nsg, boards, tmp_path, act, where):
    worst = measure_act(nsg, boards, tmp_path, act, where)
    print(act, where, "max ulps", worst)
    assert max(worst.values()) <= ACT_ULPS[act], (act, where, worst)


# ---- 4. chains at and over the limits -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family,length", [("scalar_mul", 7), ("scalar_mul", 8), ("scalar_mul", 9), ("scalar_mul", 15),
                                           ("pooled_sum", 8), ("pooled_sum", 9), ("pooled_sum", 10),
                                           ("unary_binary", 13), ("unary_binary", 14), ("unary_binary", 15)])
def test_chains_at_and_over_the_limits(nsg, boards, tmp_path, family, length):
    net, data = em.family_model(nsg, family, length)
    check_exact(nsg, net, data, boards, tmp_path)


@pytest.mark.gpu
def test_a_cut_chain_gives_the_bits_of_the_fused_one(nsg, boards, tmp_path):
    """Six scalar Mul nodes as one launch, and again with the heads reading the third tensor, which cuts the chain
    there: one launch more, the same policy."""
    fused = em.Net(nsg)
    s = fused.stem()
    one = check_exact(nsg, fused, fused.finish(em.scalar_mul_chain(fused, s, 6), s), boards, tmp_path)
    cut = em.Net(nsg)
    s = cut.stem()
    two = check_exact(nsg, cut, cut.finish(em.scalar_mul_chain(cut, s, 6), "m2"), boards, tmp_path)
    assert two[0]["launches"] == one[0]["launches"] + 1
    for (n, o1), (_, o2) in zip(one[1], two[1]):
        np.testing.assert_array_equal(o1[0], o2[0])
