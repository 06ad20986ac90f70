"""Exp, Log, Sqrt, Reciprocal, Pow, Mish, tanh-GELU and softsign on the device: the maths fixture against its float64
PyTorch outputs, batch independence and the evaluator contract on it; every op almost directly, in the harness of
tests/test_gpu_onnx_elementwise.py (an exact stem puts a known grid of values into the tensor, then the op, then
policy = Flatten(result)), bit for bit where the arithmetic is correctly rounded and in float32 ulps of the float64
definition where it is not; the tails of Mish and tanh-GELU; pad channels behind Reciprocal and Exp; a width sweep of the
fused conv -> BN -> Mish."""
import os
import sys

import numpy as np
import pytest

import elt_models as em

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

NAME = "net_graph_math"
F = em.F
SMALLEST_NORMAL = 2.0 ** -126


@pytest.fixture(scope="module")
def gen():
    import make_onnx_math_golden
    return make_onnx_math_golden


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(f"{golden_dir}/net_math.npz"))
    g["bitboards"] = np.load(f"{golden_dir}/net_graph.npz")["bitboards86"]
    g[f"{NAME}_policy"] = np.concatenate([np.load(f"{golden_dir}/{NAME}_policy_{h}.npz")["policy"] for h in range(2)])
    return g


@pytest.fixture(scope="module")
def boards(nsg):
    """The 19 seeded positions of the sibling test files and their planes in float64."""
    bb = nsg.synth.random_batch(19, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def max_err(out, ref):
    return max(float(np.abs(np.asarray(o, np.float64).reshape(-1) - np.asarray(r).reshape(-1)).max()) for o, r in zip(out, ref))


def device_outputs(nsg, path, bb, batches=(1, 19)):
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    ev.close()
    return outs


def ulps(got, ref):
    """|got - ref| in float32 ulps of the reference, with one denormal step as the floor of an ulp."""
    ref = np.asarray(ref, np.float64)
    with np.errstate(over="ignore"):
        step = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(step, 2.0 ** -149)


# ---- 1. the fixture ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_math_fixture_matches_pytorch(nsg, golden_dir, golden):
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
def test_evaluator_contract_on_the_math_fixture(nsg, golden_dir, golden):
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


# ---- 2. every op, almost directly ----------------------------------------------------------------------------------
# The stem of tests/test_gpu_onnx_elementwise.py's activation tests: channels 0-7 span about +-8 in steps of 1/8 (the
# body), channels 14-26 are the same grid times 2^10 (the tail), and here channels 8-13 are constant: +-20, +-90, +-1e4.
# "signed" ops read it as it is; "positive" ops read |s| + c with c = 1/8 on the body, 128 on the tail (which stays the
# body times 2^10 exactly) and 0 on the constants; Exp reads min(s, 88), which keeps it finite.
SPECIAL = [20.0, -20.0, 90.0, -90.0, 1.0e4, -1.0e4]
BODY, SPEC, TAIL = slice(0, 8), slice(8, 14), slice(14, F)


def softplus64(a):
    return np.logaddexp(0.0, a)


def gelu_tanh64(a):
    """0.5 a (1 + tanh(u)) with 1 + tanh(u) = 2 / (1 + exp(-2u)): the definition without float64's own cancellation
    (1 + tanh(u) is 0 in float64 from u = -19 on)."""
    with np.errstate(over="ignore"):
        return a / (1.0 + np.exp(-2.0 * np.sqrt(2.0 / np.pi) * (a + 0.044715 * a ** 3)))


def pow_case(e, operand, exact):
    return (lambda net, x: net.node("Pow", [x, net.const("e", [e])], "y"), lambda a: a ** e, operand, exact, False)


def softsign_nodes(net, x):
    return net.node("Div", [x, net.node("Add", [net.node("Abs", [x], "ab"), net.const("one", [1.0])], "den")], "y")


def mish_nodes(net, x):
    return net.node("Mul", [x, net.node("Tanh", [net.node("Softplus", [x], "sp")], "th")], "y")


def gelu_tanh_nodes(net, x):
    """The exporter's nine nodes."""
    x3 = net.node("Mul", [net.node("Mul", [x, x], "x2"), x], "x3")
    u = net.node("Mul", [net.node("Add", [x, net.node("Mul", [x3, net.const("k3", [0.044715])], "c3")], "in"),
                         net.const("k", [0.7978845608028654])], "u")
    t1 = net.node("Add", [net.node("Tanh", [u], "th"), net.const("one", [1.0])], "t1")
    return net.node("Mul", [net.node("Mul", [x, t1], "xt"), net.const("half", [0.5])], "y")


# name: (nodes, float64 definition, operand, exact, has an epilogue form)
CASES = {
    "sqrt": (lambda net, x: net.node("Sqrt", [x], "y"), np.sqrt, "positive", True, True),
    "reciprocal": (lambda net, x: net.node("Reciprocal", [x], "y"), lambda a: 1.0 / a, "positive", True, True),
    "pow_2": pow_case(2.0, "signed", True),
    "pow_3": pow_case(3.0, "signed", True),
    "pow_4": pow_case(4.0, "signed", True),
    "pow_-1": pow_case(-1.0, "positive", True)[:4] + (True,),
    "pow_0.5": pow_case(0.5, "positive", True)[:4] + (True,),
    "pow_-2": pow_case(-2.0, "positive", True),
    # three steps, each rounded once: |v| is exact, 1 + |v| and the quotient are the correctly rounded ones
    "softsign": (softsign_nodes, lambda a: a / em.f32(1.0 + np.abs(a)), "signed", True, True),
    "exp": (lambda net, x: net.node("Exp", [x], "y"), np.exp, "capped", False, True),
    "log": (lambda net, x: net.node("Log", [x], "y"), np.log, "positive", False, True),
    "pow_1.5": pow_case(1.5, "positive", False),
    "pow_-0.75": pow_case(-0.75, "positive", False),
    "mish": (mish_nodes, lambda a: a * np.tanh(softplus64(a)), "signed", False, True),
    "gelu_tanh": (gelu_tanh_nodes, gelu_tanh64, "signed", False, True),
}
EXACT = [k for k, c in CASES.items() if c[3]]
MEASURED = [k for k, c in CASES.items() if not c[3]]

# The largest error measured on an MI355X against the float64 definitions, in float32 ulps of the reference, over the
# body, the constants and the tail, the same in both placements.  The tests assert twice these, for compiler drift in
# expf / logf / powf.
#   exp 0.58 (body; tail 0.11)   log 2.07 (tail; body 1.85)   pow_1.5 0.96   pow_-0.75 0.90
#   mish 6.32: at v = -90, where expf(v) = 8e-40 is a denormal of 19 bits and Mish(v) = v expf(v) inherits its rounding;
#              2.32 on the body, below 1e-8 on the tail (v or -0 there)
#   gelu_tanh 8.03: on the body's negative side, the argument's error as for the exact GELU: exp(-2u) changes by
#              2|u| ulps per ulp of u (u = -19 at v = -7); 0 on the constants and the tail
MEASURED_ULPS = {"exp": 0.58, "log": 2.07, "pow_1.5": 0.96, "pow_-0.75": 0.90, "mish": 6.32, "gelu_tanh": 8.03}


def math_model(nsg, case, where):
    """where = "epilogue": the operand goes through a 1x1 conv with the identity as its weight (exact), whose only
    consumer is the op; "chain": the op is an instruction of the elementwise program behind the operand's own nodes
    (behind -(-s) for a signed operand, which no conv absorbs).  The heads read a stem of their own.  Returns the net,
    the model's bytes and the operand's float64 values."""
    nodes, _, operand, _, _ = CASES[case]
    net = em.Net(nsg)
    net.stem(seed=2, span=4)
    net.consts["s_w"][TAIL] *= 2.0 ** 10
    net.consts["s_b"][TAIL] *= 2.0 ** 10
    net.consts["s_w"][SPEC] = 0
    net.consts["s_b"][SPEC] = np.asarray(SPECIAL, np.float32)
    x = "s"
    if operand == "positive":
        shift = np.full((F, 1, 1), 0.125)
        shift[SPEC], shift[TAIL] = 0.0, 128.0
        x = net.node("Add", [net.node("Abs", ["s"], "sa"), net.const("shift", shift)], "pos")
    elif operand == "capped":
        x = net.node("Min", ["s", net.const("cap", [88.0])], "capped")
    elif where == "chain":
        x = net.node("Neg", [net.node("Neg", ["s"], "n1")], "n2")
    if where == "epilogue":
        net.const("eye", np.eye(F).reshape(F, F, 1, 1))
        x = net.node("Conv", [x, "eye"], "ident", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
    pre = len(net.nodes)
    y = nodes(net, x)
    net.stem(seed=4, out="hs")
    return net, net.finish(y, "hs"), x, pre


def operand_values(net, x, name, pre):
    """The operand in float64, from the nodes in front of the op (all exact: a conv on the grid, Abs, Neg, Min, an Add
    on the grid, the identity conv)."""
    full = net.nodes
    net.nodes = full[:pre]
    try:
        env = net.run(x, rounded=False)
    finally:
        net.nodes = full
    s, v = env["s"], env[name]
    g = s[:, BODY] * 8
    assert bool((g == np.round(g)).all()) and np.abs(s[:, BODY]).max() <= 16 and s[:, BODY].min() <= -6 and s[:, BODY].max() >= 6
    assert np.array_equal(s[:, SPEC], np.broadcast_to(np.asarray(SPECIAL).reshape(1, 6, 1, 1), s[:, SPEC].shape))
    t = s[:, TAIL] / 128
    assert bool((t == np.round(t)).all()) and 4096 <= np.abs(s[:, TAIL]).max() <= 16 * 1024 and np.array_equal(em.f32(v), v)
    return v


def run_case(nsg, boards, tmp_path, case, where):
    bb, x = boards
    net, data, operand, pre = math_model(nsg, case, where)
    v = operand_values(net, x, operand, pre)
    with np.errstate(over="ignore", divide="ignore"):
        want = CASES[case][1](v)
    assert np.isfinite(want).all()
    (tmp_path / "m.onnx").write_bytes(data)
    outs = device_outputs(nsg, tmp_path / "m.onnx", bb)
    # the heads read a stem of their own: value and draw against float64
    heads = em.Net(nsg)
    heads.stem(seed=4, out="hs")
    heads.heads("hs")
    env = heads.run(x, rounded=False)
    for n, o in outs:
        assert max_err(o[1:], [env["value"][:n], env["draw"][:n]]) < 1e-4
    return v, want.reshape(len(bb), -1), outs


def placements(case):
    return ["epilogue", "chain"] if CASES[case][4] else ["chain"]


@pytest.mark.gpu
@pytest.mark.parametrize("case,where", [(c, w) for c in EXACT for w in placements(c)])
def test_correctly_rounded_ops_bit_for_bit(nsg, boards, tmp_path, case, where):
    """0 ulps: the float64 definition rounded to float32.  sqrtf and the division are correctly rounded; x ** 2, 3, 4
    are products whose first factor is exact on this grid (its squares and cubes fit 24 bits), so one rounding remains;
    x ** -2 is the exact square and one division."""
    v, want, outs = run_case(nsg, boards, tmp_path, case, where)
    for n, o in outs:
        np.testing.assert_array_equal(o[0], want[:n].astype(np.float32))


def worst_ulps(outs, want):
    worst = {"body": 0.0, "special": 0.0, "tail": 0.0}
    for n, o in outs:
        assert not np.isnan(o[0]).any()
        u = ulps(o[0], want[:n]).reshape(n, F, 81)
        for key, sl in (("body", BODY), ("special", SPEC), ("tail", TAIL)):
            worst[key] = max(worst[key], float(u[:, sl].max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case,where", [(c, w) for c in MEASURED for w in placements(c)])
def test_the_other_ops_in_ulps(nsg, boards, tmp_path, case, where):
    v, want, outs = run_case(nsg, boards, tmp_path, case, where)
    worst = worst_ulps(outs, want)
    print(case, where, "max ulps", worst)
    assert max(worst.values()) <= 2 * MEASURED_ULPS[case], (case, where, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mish", "gelu_tanh"])
def test_the_tails_of_mish_and_tanh_gelu(nsg, boards, tmp_path, case):
    """At v = +-20, +-90, +-1e4 and on the grid times 2^10: no NaN; Mish(v) == v for large positive v (from v = 20 on
    tanh(softplus(v)) is 1 in float32); tanh-GELU(v) == v there too; and wherever the float64 definition is below the
    smallest normal (tanh-GELU from v = -20 on, Mish from v = -93 on: Mish(-90) = -90 exp(-90) is still 7e-38) so is
    the result.  The conv epilogue and the kEltAct instruction give the same bits."""
    res = {}
    for where in ("epilogue", "chain"):
        v, want, outs = run_case(nsg, boards, tmp_path, case, where)
        flat = v.reshape(len(v), -1)
        for n, o in outs:
            got = o[0].astype(np.float64)
            assert not np.isnan(got).any()
            big = flat[:n] >= 20.0
            assert big.any() and np.array_equal(got[big], flat[:n][big])
            tiny = (np.abs(want[:n]) < SMALLEST_NORMAL) & (flat[:n] < 0)
            assert tiny.any() and (np.abs(got[tiny]) < SMALLEST_NORMAL).all()
        res[where] = outs
    for (n, a), (_, b) in zip(res["epilogue"], res["chain"]):
        np.testing.assert_array_equal(a[0], b[0])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][4] and c not in ("mish", "gelu_tanh")])
def test_the_epilogue_and_the_instruction_give_equal_bits(nsg, boards, tmp_path, case):
    a = run_case(nsg, boards, tmp_path, case, "epilogue")[2]
    b = run_case(nsg, boards, tmp_path, case, "chain")[2]
    for (n, x), (_, y) in zip(a, b):
        np.testing.assert_array_equal(x[0], y[0])


# ---- 3. pad channels, and the fused forms at several widths ----------------------------------------------------------
def torch_boards(boards):
    import torch
    return boards[0], torch.from_numpy(boards[1])


def err_against_float64(nsg, gen, net, boards, path):
    import torch
    bb, x = torch_boards(boards)
    gen.export_model(net.float(), str(path))
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(x)]
    assert all(np.isfinite(r).all() for r in ref)
    outs = device_outputs(nsg, path, bb)
    for n, o in outs:
        assert all(np.isfinite(t).all() for t in o), n
    return max(max_err(o, [r[:n] for r in ref]) for n, o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["reciprocal_chain", "exp_chain", "exp_epilogue"])
def test_pad_channels_stay_zero_behind_reciprocal_and_exp(nsg, gen, boards, tmp_path, kind):
    """24 channels in rows of 32: 1 / 0 = inf or exp(0) = 1 in a pad channel would meet the next conv's zero weights
    (inf * 0 = NaN) or its 16-channel chunks.  reciprocal_chain: relu(stem) + 0.5 is positive on the 24 real channels;
    exp_epilogue: the Exp rides in the stem's launch."""
    import torch
    import torch.nn as nn

    class PadNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem, self.c = gen.conv(86, 24, 3), gen.conv(24, 24, 3)
            self.p, self.heads = gen.conv(24, 27, 1), gen.MeanHeads(24)

        def forward(self, x):
            x = self.stem(x)
            x = {"reciprocal_chain": lambda t: torch.reciprocal(torch.relu(t) + 0.5), "exp_chain": lambda t: torch.exp(torch.relu(t)),
                 "exp_epilogue": torch.exp}[kind](x)
            x = self.c(x)
            return (torch.flatten(self.p(x), 1),) + self.heads(x)

    torch.manual_seed(24)
    err = err_against_float64(nsg, gen, gen.randomize(PadNet(), 24).eval(), boards, tmp_path / "pad.onnx")
    print(kind, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout", [(24, 40), (40, 72), (64, 64)])
def test_fused_mish_width_sweep(nsg, gen, boards, tmp_path, cin, cout):
    """conv(cin, cout) -> BN -> Mish and a Mish behind a residual: pad channels on either side, more than one tile of
    64 output channels, and no pad at all."""
    import torch
    torch.manual_seed(cin + cout)
    net = gen.randomize(gen.MishSweepNet(cin, cout), cin * cout).eval()
    data = gen.export_model(net, str(tmp_path / "plan.onnx"))
    info = nsg.inspect_onnx(data, 86)
    assert info["launches"] == info["conv_launches"] + 1 + 2  # beside the convs only the heads' mean
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "w.onnx")
    print(cin, cout, "max abs err", err)
    assert err < 1e-4, err
