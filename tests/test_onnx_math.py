"""The general graph path's host half on elementwise maths (nsg_inspect_onnx): Exp, Log, Sqrt and Reciprocal on a
run-time tensor are one activation each (they ride in a conv's launch), Pow with a constant scalar exponent is decided
on the host, Mish, tanh-GELU and softsign as the exporter writes them are one activation each, a chain of cubes is cut
at the register limit, the decomposed LayerNorm keeps its precedence over its own Pow and Sqrt, and what stays outside
-- a run-time or per-channel exponent, Elu, Selu, opset 18's Mish node -- is refused with the node's name and the
reason.  No device needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

NAME = "net_graph_math"


@pytest.fixture(scope="module")
def gen():
    import make_onnx_math_golden
    return make_onnx_math_golden


def export(gen, net, tmp_path, name="m.onnx", opset=17):
    import torch
    torch.manual_seed(1)
    return gen.export_model(net.eval(), str(tmp_path / name), opset=opset)


def plan(nsg, gen, net, tmp_path, name="m.onnx", opset=17):
    info = nsg.inspect_onnx(export(gen, net, tmp_path, name, opset), 86)
    assert info["path"] == "graph" and info["precision"] == "fp32"
    return info


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)


def gelu_tanh(x):
    import torch.nn.functional as Fn
    return Fn.gelu(x, approximate="tanh")


def test_the_math_fixture_plans_on_the_graph_path(nsg, gen, golden_dir):
    import torch.nn as nn
    with open(f"{golden_dir}/{NAME}.onnx", "rb") as f:
        data = f.read()
    for op in (b"Exp", b"Log", b"Sqrt", b"Reciprocal", b"Pow", b"Softplus", b"Tanh", b"Abs", b"Clip"):
        assert op in data, op
    with pytest.raises(nsg.NsgError):  # the family reader refuses it
        nsg.convert_onnx(data)
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    net = gen.MathFixtureNet()
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    dense = [m for m in net.modules() if isinstance(m, nn.Linear)]
    assert info["conv_launches"] == len(convs) + len(dense) == 12
    tok = {net.ffn.fc1, net.ffn.fc2}  # Linear layers over the 81 tokens
    flops = sum(2 * 81 * m.kernel_size[0] * m.kernel_size[1] * m.in_channels * m.out_channels for m in convs)
    assert info["flops_per_position"] == flops + sum(2 * (81 if m in tok else 1) * m.in_features * m.out_features for m in dense)
    assert info["flops_per_position"] == 8137056
    # Every Mish, the tanh-GELU, the softsign and both residuals ride in a conv's launch.  Beside the convs: x ** 2 of
    # the gate, its mean over the squares, the gate itself (eps, Sqrt and Div(1, .) on the pooled tensor inlined into
    # x * g), the three branches' mix (18 registers: cut once, so two launches), the mean, clamp -> Exp inlined into the
    # policy's scaling, |h| + 0.25 -> Sqrt, the Reciprocal (10); planes and outputs (2)
    assert info["launches"] == info["conv_launches"] + 10 + 2


def single_ops():
    import torch
    import torch.nn.functional as Fn
    return {
        "exp": torch.exp, "log": torch.log, "log1p": torch.log1p, "logsigmoid": Fn.logsigmoid, "sqrt": torch.sqrt,
        "rsqrt": torch.rsqrt, "reciprocal": torch.reciprocal, "one_over_x": lambda x: 1 / x, "square": lambda x: x ** 2,
        "cube": lambda x: x.pow(3), "pow_1.5": lambda x: x ** 1.5,
    }


SINGLE = ["exp", "log", "log1p", "logsigmoid", "sqrt", "rsqrt", "reciprocal", "one_over_x", "square", "cube", "pow_1.5"]
# launches beyond the same net without the op: a single activation rides in the stem's launch (log1p's Add 1 goes into
# the stem's bias), two nodes are one launch
EXTRA = {"exp": 0, "log": 0, "sqrt": 0, "reciprocal": 0, "one_over_x": 0, "log1p": 0, "logsigmoid": 1, "rsqrt": 1, "square": 1,
         "cube": 1, "pow_1.5": 1}


@pytest.mark.parametrize("opset", [13, 17])
@pytest.mark.parametrize("op", SINGLE)
def test_each_op_alone_behind_a_1x1_stem_plans(nsg, gen, tmp_path, op, opset):
    """The parent refuses every one of them."""
    assert sorted(single_ops()) == sorted(SINGLE)
    base = plan(nsg, gen, gen.Front(None), tmp_path, "id.onnx", opset)
    info = plan(nsg, gen, gen.Front(single_ops()[op]), tmp_path, "op.onnx", opset)
    assert info["launches"] == base["launches"] + EXTRA[op]
    assert info["conv_launches"] == base["conv_launches"] and info["flops_per_position"] == base["flops_per_position"]
    # on the second half of a Split no conv absorbs it: one elementwise launch in place of the copy the policy conv
    # would need of that half
    base = plan(nsg, gen, gen.Front(None, split=True), tmp_path, "ids.onnx", opset)
    info = plan(nsg, gen, gen.Front(single_ops()[op], split=True), tmp_path, "ops.onnx", opset)
    assert info["launches"] == base["launches"]


@pytest.mark.parametrize("case", ["conv_bn_mish", "linear_gelu_tanh", "linear_gelu_tanh_pow", "groupnorm_mish", "conv_softsign"])
def test_the_patterns_ride_in_the_launch_in_front(nsg, gen, tmp_path, case):
    """The launch count equals that of the same net without the activation.  The parent counts one more each: its conv
    takes the pattern's first node only."""
    import torch.nn.functional as Fn
    f, kw = {"conv_bn_mish": (Fn.mish, dict(k=3, bn=True)), "linear_gelu_tanh": (gelu_tanh, dict(domain="token")),
             "linear_gelu_tanh_pow": (gen.gelu_tanh_pow, dict(domain="token")), "groupnorm_mish": (Fn.mish, dict(domain="norm")),
             "conv_softsign": (Fn.softsign, dict(k=3))}[case]
    for opset in (13, 17):
        base = plan(nsg, gen, gen.Front(None, **kw), tmp_path, "id.onnx", opset)
        info = plan(nsg, gen, gen.Front(f, **kw), tmp_path, "act.onnx", opset)
        for key in ("launches", "conv_launches", "flops_per_position", "activation_bytes_per_position"):
            assert info[key] == base[key], (key, opset)
        # behind a Split half the whole pattern is one instruction of one elementwise launch
        if "domain" not in kw:
            assert plan(nsg, gen, gen.Front(f, split=True), tmp_path, "s.onnx", opset)["launches"] == \
                plan(nsg, gen, gen.Front(None, split=True), tmp_path, "si.onnx", opset)["launches"]


def test_a_chain_that_deviates_from_a_pattern_stays_elementwise(nsg, gen, tmp_path):
    import torch
    import torch.nn.functional as Fn
    base = plan(nsg, gen, gen.Front(None, k=3), tmp_path, "id.onnx")
    cases = {
        "softplus_beta": lambda x: x * torch.tanh(Fn.softplus(x, beta=2.0)),           # Mul -> Softplus -> Div: no Mish
        "mish_of_another": lambda x: torch.relu(x) * torch.tanh(Fn.softplus(x)),       # the Mul's other operand is not x
        "gelu_other_constant": lambda x: 0.5 * x * (1.0 + torch.tanh(0.79 * (x + 0.044715 * x ** 3))),
        "softsign_plus_two": lambda x: x / (x.abs() + 2.0),
        "tanh_read_twice": lambda x: (lambda t: x * t + t)(torch.tanh(Fn.softplus(x))),
    }
    for name, f in cases.items():
        info = plan(nsg, gen, gen.Front(f, k=3), tmp_path, name + ".onnx")
        # the stem takes the first node at most and the rest is one launch; a tensor read twice is stored, which cuts there
        assert info["launches"] == base["launches"] + (2 if name == "tanh_read_twice" else 1), name


POW = {1: 0, 2: 1, 3: 1, 4: 1, 0.5: 0, -1: 0, -0.5: 1, -2: 1, 1.5: 1}


@pytest.mark.parametrize("exponent", list(POW))
def test_pow_with_a_constant_scalar_exponent(nsg, gen, tmp_path, exponent):
    """x ** 1 is x and launches nothing; 0.5 and -1 are the square root and the reciprocal, activations that ride in
    the stem's launch; every other exponent is one elementwise launch behind it."""
    base = plan(nsg, gen, gen.Front(None), tmp_path, "id.onnx")
    info = plan(nsg, gen, gen.Front(lambda x: x ** exponent), tmp_path, "p.onnx")
    assert info["launches"] == base["launches"] + POW[exponent]
    assert info["conv_launches"] == base["conv_launches"]


@pytest.mark.parametrize("exponent,per_node", [(3, 2), (2, 1), (1.5, 2)])
def test_a_chain_of_powers_is_cut_at_the_register_limit(nsg, gen, tmp_path, exponent, per_node):
    """On a Split half: one load, then `per_node` registers a node (x ** 3: the square and the product; x ** 1.5: the
    exponent's load and powf).  A launch holds (16 - 1) // per_node nodes; one more is cut into a second launch, never
    refused."""
    def chain(k):
        def f(x):
            for _ in range(k):
                x = x ** exponent
            return x
        return f

    fits = 15 // per_node
    if exponent == 1.5:
        fits = min(fits, 7)  # and 8 sources: the tensor and seven scalars
    base = plan(nsg, gen, gen.Front(chain(1), split=True), tmp_path, "c1.onnx")["launches"]
    for k, extra in ((fits - 1, 0), (fits, 0), (fits + 1, 1), (2 * fits, 1), (2 * fits + 1, 2)):
        assert plan(nsg, gen, gen.Front(chain(k), split=True), tmp_path, f"c{k}.onnx")["launches"] == base + extra, k


def test_refusals_name_the_node_and_the_reason(nsg, gen, tmp_path):
    import torch
    import torch.nn.functional as Fn
    per_channel = torch.linspace(1.0, 2.0, 24)[None, :, None, None]
    cases = [
        (lambda x: torch.pow(x.abs() + 1.0, torch.sigmoid(x)), "Pow", ("the exponent must be a constant scalar",)),
        (lambda x: torch.pow(x.abs() + 1.0, per_channel), "Pow", ("the exponent must be a constant scalar",)),
        (Fn.elu, "Elu", ("op 'Elu'", "outside the supported op set")),
        (Fn.selu, "Selu", ("op 'Selu'", "outside the supported op set")),
    ]
    for i, (f, op, needles) in enumerate(cases):
        refused(nsg, export(gen, gen.Front(f), tmp_path, f"r{i}.onnx"), f"node '/{op}'", *needles)
    # opset 18's Mish node: an Relu file with the op renamed, both names being four letters long
    data = export(gen, gen.Front(torch.relu), tmp_path, "mish18.onnx")
    assert data.count(b"Relu") >= 1
    refused(nsg, data.replace(b"Relu", b"Mish"), "op 'Mish' is outside the supported op set")
    # a stand-alone Softmax stays refused
    refused(nsg, export(gen, gen.Front(lambda x: torch.softmax(x, 1)), tmp_path, "sm.onnx"), "Softmax", "only the softmax over the keys")


def test_truncated_models_are_errors_not_crashes(nsg, golden_dir):
    with open(f"{golden_dir}/{NAME}.onnx", "rb") as f:
        data = f.read()
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)


@pytest.mark.parametrize("domain", ["token", "flat"])
def test_the_decomposed_layernorm_keeps_its_pow_and_sqrt(nsg, tmp_path, domain):
    """The opset-13 export of nn.LayerNorm still plans as one LayerNorm launch, as the opset-17 node does, now that
    its Pow and Sqrt would be legal elementwise nodes too."""
    import make_onnx_norm_golden as ng
    import torch
    import torch.nn as nn
    torch.manual_seed(1)
    net = ng.randomize(ng.NormNet(24, nn.LayerNorm(24), domain), 5).eval()
    d13 = ng.export_model(net, str(tmp_path / "o13.onnx"), opset=13)
    d17 = ng.export_model(net, str(tmp_path / "o17.onnx"), opset=17)
    assert b"Pow" in d13 and b"Sqrt" in d13 and b"LayerNormalization" not in d13 and b"LayerNormalization" in d17
    base = nsg.inspect_onnx(ng.export_model(ng.NormNet(24, nn.Identity(), domain).eval(), str(tmp_path / "id.onnx"), opset=13), 86)
    i13, i17 = nsg.inspect_onnx(d13, 86), nsg.inspect_onnx(d17, 86)
    assert i13["launches"] == i17["launches"] == base["launches"] + 1
