"""The general graph path's host half on the normalisations that need no batch statistics (nsg_inspect_onnx):
GroupNorm, InstanceNorm, LayerNorm below opset 17 and in the channel-last view, and RMSNorm each plan as exactly one
launch, GroupNorm's affine tail and a ReLU ride in that launch, the opset-13 and opset-17 exports of a LayerNorm plan
alike, and what stays outside is refused with the node's name and the reason.  No device needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

NAME = "net_graph_norm"
C = 24


@pytest.fixture(scope="module")
def gen():
    import make_onnx_norm_golden
    return make_onnx_norm_golden


def export(gen, net, tmp_path, name="m.onnx", opset=17):
    import torch
    torch.manual_seed(1)
    return gen.export_model(net.eval(), str(tmp_path / name), opset=opset)


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)


def test_the_norm_fixture_plans_on_the_graph_path(nsg, gen, golden_dir):
    import torch.nn as nn
    with open(f"{golden_dir}/{NAME}.onnx", "rb") as f:
        data = f.read()
    for op in (b"InstanceNormalization", b"LayerNormalization", b"ReduceMean", b"Pow", b"Sqrt", b"Transpose"):
        assert op in data, op
    assert b"BatchNormalization" not in data
    with pytest.raises(nsg.NsgError):  # the family reader refuses it
        nsg.convert_onnx(data)
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    net = gen.NormFixtureNet()
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    dense = [m for m in net.modules() if isinstance(m, nn.Linear)]
    assert info["conv_launches"] == len(convs) + len(dense) == 13
    # the normalisations count no FLOPs
    flops = sum(2 * 81 * m.kernel_size[0] * m.kernel_size[1] * (m.in_channels // m.groups) * m.out_channels for m in convs)
    tok = {net.b3.fc1, net.b3.fc2}  # Linear layers over the 81 tokens
    assert info["flops_per_position"] == flops + sum(2 * (81 if m in tok else 1) * m.in_features * m.out_features for m in dense)
    # beside the convs: three GroupNorms (two with their ReLU), the block's residual Add + ReLU, the InstanceNorm with
    # its ReLU, the channel-last LayerNorm, the token RMSNorm, the decomposed LayerNorm, the mean, the flat RMSNorm
    # (10; both residuals of the ConvNeXt and token blocks ride in a conv's launch); planes and outputs (2)
    assert info["launches"] == info["conv_launches"] + 10 + 2


def forms(gen):
    import torch.nn as nn
    return {
        "groupnorm": (lambda: nn.GroupNorm(3, C), "spatial", 17),
        "groupnorm_opset13": (lambda: nn.GroupNorm(3, C), "spatial", 13),
        "groupnorm_one_group": (lambda: nn.GroupNorm(1, C), "spatial", 17),
        "groupnorm_per_channel": (lambda: nn.GroupNorm(C, C), "spatial", 17),
        "groupnorm_no_affine": (lambda: nn.GroupNorm(3, C, affine=False), "spatial", 17),
        "instancenorm_affine": (lambda: nn.InstanceNorm2d(C, affine=True), "spatial", 17),
        "instancenorm": (lambda: nn.InstanceNorm2d(C), "spatial", 17),
        "layernorm_opset13_tokens": (lambda: nn.LayerNorm(C), "token", 13),
        "layernorm_opset13_flat": (lambda: nn.LayerNorm(C), "flat", 13),
        "layernorm_channel_last": (lambda: gen.ChanLastLN(C), "spatial", 17),
        "layernorm_channel_last_opset13": (lambda: gen.ChanLastLN(C), "spatial", 13),
        "layernorm_written_out_mul": (lambda: gen.DecomposedLN(C, square="mul", beta=False), "token", 17),
        "layernorm_written_out_bare": (lambda: gen.DecomposedLN(C, gamma=False, beta=False), "token", 17),
        "rmsnorm_rsqrt_tokens": (lambda: gen.RMSNorm(C, form="rsqrt"), "token", 17),
        "rmsnorm_div_tokens": (lambda: gen.RMSNorm(C, form="div"), "token", 17),
        "rmsnorm_rsqrt_flat": (lambda: gen.RMSNorm(C, form="rsqrt"), "flat", 13),
    }


FORMS = ["groupnorm", "groupnorm_opset13", "groupnorm_one_group", "groupnorm_per_channel", "groupnorm_no_affine",
         "instancenorm_affine", "instancenorm", "layernorm_opset13_tokens", "layernorm_opset13_flat",
         "layernorm_channel_last", "layernorm_channel_last_opset13", "layernorm_written_out_mul",
         "layernorm_written_out_bare", "rmsnorm_rsqrt_tokens", "rmsnorm_div_tokens", "rmsnorm_rsqrt_flat"]


@pytest.mark.parametrize("form", FORMS)
def test_every_form_is_exactly_one_launch(nsg, gen, tmp_path, form):
    """The launch count of a stem net with the normalisation equals that of the same net with nn.Identity() in its
    place plus one: the Reshapes, Transposes and the pattern's interior nodes launch nothing, and neither do
    GroupNorm's gamma and beta."""
    import torch.nn as nn
    make, domain, opset = forms(gen)[form]
    assert sorted(forms(gen)) == sorted(FORMS)
    base = nsg.inspect_onnx(export(gen, gen.NormNet(C, nn.Identity(), domain), tmp_path, "id.onnx", opset), 86)
    info = nsg.inspect_onnx(export(gen, gen.randomize(gen.NormNet(C, make(), domain), 3), tmp_path, "n.onnx", opset), 86)
    assert info["path"] == "graph"
    assert info["launches"] == base["launches"] + 1
    assert info["conv_launches"] == base["conv_launches"]
    assert info["flops_per_position"] == base["flops_per_position"]


def test_a_relu_rides_in_the_groupnorm_launch(nsg, gen, tmp_path):
    import torch.nn as nn
    base = nsg.inspect_onnx(export(gen, gen.NormNet(C, nn.Identity()), tmp_path, "id.onnx"), 86)
    for i, mid in enumerate((nn.GroupNorm(3, C), nn.InstanceNorm2d(C, affine=True))):
        info = nsg.inspect_onnx(export(gen, gen.NormNet(C, mid, act=True), tmp_path, f"a{i}.onnx"), 86)
        assert info["launches"] == base["launches"] + 1
    # behind the LayerNorm a ReLU stays a launch of its own: the existing LayerNorm launch takes no activation
    ln = nsg.inspect_onnx(export(gen, gen.NormNet(C, gen.ChanLastLN(C), act=True), tmp_path, "ln.onnx"), 86)
    assert ln["launches"] == base["launches"] + 2


@pytest.mark.parametrize("domain,mid", [("token", "ln"), ("flat", "ln"), ("spatial", "chanlast")])
def test_opset_13_and_17_layernorm_plan_alike(nsg, gen, tmp_path, domain, mid):
    import torch.nn as nn
    net = gen.randomize(gen.NormNet(C, nn.LayerNorm(C) if mid == "ln" else gen.ChanLastLN(C), domain), 5)
    d13, d17 = export(gen, net, tmp_path, "o13.onnx", 13), export(gen, net, tmp_path, "o17.onnx", 17)
    assert b"LayerNormalization" in d17 and b"LayerNormalization" not in d13 and b"ReduceMean" in d13
    i13, i17 = nsg.inspect_onnx(d13, 86), nsg.inspect_onnx(d17, 86)
    for key in ("launches", "conv_launches", "flops_per_position", "activation_bytes_per_position"):
        assert i13[key] == i17[key], key


def test_refusals_name_the_node_and_the_reason(nsg, gen, tmp_path):
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn
    from make_onnx_attention_golden import tokens

    class RawInstanceNorm(torch.autograd.Function):
        """One InstanceNormalization node on whatever x, scale and bias are (the exporter itself writes the node for
        4-D inputs with constant parameters only); the planner never runs it, so forward only keeps the shape."""

        @staticmethod
        def forward(ctx, x, s, b):
            return x * 1.0

        @staticmethod
        def symbolic(g, x, s, b):
            return g.op("InstanceNormalization", x, s, b, epsilon_f=1e-5)

    class WithMean(torch.autograd.Function):
        """A LayerNormalization with its mean output in use."""

        @staticmethod
        def forward(ctx, x, w, b):
            return Fn.layer_norm(x, w.shape, w, b), x.mean(-1, keepdim=True)

        @staticmethod
        def symbolic(g, x, w, b):
            y, mean, _ = g.op("LayerNormalization", x, w, b, axis_i=-1, epsilon_f=1e-5, outputs=3)
            return y, mean

    class Front(nn.Module):
        """`f` behind a 3x3 stem of C channels, then a 1x1 policy conv and mean heads."""

        def __init__(self, f):
            super().__init__()
            self.f = f
            self.stem = gen.conv(86, C, 3)
            self.w, self.b = nn.Parameter(torch.rand(C) + 0.5), nn.Parameter(torch.randn(C))
            self.p = gen.conv(C, 27, 1)
            self.heads = gen.MeanHeads(C)

        def forward(self, x):
            x = self.f(self, torch.relu(self.stem(x)))
            return (torch.flatten(self.p(x), 1),) + self.heads(x)

    def back(x, t):
        return t.transpose(1, 2).reshape(x.size(0), C, 9, 9)

    def with_mean(m, x):
        y, mean = WithMean.apply(x.permute(0, 2, 3, 1), m.w, m.b)
        return (y + mean).permute(0, 3, 1, 2)

    def deviates(m, x):
        t = tokens(x)
        d = t - t.mean(-1, keepdim=True)
        return back(x, d / torch.tanh(d.pow(2).mean(-1, keepdim=True) + 1e-5))

    def interior_read_twice(m, x):
        t = tokens(x)
        v = t.pow(2).mean(-1, keepdim=True)
        return back(x, t / torch.sqrt(v + 1e-5) + v)

    def groups_read_elsewhere(m, x):
        g = x.reshape(x.size(0), 3, -1)
        return (Fn.instance_norm(g) + g).reshape(x.size(0), C, 9, 9)

    cases = [
        (lambda m, x: RawInstanceNorm.apply(x, x.mean(dim=(2, 3)), m.b), "InstanceNormalization", ("the scale must be a constant",)),
        (lambda m, x: RawInstanceNorm.apply(x, m.w, torch.tanh(x).mean(dim=(2, 3))), "InstanceNormalization", ("the bias must be a constant",)),
        (lambda m, x: back(x, RawInstanceNorm.apply(tokens(x), torch.ones(81), torch.zeros(81))), "InstanceNormalization",
         ("[N,81,24]", "spatial tensor only")),
        (lambda m, x: x * RawInstanceNorm.apply(x.mean(dim=(2, 3)), m.w, m.b)[:, :, None, None], "InstanceNormalization",
         ("[N,24]", "spatial tensor only")),
        (lambda m, x: Fn.instance_norm(x.reshape(x.size(0), 9, -1)).reshape(x.size(0), C, 9, 9), "Reshape",
         ("9 groups over 24 channels", "does not divide")),
        (lambda m, x: (x - x.mean(1, keepdim=True)) * m.w[:, None, None], "ReduceMean", ("over the squares only",)),
        (with_mean, "LayerNormalization", ("mean / inverse-deviation outputs",)),
        (deviates, "Tanh", ("decomposed normalisation", "expected Sqrt")),
        (interior_read_twice, "Add_1", ("interior tensor of the decomposed normalisation",)),
        (groups_read_elsewhere, "Add", ("[N,3,648]", "GroupNorm pattern")),
        (lambda m, x: (x.permute(0, 2, 3, 1) * m.w).permute(0, 3, 1, 2), "Mul", ("[N,9,9,24]", "channel-last view")),
    ]
    for i, (f, node, needles) in enumerate(cases):
        refused(nsg, export(gen, Front(f), tmp_path, f"r{i}.onnx"), f"node '/{node}'", *needles)
    # opset 18's GroupNormalization node is outside the op set (and the opset range): a LayerNormalization file with the
    # op renamed, both names being eighteen letters long
    data = export(gen, gen.NormNet(C, nn.LayerNorm(C), "token"), tmp_path, "gn18.onnx")
    assert data.count(b"LayerNormalization") >= 1
    refused(nsg, data.replace(b"LayerNormalization", b"GroupNormalization"), "GroupNormalization", "op 'GroupNormalization' is outside the supported op set")


def test_truncated_models_are_errors_not_crashes(nsg, golden_dir):
    with open(f"{golden_dir}/{NAME}.onnx", "rb") as f:
        data = f.read()
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)
