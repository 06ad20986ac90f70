"""The general graph path's host half on rank and file pooling and line tensors (nsg_inspect_onnx): a coordinate-
attention net plans on the graph path at opsets 13 and 17, the simplest gates cost one pool and one elementwise launch,
and what stays outside is refused with the node's name and the reason.  No device needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import line_models as lm


@pytest.fixture(scope="module")
def gen():
    import make_onnx_norm_golden
    return make_onnx_norm_golden


def export(gen, net, tmp_path, name="m.onnx", opset=17):
    import torch
    torch.manual_seed(1)
    return gen.export_model(net.eval(), str(tmp_path / name), fold=False, opset=opset)


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)


def front(f, width=86, mods=()):
    """`f` on the planes, then a 1x1 policy conv and mean heads."""
    import torch
    import torch.nn as nn

    class Front(nn.Module):
        def __init__(self):
            super().__init__()
            self.p = nn.Conv2d(width, 27, 1)
            self.fc_v, self.fc_d = nn.Linear(width, 1), nn.Linear(width, 1)
            self.mods = nn.ModuleList(mods)  # what `f` calls

        def forward(self, x):
            x = f(x)
            h = x.mean(dim=(2, 3))
            return torch.flatten(self.p(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))

    return Front()


@pytest.mark.parametrize("opset", [13, 17])
@pytest.mark.parametrize("form", ["reduce", "adaptive", "max"])
def test_a_coordinate_attention_net_plans_on_the_graph_path(nsg, gen, tmp_path, form, opset):
    import torch.nn as nn
    net = lm.randomize(lm.coord_att_net(form), 3)
    data = export(gen, net, tmp_path, opset=opset)
    for op in ((b"AveragePool",) if form == "adaptive" else (b"ReduceMax",) if form == "max" else (b"ReduceMean",)) + (b"Concat", b"Split", b"BatchNormalization"):
        assert op in data, op
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    dense = [m for m in net.modules() if isinstance(m, nn.Linear)]
    assert len(convs) == 5 and len(dense) == 2
    assert info["conv_launches"] == len(convs) + len(dense)
    # the stem and the policy conv run over 81 squares, the shared conv over 18 lines, the two gate convs over 9
    rows = {net.stem: 81, net.policy: 81, net.att.conv1: 18, net.att.conv_h: 9, net.att.conv_w: 9}
    flops = sum(2 * rows[m] * m.kernel_size[0] * m.kernel_size[1] * m.in_channels * m.out_channels for m in convs)
    assert info["flops_per_position"] == flops + sum(2 * m.in_features * m.out_features for m in dense)
    # beside the convs: the two poolings, which write the halves of the 18-line block themselves (the Concat costs no
    # launch); the copies of the Split's two 9-line views into rows of their own in front of the gate convs (2: the
    # conv kernel reads contiguous rows); x * a_h * a_w in one elementwise launch (the sigmoids ride in the gate
    # convs); the mean of the heads; planes and outputs (2).  At opset 17 BatchNorm and HardSwish ride in the shared
    # conv's launch; at opset 13 the exporter writes hardswish as x * HardSigmoid(x), whose x has two readers, so the
    # two nodes are one elementwise launch on the 18-line tensor behind the conv.
    assert info["launches"] == info["conv_launches"] + 2 + 2 + 1 + 1 + 2 + (1 if opset == 13 else 0)


@pytest.mark.parametrize("opset", [13, 17])
def test_the_simplest_gates_cost_one_pool_and_one_elementwise_launch(nsg, gen, tmp_path, opset):
    import torch
    import torch.nn.functional as Fn
    # the policy conv, the mean, value, draw + planes + outputs
    base = 4 + 2
    forms = {
        "mean3": (lambda x: x * torch.sigmoid(x.mean(3, keepdim=True)), 1),
        "meanm1": (lambda x: x * torch.sigmoid(x.mean(-1, keepdim=True)), 1),
        "amax2": (lambda x: x * torch.sigmoid(x.amax(2, keepdim=True)), 1),
        "aap91": (lambda x: torch.sigmoid(Fn.adaptive_avg_pool2d(x, (9, 1))) * x, 1),
        "amp19": (lambda x: x + torch.sigmoid(Fn.adaptive_max_pool2d(x, (1, 9))), 1),
        "both": (lambda x: x * torch.sigmoid(x.mean(3, keepdim=True)) * torch.sigmoid(x.amax(2, keepdim=True)), 2),
    }
    for name, (f, pools) in forms.items():
        info = nsg.inspect_onnx(export(gen, front(f), tmp_path, name + ".onnx", opset), 86)
        assert info["path"] == "graph" and info["conv_launches"] == 3, name
        assert info["launches"] == base + pools + 1, (name, info["launches"])
        assert info["flops_per_position"] == 2 * 81 * 86 * 27 + 2 * 2 * 86, name


def test_refusals_name_the_node_and_the_reason(nsg, gen, tmp_path):
    import torch
    import torch.nn as nn

    conv31, conv11, fc = nn.Conv2d(86, 86, (3, 1), padding=(1, 0)), nn.Conv2d(86, 86, 1), nn.Linear(86 * 9, 86)

    def lines18(x):
        return torch.cat([x.mean(3, keepdim=True), x.mean(2, keepdim=True).permute(0, 1, 3, 2)], dim=2)

    cases = [
        (lambda x: x * x.mean(3).unsqueeze(3), "ReduceMean", ("keepdims = 0",)),
        (lambda x: x * conv31(x.mean(3, keepdim=True)), "mods.0/Conv", ("3x1 kernel", "line tensor [N,86,9,1]", "1x1")),
        (lambda x: x * fc(torch.flatten(x.mean(3, keepdim=True), 1)).reshape(-1, 86, 1, 1), "Flatten", ("line tensor", "[N,86,9,1]")),
        (lambda x: x * (x.mean(3, keepdim=True) + x.mean(2, keepdim=True)).mean(dim=(2, 3), keepdim=True), "Add", ("rank lines [N,86,9,1]", "file lines [N,86,1,9]", "Transpose")),
        (lambda x: x * torch.cat([x.amax(3, keepdim=True), torch.relu(lines18(x))], dim=2)[:, :, :9], "Concat_1", ("[N,86,9,1] and [N,86,18,1]", "9 + 9")),
        (lambda x: x * (x.mean(3, keepdim=True) * x.mean(dim=(2, 3), keepdim=True)), "Mul", ("flat operand [N,86,1,1]", "line tensors")),
        (lambda x: x.mean(1, keepdim=True) * x, "ReduceMean", ("over the squares only",)),
    ]
    for i, (f, op, needles) in enumerate(cases):
        refused(nsg, export(gen, front(f, mods=(conv31, conv11, fc)), tmp_path, f"r{i}.onnx"), f"node '/{op}'", *needles)

    class LinePolicy(nn.Module):
        """policy is a line tensor [N,243,9,1]."""

        def __init__(self):
            super().__init__()
            self.p = nn.Conv2d(86, 243, 1)
            self.fc_v, self.fc_d = nn.Linear(86, 1), nn.Linear(86, 1)

        def forward(self, x):
            h = x.mean(dim=(2, 3))
            return self.p(x.mean(3, keepdim=True)), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))

    refused(nsg, export(gen, LinePolicy(), tmp_path, "pol.onnx"), "node '/p/Conv'", "output 'policy'", "line tensor [N,243,9,1]")


def test_a_per_line_constant_is_refused_by_name(nsg):
    net = lm.LNet(nsg)
    s = net.stem()
    m = net.line(s, "m", "mean")
    y = net.node("Add", [m, net.const("pos", np.ones((em_F(), 9, 1)))], "y")
    z = net.node("Mul", [s, y], "z")
    refused(nsg, net.finish(z, s), "node 'y'", "per-(line, channel) constant", "[N,27,9,1]")


def em_F():
    import elt_models
    return elt_models.F


def test_truncated_models_are_errors_not_crashes(nsg, gen, tmp_path):
    data = export(gen, lm.randomize(lm.coord_att_net("reduce"), 3), tmp_path)
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)
