"""The general graph path's host half on pooling, the global max, Split and the clamp activations (nsg_inspect_onnx):
the pooling fixture plans on the graph path, a Split is a view, relu6 / hardswish / hardsigmoid ride in the conv's
launch while LeakyRelu and PRelu are one elementwise launch behind it, pooling adds no FLOPs, and what stays outside
-- even kernels, strides, pads that change the board, ceil_mode, a halo above 4, a used Indices output, Elu -- is
refused with the node's name and the reason.  No device needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

NAME = "net_graph_pool"


@pytest.fixture(scope="module")
def gen():
    import make_onnx_pool_golden
    return make_onnx_pool_golden


@pytest.fixture(scope="module")
def calib(nsg):
    import torch
    bb = nsg.synth.random_batch(19, 86, seed=31)
    return torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64))


def export(gen, net, tmp_path, name="m.onnx"):
    import torch
    torch.manual_seed(1)
    return gen.export_model(net.eval(), str(tmp_path / name))


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)


def test_the_pool_fixture_plans_on_the_graph_path(nsg, gen, golden_dir):
    import torch.nn as nn
    with open(f"{golden_dir}/{NAME}.onnx", "rb") as f:
        data = f.read()
    for op in (b"MaxPool", b"AveragePool", b"ReduceMax", b"Split", b"Clip", b"HardSwish", b"HardSigmoid", b"LeakyRelu",
               b"PRelu"):
        assert op in data, op
    with pytest.raises(nsg.NsgError):  # the family reader refuses it
        nsg.convert_onnx(data)
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    net = gen.PoolNet()
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    dense = [m for m in net.modules() if isinstance(m, nn.Linear)]
    assert len(convs) == 10 and len(dense) == 6
    # hardswish, relu6 and every BatchNorm ride in their conv's launch
    assert info["conv_launches"] == len(convs) + len(dense)
    # pooling, the global max and the elementwise launches count no FLOPs
    flops = sum(2 * 81 * m.kernel_size[0] * m.kernel_size[1] * (m.in_channels // m.groups) * m.out_channels for m in convs)
    assert info["flops_per_position"] == flops + sum(2 * m.in_features * m.out_features for m in dense)
    # beside the convs: block 1's mean, max, concat and bias-add + relu (4); block 2's mean, hardsigmoid gate times h
    # (2; the hardsigmoid itself rides in se2's launch); block 3's two pools, the copy of the 3x3 branch's LeakyRelu,
    # concat and PReLU + residual (5); the value head's mean, max and concat (3); planes and outputs (2)
    assert info["launches"] == info["conv_launches"] + 4 + 2 + 5 + 3 + 2


def test_a_split_is_a_view(nsg, gen, tmp_path):
    # stem, concat, policy, mean, value, draw + planes + outputs: the Split itself launches nothing
    info = nsg.inspect_onnx(export(gen, gen.PoolBlockNet(32, 16, None), tmp_path, "cat.onnx"), 86)
    assert info["launches"] == 6 + 2 and info["conv_launches"] == 4
    # its first part feeding a 1x1 conv costs what a Slice costs: the conv kernel reads whole rows, so the part is
    # copied into rows of its own (one graphConcat launch), however the split is aligned
    whole = nsg.inspect_onnx(export(gen, gen.PoolBlockNet(32, 32, None, through=True), tmp_path, "whole.onnx"), 86)
    split = nsg.inspect_onnx(export(gen, gen.PoolBlockNet(32, 16, None, through=True), tmp_path, "split.onnx"), 86)
    sliced = nsg.inspect_onnx(export(gen, gen.PoolBlockNet(32, 16, None, through=True, sliced=True), tmp_path, "slice.onnx"), 86)
    assert whole["launches"] == 6 + 2
    assert split["launches"] == sliced["launches"] == whole["launches"] + 1
    assert split["conv_launches"] == sliced["conv_launches"] == whole["conv_launches"] == 5
    # a pool reads the second part where it lies: no copy in front of it
    pooled = nsg.inspect_onnx(export(gen, gen.PoolBlockNet(32, 16, "max", 3), tmp_path, "pool.onnx"), 86)
    assert pooled["launches"] == info["launches"] + 1 and pooled["flops_per_position"] == info["flops_per_position"]


@pytest.mark.parametrize("act,extra", [("relu6", 0), ("hardswish", 0), ("hardsigmoid", 0), ("leaky_relu", 1), ("prelu", 1),
                                       ("hardtanh", 1), ("clamp_min", 1), ("abs", 1), ("neg", 1)])
def test_what_the_conv_epilogue_absorbs(nsg, gen, calib, tmp_path, act, extra):
    """stem, conv + BatchNorm (+ the parameter-free activation), policy, mean, value, draw + planes + outputs;
    everything with a parameter is one elementwise launch behind the conv."""
    info = nsg.inspect_onnx(export(gen, gen.ActNet(act, "epilogue", calib), tmp_path), 86)
    assert info["conv_launches"] == 5 and info["launches"] == 6 + 2 + extra
    # behind a runtime residual Add the activation joins the Add's launch, whichever it is
    chain = nsg.inspect_onnx(export(gen, gen.ActNet(act, "chain", calib), tmp_path, "c.onnx"), 86)
    assert chain["conv_launches"] == 5 and chain["launches"] == 6 + 2 + 1


@pytest.mark.parametrize("kind,k,d", [("max", 3, 1), ("max", 9, 1), ("max", (1, 9), 1), ("max", 3, 4), ("avg", 5, 0),
                                      ("avg", (3, 1), 1)])
def test_pooling_counts_no_flops(nsg, gen, tmp_path, kind, k, d):
    net = gen.PoolTapNet(kind, k, d)
    info = nsg.inspect_onnx(export(gen, net, tmp_path), 86)
    # the pool, the policy conv, the mean, value and draw + planes + outputs
    assert info["path"] == "graph" and info["conv_launches"] == 3 and info["launches"] == 5 + 2
    assert info["flops_per_position"] == 2 * 81 * 86 * 27 + 2 * 2 * 86


def test_both_forms_of_the_global_max_plan(nsg, gen, tmp_path):
    data = export(gen, gen.GlobalMaxNet(), tmp_path)
    assert b"ReduceMax" in data and b"MaxPool" in data
    info = nsg.inspect_onnx(data, 86)
    # stem, two global maxima, concat, policy Linear, mean, value, draw + planes + outputs
    assert info["launches"] == 8 + 2 and info["conv_launches"] == 4


def test_refusals_name_the_node_and_the_reason(nsg, gen, tmp_path):
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn

    class Front(nn.Module):
        """`f` on the planes, then a 1x1 policy conv and mean heads."""

        def __init__(self, f):
            super().__init__()
            self.f = f
            self.p = nn.Conv2d(86, 27, 1)
            self.heads = gen.MeanHeads(86)

        def forward(self, x):
            x = self.f(x)
            return (torch.flatten(self.p(x), 1),) + self.heads(x)

    def with_indices(x):
        y, i = Fn.max_pool2d(x, 3, 1, 1, return_indices=True)
        return y + i.float()

    cases = [
        (lambda x: Fn.max_pool2d(x, 2, 1, 1), "MaxPool", ("2x2", "odd")),                   # an even kernel
        (lambda x: Fn.max_pool2d(x, 3, 2, 1), "MaxPool", ("stride 2",)),
        (lambda x: Fn.max_pool2d(x, 3, 1, 0), "MaxPool", ("pads [0,0,0,0]", "[1,1,1,1]")),  # the output would be 7x7
        (lambda x: Fn.max_pool2d(x, 3, 1, 1, ceil_mode=True), "MaxPool", ("ceil_mode",)),
        (lambda x: gen.pool(x, "max", 3, 5), "MaxPool", ("halo", "5 squares")),             # reaches 5 squares past the edge
        (with_indices, "MaxPool", ("Indices",)),
        (lambda x: Fn.avg_pool2d(x, 4, 1, 2), "AveragePool", ("4x4", "odd")),
        (lambda x: Fn.avg_pool2d(x, 3, 3, 0), "AveragePool", ("stride 3",)),
        (Fn.elu, "Elu", ("op 'Elu'", "outside")),
    ]
    for i, (f, op, needles) in enumerate(cases):
        refused(nsg, export(gen, Front(f), tmp_path, f"r{i}.onnx"), f"node '/{op}'", *needles)


def test_truncated_models_are_errors_not_crashes(nsg, golden_dir):
    with open(f"{golden_dir}/{NAME}.onnx", "rb") as f:
        data = f.read()
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)
