"""The general graph path's host half on convolution geometries (nsg_inspect_onnx): k x k, 1 x k and k x 1 kernels,
dilations and depthwise convs plan as conv launches with their epilogues fused, the FLOP count follows the kernel
size, and everything else -- even kernels, pads that change the board, a halo above 4, grouped convs that are not
depthwise, channel multipliers, strides -- is refused with the node's name and the reason.  No device needed."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


@pytest.fixture(scope="module")
def gen():
    import make_onnx_geometry_golden
    return make_onnx_geometry_golden


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


def conv_flops(m):
    """2 * 81 * kh * kw * Cin * Cout for a dense conv, 2 * 81 * kh * kw * C for a depthwise one."""
    kh, kw = m.kernel_size
    return 2 * 81 * kh * kw * (m.in_channels // m.groups) * m.out_channels


def test_the_geometry_fixture_plans_on_the_graph_path(nsg, gen, golden_dir):
    import torch.nn as nn
    with open(f"{golden_dir}/net_graph_geom.onnx", "rb") as f:
        data = f.read()
    with pytest.raises(nsg.NsgError):  # the family reader refuses it
        nsg.convert_onnx(data)
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    net = gen.GeomNet()
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    dense = [m for m in net.modules() if isinstance(m, nn.Linear)]
    assert len(convs) == 9 and len(dense) == 3
    assert sorted(m.kernel_size for m in convs) == [(1, 1), (1, 1), (1, 1), (1, 9), (3, 3), (3, 3), (5, 5), (7, 7), (9, 1)]
    # every BatchNorm (the one behind the depthwise conv too), residual add and activation rides in a conv launch:
    # beside the convs and the dense layers there is the value head's flatten, the planes and the outputs
    assert info["conv_launches"] == len(convs) + len(dense)
    assert info["launches"] == info["conv_launches"] + 1 + 2
    flops = sum(conv_flops(m) for m in convs) + sum(2 * m.in_features * m.out_features for m in dense)
    assert info["flops_per_position"] == flops
    F = 32
    assert conv_flops(net.dw) == 2 * 81 * 49 * F and conv_flops(net.stem) == 2 * 81 * 25 * 86 * F


@pytest.mark.parametrize("k,d", [(5, 1), (7, 1), (9, 1), ((1, 9), 1), ((9, 1), 1), ((3, 1), 1), (3, 2), (3, 4), (5, 2),
                                 ((3, 5), (4, 1))])
def test_dense_geometries_plan_as_one_launch(nsg, gen, tmp_path, k, d):
    net = gen.TapNet(k, d)
    info = nsg.inspect_onnx(export(gen, net, tmp_path), 86)
    # the policy conv, the mean, value and draw + planes + outputs
    assert info["path"] == "graph" and info["conv_launches"] == 3 and info["launches"] == 4 + 2
    assert info["flops_per_position"] == conv_flops(net.p) + 2 * 2 * 86


def test_batchnorm_behind_a_depthwise_conv_adds_no_launch(nsg, gen, tmp_path):
    bare = nsg.inspect_onnx(export(gen, gen.DwNet(24, 5, full=False), tmp_path, "bare.onnx"), 86)
    data = export(gen, gen.DwNet(24, 5, full=True), tmp_path, "full.onnx")
    assert b"BatchNormalization" in data  # the exporter left it in the file
    full = nsg.inspect_onnx(data, 86)
    # stem, depthwise (+ BatchNorm + residual + swish), policy, mean, value, draw
    assert bare["launches"] == full["launches"] == 6 + 2
    assert bare["conv_launches"] == full["conv_launches"] == 5
    assert full["flops_per_position"] == 2 * 81 * (9 * 86 * 24 + 25 * 24 + 24 * 27) + 2 * 2 * 24


def test_refusals_name_the_node_and_the_reason(nsg, gen, tmp_path):
    import torch.nn as nn
    F = 32
    cases = [
        (nn.Conv2d(86, F, 4, padding=2), ("4x4", "odd")),                        # an even kernel
        (nn.Conv2d(86, F, 3, padding=0), ("pads [0,0,0,0]", "[1,1,1,1]")),       # the output would be 7x7
        (nn.Conv2d(86, F, 3, padding=5, dilation=5), ("halo", "5 squares")),     # reaches 5 squares past the edge
        (nn.Conv2d(86, F, 3, padding=1, groups=2), ("group 2", "depthwise")),    # 1 < groups < Cin
        (nn.Conv2d(86, 172, 3, padding=1, groups=86), ("multiplier 2",)),        # depthwise with two outputs per input
        (nn.Conv2d(86, F, 3, padding=1, stride=2), ("stride",)),
        (nn.Conv2d(86, F, (3, 9), padding=(1, 3)), ("pads [1,3,1,3]", "[1,4,1,4]")),
        (nn.Conv2d(86, F, 11, padding=5), ("11x11",)),
    ]
    for i, (stem, needles) in enumerate(cases):
        refused(nsg, export(gen, gen.StemNet(stem), tmp_path, f"r{i}.onnx"), "node '/stem/Conv'", *needles)
