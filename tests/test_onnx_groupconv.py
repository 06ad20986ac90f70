"""The general graph path's host half on grouped convolutions (nsg_inspect_onnx): a Conv with 1 < group < Cin whose
group width is a multiple of 4 plans as one conv launch with its epilogue fused, the FLOP count follows Cin / group, and
everything outside the rule -- a group width that 4 does not divide, a group count that does not divide the output
channels, strides, even kernels, a halo above 4, channel multipliers -- is refused with the node's name and the reason.
No device needed."""
import numpy as np
import pytest

import group_models as gm


def inspect(nsg, net, tmp_path, name="m.onnx"):
    import torch
    torch.manual_seed(1)
    return nsg.inspect_onnx(gm.export(net, tmp_path / name), 86)


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)


@pytest.mark.parametrize("cin,cout,G", gm.SHAPES, ids=gm.sid)
def test_each_shape_plans_as_one_conv_launch(nsg, tmp_path, cin, cout, G):
    net = gm.GroupNet(cin, cout, G)
    info = inspect(nsg, net, tmp_path)
    # stem, the grouped conv, policy, the mean, value and draw + planes + outputs
    assert info["path"] == "graph" and info["precision"] == "fp32"
    assert info["conv_launches"] == 5 and info["launches"] == 6 + 2
    per_group = 2 * 81 * 9 * (cin // G) * cout
    assert gm.conv_flops(net.g) == per_group
    assert info["flops_per_position"] == gm.conv_flops(net.stem) + per_group + gm.conv_flops(net.p) + 2 * 2 * cout
    # the same function written as Split -> G convs -> Concat costs a copy and a launch per group, and a concat
    twin = inspect(nsg, gm.twin_of(net), tmp_path, "twin.onnx")
    assert twin["conv_launches"] == 4 + G and twin["launches"] > info["launches"]
    assert twin["flops_per_position"] == info["flops_per_position"]


@pytest.mark.parametrize("k,d", [(1, 1), (3, 1)] + gm.GEOMETRIES[1:], ids=gm.sid)
def test_flops_follow_the_kernel_and_the_group_width(nsg, tmp_path, k, d):
    net = gm.GroupNet(72, 48, 3, k, d)
    info = inspect(nsg, net, tmp_path)
    kh, kw = gm.gen.pair(k)
    assert gm.conv_flops(net.g) == 2 * 81 * kh * kw * 24 * 48
    assert info["conv_launches"] == 5 and info["launches"] == 6 + 2
    assert info["flops_per_position"] == gm.conv_flops(net.stem) + gm.conv_flops(net.g) + gm.conv_flops(net.p) + 2 * 2 * 48


def test_batchnorm_residual_and_relu_behind_a_grouped_conv_add_no_launch(nsg, tmp_path):
    bare = inspect(nsg, gm.GroupBlockNet(32, 4, full=False), tmp_path, "bare.onnx")
    data = gm.export(gm.GroupBlockNet(32, 4, full=True), tmp_path / "full.onnx")
    assert b"BatchNormalization" in data  # the exporter left it in the file
    full = nsg.inspect_onnx(data, 86)
    assert bare["launches"] == full["launches"] == 6 + 2
    assert bare["conv_launches"] == full["conv_launches"] == 5
    assert full["flops_per_position"] == 2 * 81 * (9 * 86 * 32 + 9 * 8 * 32 + 32 * 27) + 2 * 2 * 32


def test_the_resnext_net_plans_one_launch_per_conv(nsg, tmp_path):
    import torch.nn as nn
    net = gm.ResNeXtNet(32, 8)
    info = inspect(nsg, net, tmp_path)
    convs = [m for m in net.modules() if isinstance(m, nn.Conv2d)]
    dense = [m for m in net.modules() if isinstance(m, nn.Linear)]
    assert len(convs) == 1 + 3 * 3 + 2 and len(dense) == 3
    # every BatchNorm, residual and activation rides in a conv launch; beside them the value head's flatten
    assert info["conv_launches"] == len(convs) + len(dense)
    assert info["launches"] == info["conv_launches"] + 1 + 2
    assert info["flops_per_position"] == sum(gm.conv_flops(m) for m in convs) + sum(2 * m.in_features * m.out_features for m in dense)


def hand_built(nsg, cin, cout, group, per):
    """stem(cin) -> Conv(group, weight [cout, per, 3, 3]) by hand: torch will not construct what the planner refuses."""
    import elt_models as em
    net = em.Net(nsg)
    net.stem(cin)
    net.const("g_w", np.ones((cout, per, 3, 3)))
    net.node("Conv", ["s", "g_w"], "y", name="grouped", kernel_shape=[3, 3], pads=[1, 1, 1, 1], group=group)
    return net.finish("y", "y")


def test_refusals_name_the_node_and_the_reason(nsg, tmp_path):
    import torch.nn as nn
    from make_onnx_geometry_golden import StemNet
    cases = [
        (nn.Conv2d(24, 24, 3, padding=1, groups=4), ("group 4", "6 per group", "multiple of 4", "depthwise")),
        (nn.Conv2d(36, 36, 3, padding=1, groups=2), ("group 2", "18 per group", "multiple of 4")),
        (nn.Conv2d(32, 32, 3, padding=1, stride=2, groups=4), ("stride",)),
        (nn.Conv2d(32, 32, 4, padding=2, groups=4), ("4x4", "odd")),
        (nn.Conv2d(32, 32, 3, padding=5, dilation=5, groups=4), ("halo", "5 squares")),
        (nn.Conv2d(32, 32, 3, padding=0, groups=4), ("pads [0,0,0,0]", "[1,1,1,1]")),
        (nn.Conv2d(32, 64, 3, padding=1, groups=32), ("multiplier 2",)),
    ]
    for i, (g, needles) in enumerate(cases):
        net = gm.GroupNet(g.in_channels, g.out_channels, g.groups)
        net.g = g
        refused(nsg, gm.export(net, tmp_path / f"r{i}.onnx"), "node '/g/Conv'", *needles)
    # a group count that divides the input channels but not the output channels, and a weight of another width
    refused(nsg, hand_built(nsg, 24, 32, 3, 8), "node 'grouped'", "group 3", "32 output channels", "does not divide")
    refused(nsg, hand_built(nsg, 24, 32, 5, 8), "node 'grouped'", "group 5", "does not divide the input channels")
    refused(nsg, hand_built(nsg, 32, 32, 4, 16), "node 'grouped'", "group 4", "16 channels per group", "[Cout,8,kh,kw]")
    # on the 86 planes the needles of tests/test_onnx_geometry.py still hold
    refused(nsg, gm.export(StemNet(nn.Conv2d(86, 32, 3, padding=1, groups=2)), tmp_path / "p2.onnx"), "node '/stem/Conv'",
            "group 2", "43 per group", "depthwise")
    refused(nsg, gm.export(StemNet(nn.Conv2d(86, 172, 3, padding=1, groups=86)), tmp_path / "p86.onnx"), "node '/stem/Conv'",
            "multiplier 2")
