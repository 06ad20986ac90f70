"""The general graph path's host half on one-channel maps (nsg_inspect_onnx, plan_dump): a reduction over the channels
is one kLaunchChanReduce, a one-channel tensor is broadcast over the channels inside the elementwise launch that reads it,
an Expand to the broadcast shape is a view, and what stays outside is refused with the node, the shapes and the reason.
The float32 emulation of gate_models fits the bounds the device test uses, and each listed fault does not.  No device
needed.  Before kLaunchChanReduce and kSrcRowOne every model here but the refused ones was refused at its first gate."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import gate_models as gm
from test_plan_snapshot import PLAN_DUMP

F = gm.F
STEM = 2 * 81 * 9 * 86  # flops of a 3x3 stem per output channel
HEADS = 2 * 2  # value and draw per input channel


@pytest.fixture(scope="module")
def gen():
    import make_onnx_norm_golden
    return make_onnx_norm_golden


@pytest.fixture(scope="module")
def planes(nsg):
    bb = nsg.synth.random_batch(3, 86, seed=31)
    return nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


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


def dump(data, tmp_path):
    """plan_dump's launch lines of the model, by launch name."""
    path = tmp_path / "d.onnx"
    path.write_bytes(data)
    out = subprocess.run([PLAN_DUMP, str(path)], check=True, capture_output=True, text=True).stdout
    assert "ERROR" not in out, out
    return {m.group(1): line for line in out.splitlines() if (m := re.match(r"#\d+ kind=\d+ name=(\S+)", line))}


# ---- plans ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spatial", "token", "flat", "board"])
def test_a_one_channel_gate_is_read_inside_the_elementwise_launch(nsg, kind):
    """stem, heads (mean + 2), planes, outputs = 6 launches (+ the global max and, for the flat rows, the selection Gemm);
    the open one-channel group |g| + 1 is launched (its domain is one channel), op(x, gate) is one launch more."""
    base = 6 + {"spatial": 0, "token": 0, "flat": 2, "board": 1}[kind]
    for op in gm.BINARY:
        for side in ("left", "right"):
            _, data = gm.bcast_model(nsg, kind, op, side)
            info = nsg.inspect_onnx(data, 86)
            assert info["path"] == "graph" and info["launches"] == base + 2, (op, side, info["launches"])
            _, data = gm.bcast_model(nsg, kind, op, side, plain_gate=True)
            assert nsg.inspect_onnx(data, 86)["launches"] == base + 1, (op, side)
            # the Expand to the broadcast shape adds no launch
            _, data = gm.bcast_model(nsg, kind, op, side, expand=True)
            assert nsg.inspect_onnx(data, 86)["launches"] == base + 2, (op, side)


def test_a_gate_from_a_conv_is_one_elementwise_launch(nsg, gen, tmp_path):
    """x * sigmoid(conv1x1_{C->1}(x)): the sigmoid rides in the conv, the Mul is the one elementwise launch."""
    import torch
    import torch.nn as nn
    from test_onnx_linepool import front
    sq = nn.Conv2d(86, 1, 1)
    for i, f in enumerate((lambda x: x * torch.sigmoid(sq(x)), lambda x: torch.sigmoid(sq(x)).expand_as(x) * x)):
        info = nsg.inspect_onnx(export(gen, front(f, mods=(sq,)), tmp_path, f"g{i}.onnx"), 86)
        assert info["conv_launches"] == 4 and info["launches"] == 4 + 1 + 1 + 2, (i, info)
        assert info["flops_per_position"] == 2 * 81 * 86 * (27 + 1) + HEADS * 86


@pytest.mark.parametrize("sigmoid", [False, True])
def test_a_token_score_is_a_dense_launch_read_through_ksrcrowone(nsg, tmp_path, sigmoid):
    """tok * [sigmoid](tok @ w[27,1]): the MatMul is a dense launch of one output channel on token rows (the Sigmoid rides
    in it and opens no one-channel group), its [N,81,1] result a row of stride 16 read at channel 0 by the one Mul launch."""
    _, data = gm.score_model(nsg, sigmoid)
    info = nsg.inspect_onnx(data, 86)
    # stem, score, value, draw; the Mul; the mean; planes and outputs
    assert info["path"] == "graph" and info["conv_launches"] == 4 and info["launches"] == 4 + 1 + 1 + 2
    assert info["flops_per_position"] == STEM * F + 2 * 81 * F * 1 + HEADS * F
    lines = dump(data, tmp_path)
    score = lines["score+gate" if sigmoid else "score"]
    assert " kind=0 " in score and " out=1/16/0/1/s in=0/32/0/27/s " in score and f" dense=0 " in score and f" act={2 if sigmoid else 0} " in score, score
    assert " out=2/32/0/27/s " in lines["y"]
    assert " srcs=2 [mode=0 v=0/32/0/27/s constOff=0 scalar=0x0p+0] [mode=8 v=1/16/0/1/s constOff=0 scalar=0x0p+0] code=3 0:0,0,0 0:1,1,0 4:2,0,1 " in lines["y"]


@pytest.mark.parametrize("kind", ["spatial", "token", "flat"])
def test_one_launch_per_reduction_and_the_flops_of_the_sums(nsg, kind, tmp_path):
    net, data, names = gm.reduce_model(nsg, kind, 1)
    info = nsg.inspect_onnx(data, 86)
    W = 1 + 100 + 1
    rows = 1 if kind == "flat" else 81
    sums = sum(C for op, C in names if op == "ReduceSum")
    assert info["flops_per_position"] == STEM * W + HEADS * W + rows * sums + (2 * F * F * 81 if kind == "flat" else 0)
    lines = dump(data, tmp_path)
    red = {n: l for n, l in lines.items() if " kind=15 " in l}
    assert sorted(red) == sorted(f"r_{op}_{C}" for op, C in names)
    for (op, C) in names:
        line = red[f"r_{op}_{C}"]
        assert f" redMode={gm.OPS.index(op)} " in line and " scale=0x1p+0 " in line
        assert re.search(rf" out=\d+/16/0/1/{'f' if kind == 'flat' else 's'} in=\d+/112/1/{C}/", line), line


def test_a_mean_over_token_and_flat_channels_is_the_sum_times_one_over_c(nsg, tmp_path):
    for kind in ("token", "flat"):
        net, data, names = gm.reduce_model(nsg, kind, 4, ops=["ReduceMean"], widths=[3, 17])
        lines = dump(data, tmp_path)
        for C in (3, 17):
            line = lines[f"r_ReduceMean_{C}"]
            assert " kind=15 " in line and " redMode=2 " in line, line
            assert np.float32(float.fromhex(re.search(r" scale=(\S+) ", line).group(1))) == np.float32(1.0 / C), line


def test_the_dump_of_two_gate_models(nsg, tmp_path):
    """The gate's launches as plan_dump prints them: the source modes 8 (kSrcRowOne), 9 (kSrcBoardOne), 10 (kSrcSquare)."""
    _, data = gm.bcast_model(nsg, "spatial", "Mul", "right")
    lines = dump(data, tmp_path)
    assert " out=1/16/0/1/s " in lines["g_abs+gate"] and " srcs=2 [mode=0 v=0/32/5/1/s constOff=0 scalar=0x0p+0] [mode=3 " in lines["g_abs+gate"]
    assert " out=2/32/0/27/s " in lines["y"]
    assert " srcs=2 [mode=0 v=0/32/0/27/s constOff=0 scalar=0x0p+0] [mode=8 v=1/16/0/1/s constOff=0 scalar=0x0p+0] code=3 0:0,0,0 0:1,1,0 4:2,0,1 " in lines["y"]
    _, data = gm.bcast_model(nsg, "board", "Sub", "left", plain_gate=True)
    lines = dump(data, tmp_path)
    assert " srcs=2 [mode=9 v=1/32/5/1/f constOff=0 scalar=0x0p+0] [mode=0 v=0/32/0/27/s constOff=0 scalar=0x0p+0] code=3 0:0,0,0 0:1,1,0 3:2,0,1 " in lines["y"]
    _, data = gm.square_const_model(nsg, "token")
    line = dump(data, tmp_path)["y"]
    assert "[mode=10 v=-1/0/0/0/f constOff=" in line and re.search(r" consts=\d+\+84:", line), line


def test_both_forms_of_the_axes_and_views_at_any_offset(nsg):
    for kind, axis in (("spatial", 1), ("token", 2), ("token", -1), ("flat", 1), ("flat", -1)):
        for op in ("ReduceMax", "ReduceMin", "ReduceSum"):
            for as_input in (False, True):
                net = gm.GNet(nsg)
                net.stem(F + 7)
                x, ax = gm.rows_of(net, kind, F + 7)
                r = net.reduce(op, net.slice(x, 7, 7 + F, ax, "v"), "r", axis, as_input=as_input)
                net.show(net.widen(r, kind), kind)
                net.heads_of("s", F + 7)
                info = nsg.inspect_onnx(net.data(), 86)
                assert info["path"] == "graph", (kind, axis, op, as_input)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_node_the_shapes_and_the_reason(nsg, gen, tmp_path):
    import torch
    from test_onnx_linepool import front
    cases = [
        (lambda x: x * x.amax(1).unsqueeze(1), "ReduceMax", ("[N,86,9,9]", "keepdims = 0", "[N,9,9] is ambiguous")),
        (lambda x: x * x.sum(1).unsqueeze(1), "ReduceSum", ("[N,86,9,9]", "keepdims = 0")),
        (lambda x: x * x.mean(dim=(2, 3), keepdim=True).expand_as(x), "Expand", ("[N,86,1,1]", "[N,86,9,9]", "only a one-channel tensor expanded over the channels")),
        (lambda x: x * x.amax(3, keepdim=True).expand_as(x), "Expand", ("[N,86,9,1]", "line tensor")),
        (lambda x: x * (x.mean(3, keepdim=True) * x.amax(1, keepdim=True).amax(3, keepdim=True)), "Mul", ("one-channel line operand [N,1,9,1]", "[N,86,9,1]", "not over the channels of lines")),
        (lambda x: x * x.prod(1, keepdim=True), "ReduceProd", ("op 'ReduceProd'", "outside the supported op set")),
        (lambda x: x * x.sum(dim=(1, 2), keepdim=True), "ReduceSum", ("[N,86,9,9]", "over the channels only")),
        (lambda x: x.mean(1, keepdim=True) * x, "ReduceMean", ("over the squares only",)),
        (lambda x: x * torch.softmax(x.amax(1, keepdim=True).flatten(1), 1).reshape(-1, 1, 9, 9), "Softmax", ("Softmax on",)),
    ]
    for i, (f, op, needles) in enumerate(cases):
        refused(nsg, export(gen, front(f), tmp_path, f"r{i}.onnx"), f"/{op}", *needles)


def test_hand_built_refusals(nsg):
    def model(build):
        net = gm.GNet(nsg)
        net.stem(F)
        y = build(net)
        net.show(y, "spatial")
        net.heads_of("s", F)
        return net.data()

    # an Expand whose target is not what its reader broadcasts to
    refused(nsg, model(lambda n: n.node("Relu", [n.node("Expand", [n.slice("s", 5, 6, 1, "g"), n.const("sh", [1, F, 9, 9], np.int64)], "e")], "y")),
            "node 'y'", "[N,1,9,9] behind an Expand to [N,27,9,9]", "only Add, Sub, Mul, Div, Max and Min read")
    # a per-square PRelu slope and a run-time slope stay outside
    refused(nsg, model(lambda n: n.node("PRelu", ["s", n.const("sl", np.full((1, 9, 9), 0.25))], "y")), "node 'y'", "[1,9,9]", "[N,27,9,9]")
    refused(nsg, model(lambda n: n.node("PRelu", ["s", n.slice("s", 5, 6, 1, "g")], "y")), "node 'y'", "the slope must be a constant")
    # keepdims 0 on flat rows is refused like the other two
    def flat_sum(n):
        fm = n.flat_max("s")
        r = n.node("Unsqueeze", [n.reduce("ReduceSum", fm, "r", 1, keepdims=0), n.const("ax1", [1], np.int64)], "r1")
        return n.node("Mul", ["s", n.node("Reshape", [r, n.const("to4", [-1, 1, 1, 1], np.int64)], "r4")], "y")
    refused(nsg, model(flat_sum), "node 'r'", "[N,27]", "keepdims = 0", "keeps the axis")
    # a per-square constant of the wrong size
    refused(nsg, model(lambda n: n.node("Mul", ["s", n.const("m", np.ones((1, 9, 1)))], "y")), "node 'y'", "[1,9,1]", "[N,27,9,9]")


def test_truncated_models_are_errors_not_crashes(nsg):
    _, data, _ = gm.reduce_model(nsg, "spatial", 1, widths=[3, 17])
    for cut in np.linspace(1, len(data) - 1, 25).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)


@pytest.mark.parametrize("opset", [13, 17])
@pytest.mark.parametrize("block,expand", [("scse", False), ("scse", True), ("cbam", False)])
def test_exported_gate_blocks_plan_on_the_graph_path(nsg, gen, tmp_path, block, expand, opset):
    net = gm.randomize(gm.gate_net(block, expand=expand), 5)
    data = export(gen, net, tmp_path, opset=opset)
    for op in {"scse": (b"Expand",) if expand else (), "cbam": (b"ReduceSum", b"ReduceMax", b"Concat")}[block]:
        assert op in data, op
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32"
    Fw = net.F
    if block == "scse":
        # stem, fc1, fc2, the squeeze conv, policy, value, draw; two means; x * c + x * g in one launch; planes and outputs
        assert info["conv_launches"] == 7 and info["launches"] == 7 + 2 + 1 + 2
        assert info["flops_per_position"] == STEM * Fw + 2 * 2 * Fw * (Fw // 4) + 2 * 81 * Fw * (1 + 27) + HEADS * Fw
    else:
        # stem, the 7x7 conv, policy, value, draw; the sum (with its factor as one elementwise launch) and the max, the
        # Concat of the two maps, x * gate, the mean; planes and outputs
        assert info["conv_launches"] == 5 and info["launches"] == 5 + 3 + 1 + 1 + 1 + 2
        assert info["flops_per_position"] == STEM * Fw + 81 * Fw + 2 * 81 * 49 * 2 + 2 * 81 * Fw * 27 + HEADS * Fw


# ---- the bounds of the device test, on the host -------------------------------------------------------------------------
def test_the_emulation_fits_the_bounds_and_the_faults_do_not(nsg, planes):
    off, C = 1, 100  # the widest view: the element behind it is the poisoned channel
    net, _, _ = gm.reduce_model(nsg, "spatial", off, fine=True, exp=-11)
    buf = gm.reduce_inputs(net, planes, "spatial", 0, off + 100 + 1)
    rows = buf[..., off:off + C]
    assert not gm.sums_exact(buf[..., off:off + 100], -11)  # the fine grid does round
    worst = {}
    for op in ("ReduceSum", "ReduceMean"):
        ref = rows.sum(axis=-1) / (C if op == "ReduceMean" else 1)
        bound = gm.sum_bound(rows, op == "ReduceMean")
        for fault in (None, "drop_last", "tail_past", "mean_before_last_add"):
            if fault == "mean_before_last_add" and op == "ReduceSum":
                continue
            err = np.abs(gm.emulate_reduce(buf, off, C, op, fault).astype(np.float64) - ref)
            worst[op, fault] = float((err / bound).max())
    print(worst)
    for (op, fault), r in worst.items():
        assert (r <= 1.0) if fault is None else (r > 1.0), (op, fault, r)
    # on the coarse grid the sums are exact: the bound is zero, and a neighbour's rows give other bits
    net, _, _ = gm.reduce_model(nsg, "spatial", off)
    buf = gm.reduce_inputs(net, planes, "spatial", 0, off + 100 + 1)
    rows = buf[..., off:off + C]
    assert gm.sums_exact(buf[..., off:off + 100], -3)
    assert np.array_equal(gm.emulate_reduce(buf, off, C, "ReduceSum"), rows.sum(axis=-1).astype(np.float32))
    for fault in ("next_board", "drop_last", "tail_past"):
        assert not np.array_equal(gm.emulate_reduce(buf, off, C, "ReduceSum", fault), rows.sum(axis=-1).astype(np.float32)), fault
    # max and min are exact
    for op in ("ReduceMax", "ReduceMin"):
        ref = (rows.max if op == "ReduceMax" else rows.min)(axis=-1)
        assert np.array_equal(gm.emulate_reduce(buf, off, C, op), ref.astype(np.float32))
        # (a dropped last element shows in a max or min only where it is the extreme, and the poison of +1e30 behind the
        # view never is a minimum: the sums above carry those two faults, the range logic is one template for all three)
        for fault in ("next_board", "tail_past") if op == "ReduceMax" else ("next_board",):
            assert not np.array_equal(gm.emulate_reduce(buf, off, C, op, fault), ref.astype(np.float32)), (op, fault)
    # the broadcast: channel 0 of the gate's own row
    x, gate = buf[..., :F], np.abs(buf[..., 5:5 + F]) + 1.0
    ref = (em_f32(x * gate[..., :1])).astype(np.float32)
    assert np.array_equal(gm.emulate_bcast(x, gate), ref)
    for fault in ("wrong_channel", "next_board"):
        assert not np.array_equal(gm.emulate_bcast(x, gate, fault), ref), fault


def em_f32(a):
    import elt_models
    return elt_models.f32(a)
