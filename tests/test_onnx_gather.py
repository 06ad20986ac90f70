"""Gather with constant indices and board flips on the host ("indexing"): the plans
nsg_inspect_onnx reports for the models of tests/gather_models.py, the refusals, and the references that
tests/test_gpu_onnx_gather.py holds the device to.  No device needed."""
import numpy as np
import pytest

import gather_models as gm


@pytest.fixture(scope="module")
def planes(nsg):
    """Three of the seeded positions of the sibling files, as float64 planes."""
    bb = nsg.synth.random_batch(3, 86, seed=31)
    return nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def stem_flops(W):
    return 2 * 81 * 9 * 86 * W + 2 * 2 * W


def select_flops(c):
    if not gm.selects_of(c):
        return 0
    return 2 * c.C * gm.WIN * 81 if c.out_kind == "flat" else 2 * 81 * c.C * gm.WIN


# ---- the plans -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opset", [13, 17])
@pytest.mark.parametrize("name", list(gm.CASES))
def test_every_form_is_one_launch(nsg, name, opset):
    """launches = the baseline's (stem, mean, value, draw; planes and outputs) plus one per gather or flip, plus the
    selection where the policy needs one.  A Slice in front adds none, the flattened view is read where it lies (no
    flatten launch), and a gather adds nothing to the FLOPs."""
    c = gm.case(nsg, name, opset)
    base = nsg.inspect_onnx(gm.baseline(nsg, c.W), 86)
    assert base["path"] == "graph" and base["launches"] == 4 + 2 and base["conv_launches"] == 3
    info = nsg.inspect_onnx(c.data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    sel = gm.selects_of(c)
    assert info["launches"] == base["launches"] + gm.gathers_of(name) + sel, info
    assert info["conv_launches"] == base["conv_launches"] + sel
    assert info["flops_per_position"] == stem_flops(c.W) + select_flops(c)


@pytest.mark.parametrize("name", list(gm.PADS))
def test_the_pad_models_plan(nsg, name):
    c = gm.pad_case(nsg, name)
    info = nsg.inspect_onnx(c.data, 86)
    # stem, 1 / stem, the gather, the selection with the Reciprocal behind it, mean, value, draw; planes and outputs
    assert info["path"] == "graph" and info["launches"] in (7 + 2, 8 + 2), info


def test_integer_indexing_of_a_head_costs_what_its_slice_twin_costs(nsg):
    """o[:, 0] and o[:, 1] of a flat [N,2] are views: no launch, as o[:, 0:1] and o[:, 1:2] are."""
    a = nsg.inspect_onnx(gm.two_heads(nsg, "gather").data(), 86)
    b = nsg.inspect_onnx(gm.two_heads(nsg, "slice").data(), 86)
    assert a["path"] == b["path"] == "graph"
    assert a["launches"] == b["launches"] and a["conv_launches"] == b["conv_launches"]
    assert a["flops_per_position"] == b["flops_per_position"]
    # stem, mean, fc, two sigmoids; planes and outputs
    assert a["launches"] == 5 + 2, a


def test_a_list_of_one_on_a_flat_tensor_is_a_launch_and_a_scalar_is_not(nsg):
    net = gm.two_heads(nsg, "gather")
    scalar = nsg.inspect_onnx(net.data(), 86)["launches"]
    net.consts["i0"] = np.asarray([0], np.int64)  # o[:, [0]]: flat [N,1] through the kernel
    assert nsg.inspect_onnx(net.data(), 86)["launches"] == scalar + 1


def test_a_scalar_index_into_the_flattened_view(nsg):
    """x.flatten(1)[:, i] is a flat [N]: one launch that reads the spatial rows, and a value head can show it."""
    net = gm.two_heads(nsg, "gather")
    base = nsg.inspect_onnx(net.data(), 86)["launches"]
    i = [n[4] for n in net.nodes].index("value_pick")
    net.consts["i0"] = np.asarray(-5, np.int64)
    net.nodes[i] = ("Gather", ["policy", "i0"], ["value_z"], {"axis": 1}, "value_pick")
    assert nsg.inspect_onnx(net.data(), 86)["launches"] == base + 1


# ---- the refusals ----------------------------------------------------------------------------------------------------
def refused(nsg, kind):
    """A model around one Gather that the planner refuses; returns its bytes."""
    W = 24
    c = gm.GatherCase(nsg, "chan", W, idx=[1, 2, 3])
    net = c.net
    i = [n[4] for n in net.nodes].index("gather")
    op, ins, outs, at, nm = net.nodes[i]

    def put(data, idx, axis, before=()):
        net.consts["idx"] = np.asarray(idx, np.int64)
        net.nodes[i:i + 1] = list(before) + [("Gather", [data, "idx"], outs, {"axis": axis}, nm)]

    tokens = [("Reshape", ["s", net.const("r_to3", [-1, W, 81], np.int64)], ["r_c3"], {}, "r_c3"),
              ("Transpose", ["r_c3"], ["r_tok"], {"perm": [0, 2, 1]}, "r_tok")]
    if kind == "runtime_indices":
        net.nodes[i:i + 1] = [("Gather", ["s", "gpf"], outs, {"axis": 1}, nm)]
        net.nodes.sort(key=lambda n: n[4] not in ("s", "gap", "gflat"))  # the mean before its reader
    elif kind == "rank2_indices":
        put("s", [[0, 1], [2, 3]], 1)
    elif kind == "index_too_large":
        put("s", [0, 24], 1)
    elif kind == "index_too_small":
        put("s", [-25], 1)
    elif kind == "axis0":
        put("s", [0], 0)
    elif kind == "spatial_scalar":
        put("s", 3, 1)
    elif kind == "token_squares_not_81":
        put("r_tok", np.arange(27), 1, tokens)
    elif kind == "flat_axis2":
        put("gp", [0], 2)  # [N,24,1,1]
        net.nodes.sort(key=lambda n: n[4] not in ("s", "gap"))
    elif kind == "spatial_axis2":
        put("s", [0, 1], 2)
    elif kind == "spatial_axis3":
        put("s", [0, 1], -1)
    elif kind == "chan3":
        put("r_c3", [0, 1], 1, tokens[:1])
    elif kind == "channel_last":
        put("r_cl", [0, 1], 3, [("Transpose", ["s"], ["r_cl"], {"perm": [0, 2, 3, 1]}, "r_cl")])
    return net.data()


REFUSALS = {
    "runtime_indices": ["[N,24,9,9]", "computed at run time"],
    "rank2_indices": ["[N,24,9,9]", "[2,2]", "rank 2"],
    "index_too_large": ["[N,24,9,9]", "index 24", "extent 24"],
    "index_too_small": ["[N,24,9,9]", "index -25", "extent 24"],
    "axis0": ["[N,24,9,9]", "axis 0"],
    "spatial_scalar": ["[N,24,9,9]", "[N,9,9]", "x[:, c:c+1]"],
    "token_squares_not_81": ["[N,81,24]", "[27]", "81"],
    "flat_axis2": ["[N,24,1,1]", "axis 2", "flat"],
    "spatial_axis2": ["[N,24,9,9]", "axis 2", "board axis"],
    "spatial_axis3": ["[N,24,9,9]", "axis 3", "board axis"],
    "chan3": ["[N,24,81]", "outside the token-view and attention patterns"],
    "channel_last": ["[N,9,9,24]", "channel-last view"],
}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refusals_name_the_node_the_shapes_and_the_reason(nsg, kind):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(refused(nsg, kind), 86)
    msg = str(e.value)
    assert "node 'gather' (Gather)" in msg, msg
    for w in REFUSALS[kind]:
        assert w in msg, (w, msg)


def test_a_gather_of_a_line_tensor_keeps_the_line_handler(nsg):
    c = gm.GatherCase(nsg, "chan", 24, idx=[1, 2, 3])
    net = c.net
    i = [n[4] for n in net.nodes].index("gather")
    op, ins, outs, at, nm = net.nodes[i]
    net.nodes[i:i + 1] = [("AveragePool", ["s"], ["lines"], {"kernel_shape": [1, 9]}, "rank_pool"), ("Gather", ["lines", "idx"], outs, at, nm)]
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(net.data(), 86)
    assert "node 'gather' (Gather)" in str(e.value) and "line" in str(e.value), str(e.value)


def test_a_gather_of_constants_is_still_folded_on_the_host(nsg):
    """Shape / Gather / Concat in front of a Reshape, as the exporter writes x.reshape(x.size(0), -1)."""
    c = gm.GatherCase(nsg, "chan", 27, idx=np.arange(27)[::-1])
    net = c.net
    i = [n[4] for n in net.nodes].index("pflat")
    net.const("zero", 0, np.int64)
    net.const("minus1", [-1], np.int64)
    net.const("ax0", [0], np.int64)
    net.nodes[i:i + 1] = [("Shape", ["g"], ["shp"], {}, "shp"), ("Gather", ["shp", "zero"], ["n"], {"axis": 0}, "batch"),
                          ("Unsqueeze", ["n", "ax0"], ["n1"], {}, "n1"), ("Concat", ["n1", "minus1"], ["to"], {"axis": 0}, "to"),
                          ("Reshape", ["g", "to"], ["policy"], {}, "pflat")]
    info = nsg.inspect_onnx(net.data(), 86)
    assert info["launches"] == 4 + 2 + 1


def flip_model(nsg, starts, ends, steps, axes, W=27):
    c = gm.GatherCase(nsg, "flip", W)
    for nm, val in (("st", starts), ("en", ends), ("sp", steps), ("ax", axes)):
        c.net.consts["flip00_" + nm] = np.asarray(val, np.int64)
    return c.net.data()


@pytest.mark.parametrize("starts,ends,steps,axes", [
    ([0], [9], [2], [3]),            # every other file
    ([-1], [-10], [-2], [3]),
    ([-1], [0], [-1], [3]),          # files 8..1: part of the axis
    ([7], [-10], [-1], [2]),         # ranks 7..0
    ([-1], [-10], [-1], [1]),        # the channels reversed is a Gather, not a Slice
    ([-1, -1], [-10, -10], [-1, -1], [3, 3]),
])
def test_other_steps_keep_their_message(nsg, starts, ends, steps, axes):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(flip_model(nsg, starts, ends, steps, axes), 86)
    assert "node 'flip00' (Slice)" in str(e.value) and "Slice with a step other than 1" in str(e.value), str(e.value)


@pytest.mark.parametrize("starts,ends", [([-1], [-10]), ([8], [-100]), ([100], [gm.INT64_LOW])])
def test_the_ways_to_write_a_whole_flip(nsg, starts, ends):
    info = nsg.inspect_onnx(flip_model(nsg, starts, ends, [-1], [-1]), 86)
    assert info["launches"] == 4 + 2 + 1


@pytest.mark.parametrize("name", ["chan_w97_m17_at4", "toksq_w24_repeated_at5", "flat_policy_map", "flip_both_w24"])
def test_truncated_models_are_errors_not_crashes(nsg, name):
    data = gm.case(nsg, name).data
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)


# ---- the exported module ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opset", [13, 17])
def test_the_exported_module_plans_like_its_slice_twin(nsg, tmp_path, opset):
    data = gm.export(gm.gather_net(), tmp_path / "g.onnx", opset)
    assert b"Gather" in data and b"Slice" in data
    info = nsg.inspect_onnx(data, 86)
    twin = nsg.inspect_onnx(gm.export(gm.gather_net(slice_heads=True), tmp_path / "t.onnx", opset), 86)
    assert info["path"] == twin["path"] == "graph"
    assert info["launches"] == twin["launches"], (info, twin)
    assert info["flops_per_position"] == twin["flops_per_position"]
    F = 32
    # stem, f twice, the policy Linear, fc
    assert info["conv_launches"] == 5
    assert info["flops_per_position"] == 2 * 81 * 9 * 86 * F + 2 * (2 * 81 * 9 * 24 * F) + 2 * 81 * F * 32 + 2 * F * 2
    # ... the channel index, two flips, the policy map (4 gathers), the average of the two branches, the mean over the
    # squares, two sigmoids; planes and outputs
    assert info["launches"] - info["conv_launches"] - 2 in (8, 9), info


# ---- the references --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gm.CASES))
def test_the_reference_has_something_to_compare(nsg, planes, name):
    c = gm.case(nsg, name)
    inp, ref, bound = c.expected(planes)
    assert ref.shape == (3, 2187) and not bound.any()
    assert np.array_equal(ref, gm.em.f32(ref)) and np.isfinite(ref).all()
    assert len(np.unique(ref)) > 50, len(np.unique(ref))
    if c.form == "flip":
        y = inp["s"][:, c.off:c.off + c.K]
        assert np.array_equal(c.ref(inp), y) == c.twice  # a flip moves something; twice moves nothing


@pytest.mark.parametrize("name", list(gm.PADS))
def test_the_pad_models_hold_an_inf_no_index_reads(nsg, planes, name):
    c = gm.pad_case(nsg, name)
    inp, ref, bound = c.expected(planes)
    assert np.isfinite(ref).all() and float(ref.min()) > 0.0 and float(bound.max()) < 1e-3
    assert len(np.unique(ref)) > 50
    assert int(c.idx.min()) >= -c.K and c.off > 0  # channel 0 of the rows lies in front of the view
