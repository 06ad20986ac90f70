"""The general graph path's host half (nsg_inspect_onnx): which models load, on which path, and what is refused.
No device needed."""
import numpy as np
import pytest

GRAPH_MODELS = [("net_graph_se", 86), ("net_graph_gpool93", 93), ("net_graph_softplus", 86), ("net_graph_views", 86)]
FAMILY_MODELS = ["net_torch_2x64", "net_torch_bn_1x64", "net_torch_sigtanh_eps_1x64"]


def read(golden_dir, name):
    with open(f"{golden_dir}/{name}.onnx", "rb") as f:
        return f.read()


@pytest.mark.parametrize("name,planes", GRAPH_MODELS)
def test_models_outside_the_family_plan_on_the_general_path(nsg, golden_dir, name, planes):
    data = read(golden_dir, name)
    with pytest.raises(nsg.NsgError):  # the family reader refuses them
        nsg.convert_onnx(data)
    info = nsg.inspect_onnx(data, planes)
    assert info["path"] == "graph" and info["precision"] == "fp32"
    assert 0 < info["conv_launches"] < info["launches"] < info["nodes"]
    assert info["param_count"] > 10000 and info["flops_per_position"] > 1e6
    assert info["activation_bytes_per_position"] > 0 and info["activation_bytes"] == 0


def test_the_se_chain_is_fused(nsg, golden_dir):
    """Per SE block: two convs, the pool, two dense layers and ONE launch for sigmoid(w) * x + b, + residual, swish."""
    info = nsg.inspect_onnx(read(golden_dir, "net_graph_se"), 86)
    # stem 1 + 2 blocks x 6 + policy 2 + value conv, mean, flatten, concat, 3 dense + planes + outputs
    assert info["launches"] == 24
    assert info["conv_launches"] == 15


@pytest.mark.parametrize("name", FAMILY_MODELS)
def test_family_models_report_the_specialised_path(nsg, golden_dir, name):
    info = nsg.inspect_onnx(read(golden_dir, name), 86)
    assert info["path"] == "specialised" and info["nodes"] > 0 and info["launches"] == 0


def test_family_model_the_specialised_loader_refuses_goes_to_the_planner(nsg):
    w = nsg.weights.make_random(1, 48, value_channels=8, value_hidden=32, seed=5)
    info = nsg.inspect_onnx(nsg.onnx_io.export_onnx(w), 86)
    assert info["path"] == "graph"


def refused(nsg, data, planes, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, planes)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)
    return str(e.value)


def test_refusals_name_the_node(nsg, golden_dir):
    se = read(golden_dir, "net_graph_se")
    # an op outside the set: Sigmoid renamed to another 7-letter op in the bytes
    msg = refused(nsg, se.replace(b"\x22\x07Sigmoid", b"\x22\x07Softmax"), 86, "Softmax", "node '")
    assert "Sigmoid" in msg or "/" in msg
    # a wrong plane count: the stem conv is named
    refused(nsg, se, 93, "/stem/Conv")
    # `policy` renamed
    refused(nsg, se.replace(b"policy", b"polixy"), 86, "policy")
    # a stride-2 conv: a 3x3 conv of the family exporter with strides [2, 2]
    w = nsg.weights.make_random(1, 48, value_channels=8, value_hidden=32)
    data = nsg.onnx_io.export_onnx(w)
    strided = data.replace(b"\x0a\x07strides\x40\x01\x40\x01", b"\x0a\x07strides\x40\x02\x40\x02", 1)
    assert strided != data
    refused(nsg, strided, 86, "stride")
    # a policy width other than 2187: 26 policy channels
    w2 = dict(w)
    w2["policy_w"], w2["policy_b"] = w["policy_w"][:26], w["policy_b"][:26]
    w2["_meta"] = dict(w["_meta"], policy_channels=26)
    refused(nsg, nsg.onnx_io.export_onnx(w2), 86, "2187", "node '")


@pytest.mark.parametrize("name,planes", GRAPH_MODELS + [("net_torch_2x64", 86)])
def test_truncated_models_are_errors_not_crashes(nsg, golden_dir, name, planes):
    data = read(golden_dir, name)
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], planes)


def view_model(nsg, chain, F=16):
    """A small hand-built model: stem conv (86 -> F), then `chain` (view ops behind an elementwise op).  The chain
    returns its [N,F,9,9] result, which feeds value and draw through the global mean, and the policy tensor it made
    (None: a 1x1 policy conv of the result)."""
    io = nsg.onnx_io
    rng = np.random.default_rng(0)
    inits, nodes = [], []

    def init(name, arr, dtype=np.float32):
        inits.append(io._tensor(name, np.asarray(arr, dtype)))
        return name

    def conv_attrs(k):
        return [io._attr_ints("kernel_shape", [k, k]), io._attr_ints("pads", [k // 2] * 4)]

    nodes.append(io._node("Conv", ["input", init("w0", rng.normal(size=(F, 86, 3, 3)) * 0.05)], ["x"], conv_attrs(3), name="stem"))
    x, pol = chain(nodes, init, "x")
    if pol is None:
        nodes.append(io._node("Conv", [x, init("wp", rng.normal(size=(27, F, 1, 1)))], ["pmap"], conv_attrs(1), name="pconv"))
        nodes.append(io._node("Flatten", ["pmap"], ["policy"], [io._attr_i("axis", 1)], name="pflat"))
    nodes.append(io._node("GlobalAveragePool", [x], ["gp"], name="gap"))
    nodes.append(io._node("Flatten", ["gp"], ["gpf"], [io._attr_i("axis", 1)], name="gflat"))
    for out in ("value", "draw"):
        nodes.append(io._node("Gemm", ["gpf", init(out + "_w", rng.normal(size=(1, F))), init(out + "_b", [0.1])], [out + "_z"],
                              [io._attr_i("transB", 1)], name=out + "_fc"))
        nodes.append(io._node("Sigmoid", [out + "_z"], [out], name=out + "_sig"))
    graph = b"".join(io._f_bytes(1, n) for n in nodes) + io._f_bytes(2, "views") + b"".join(io._f_bytes(5, t) for t in inits)
    graph += io._f_bytes(11, io._value_info("input", ["N", 86, 9, 9]))
    for name, dims in (("policy", ["N", 2187]), ("value", ["N", 1]), ("draw", ["N", 1])):
        graph += io._f_bytes(12, io._value_info(name, dims))
    return io._f_varint(1, 7) + io._f_bytes(7, graph) + io._f_bytes(8, io._f_bytes(1, "") + io._f_varint(2, 17))


@pytest.mark.parametrize("form", ["identity", "same_shape_reshape", "flatten_elementwise", "flatten_gemm",
                                  "unsqueeze_rank5"])
def test_view_ops_behind_an_elementwise_chain(nsg, form):
    """An elementwise chain not yet launched when a view op reads it: the view keeps the chain's shape."""
    io = nsg.onnx_io

    def chain(nodes, init, x):
        nodes.append(io._node("Mul", [x, init("half", [0.5])], ["h"], name="half"))
        shape = lambda n, v: init(n, v, np.int64)  # noqa: E731
        if form == "identity":
            nodes.append(io._node("Identity", ["h"], ["y"], name="ident"))
        elif form == "same_shape_reshape":
            nodes.append(io._node("Reshape", ["h", shape("shape", [-1, 16, 9, 9])], ["y"], name="reshape"))
        elif form == "flatten_elementwise":  # policy = flatten(x * 0.5) * 2 (27 channels)
            nodes.append(io._node("Flatten", ["h"], ["hf"], [io._attr_i("axis", 1)], name="flat"))
            nodes.append(io._node("Mul", ["hf", init("two", [2.0])], ["policy"], name="twice"))
            return "h", "policy"
        elif form == "flatten_gemm":  # policy = fc(flatten(x * 0.5))
            nodes.append(io._node("Flatten", ["h"], ["hf"], [io._attr_i("axis", 1)], name="flat"))
            nodes.append(io._node("Gemm", ["hf", init("fcw", np.ones((2187, 16 * 81)) * 1e-3)], ["policy"],
                                  [io._attr_i("transB", 1)], name="fc"))
            return "h", "policy"
        else:
            nodes.append(io._node("Unsqueeze", ["h", shape("axes", [4])], ["y"], name="unsq"))
        return "y", None

    if form == "unsqueeze_rank5":  # rank 5 is outside the runtime shapes: refused with the node's name
        with pytest.raises(nsg.NsgError, match="unsq"):
            nsg.inspect_onnx(view_model(nsg, chain), 86)
        return
    info = nsg.inspect_onnx(view_model(nsg, chain, F=27 if form == "flatten_elementwise" else 16), 86)
    assert info["path"] == "graph"
