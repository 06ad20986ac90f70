"""The product of two run-time token tensors on the host ("run-time products"): the plans
nsg_inspect_onnx reports for the models of tests/bmm_models.py, the refusals, and the honesty of the bounds that
tests/test_gpu_onnx_bmm.py holds the device to.  No device needed."""
import numpy as np
import pytest

import bmm_models as bm
import reduction_models as rm
from reduction_models import ratio


@pytest.fixture(scope="module")
def planes(nsg):
    """Five of the seeded positions of the sibling files, as float64 planes."""
    bb = nsg.synth.random_batch(5, 86, seed=31)
    return nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def stem_flops(W):
    return 2 * 81 * 9 * 86 * W + 2 * 2 * W


# ---- the plans -------------------------------------------------------------------------------------------------------
PLANS = ["nt_k4", "nt_k16", "nt_k20_at4", "nt_k64_at20", "nt_k80", "gram_k80", "gram_k81_spatial", "nn_m16", "nn_m27_at4",
         "nn_m68_at20", "nn_m81", "ntnn", "nt_k64_sigmoid", "nt_k256_relu"]


@pytest.mark.parametrize("name", PLANS)
def test_a_product_is_one_launch(nsg, name):
    """launches = the baseline's (stem, mean, value, draw; planes and outputs) plus one per product, plus the selection
    where the policy needs one; a scalar Div / Mul and an activation behind the product add none, a view at a multiple
    of 4 adds none; the FLOPs are the formula's."""
    case = bm.case(nsg, name)
    base = nsg.inspect_onnx(bm.baseline(nsg, case.W), 86)
    assert base["path"] == "graph" and base["launches"] == 4 + 2 and base["conv_launches"] == 3
    info = nsg.inspect_onnx(case.data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    products = 2 if case.form == "ntnn" else 1
    select = 0 if case.form == "nt" or case.C == bm.WIN else 1
    assert info["launches"] == base["launches"] + products + select, info
    assert info["conv_launches"] == base["conv_launches"] + select
    flops = {"nt": 2 * 81 * 81 * case.K, "nn": 2 * 81 * 81 * case.M, "ntnn": 2 * 81 * 81 * (case.K + case.M)}[case.form]
    assert info["flops_per_position"] == stem_flops(case.W) + flops + select * 2 * 81 * case.C * bm.WIN


def test_a_view_off_the_multiples_of_four_is_copied_first(nsg):
    at4, at2 = bm.case(nsg, "nt_k20_at4"), bm.BmmCase(nsg, "nt", K=20, offs=(2, 24))
    a, b = nsg.inspect_onnx(at4.data, 86), nsg.inspect_onnx(at2.data, 86)
    assert b["launches"] == a["launches"] + 1
    both = nsg.inspect_onnx(bm.case(nsg, "nt_k20_at2").data, 86)
    assert both["launches"] == a["launches"] + 2
    assert a["flops_per_position"] - stem_flops(at4.W) == b["flops_per_position"] - stem_flops(at2.W)


def test_what_does_not_fold_stays_a_launch(nsg):
    """A per-channel Mul, an Add, and a scalar Mul behind the activation are elementwise launches of their own."""
    plain = nsg.inspect_onnx(bm.case(nsg, "nt_k16").data, 86)["launches"]
    for tail in ("row_mul", "add", "mul_after_act"):
        case = bm.BmmCase(nsg, "nt", K=16, offs=(16, 0))
        net = case.net
        i = [n[4] for n in net.nodes].index("show")
        op, ins, outs, at, nm = net.nodes[i]
        if tail == "row_mul":
            extra = [("Mul", ["prod", net.const("per_column", np.arange(81) / 8.0)], ["tail"], {}, "tail")]
        elif tail == "add":
            extra = [("Add", ["prod", net.const("one", [1.0])], ["tail"], {}, "tail")]
        else:
            extra = [("Sigmoid", ["prod"], ["sg"], {}, "sg"), ("Mul", ["sg", net.const("two", [2.0])], ["tail"], {}, "tail")]
        net.nodes[i:i + 1] = extra + [(op, ["tail"] + ins[1:], outs, at, nm)]
        assert nsg.inspect_onnx(net.data(), 86)["launches"] == plain + 1, tail


# ---- the refusals ----------------------------------------------------------------------------------------------------
def rewired(nsg, kind):
    case = bm.BmmCase(nsg, "nt", K=16, offs=(16, 0), width=97)
    net = case.net
    i = [n[4] for n in net.nodes].index("product")
    for nm, val in (("st", [16]), ("en", [97]), ("ax", [2])):
        net.const("wide_" + nm, val, np.int64)
    wide = ("Slice", ["tok", "wide_st", "wide_en", "wide_ax"], ["wide"], {}, "wide")  # [N,81,81]
    if kind == "transposed_first":  # [N,K,81] x [N,81,M]
        net.nodes[i:i + 1] = [wide, ("Transpose", ["op0"], ["at"], {"perm": [0, 2, 1]}, "a_t"), ("MatMul", ["at", "wide"], ["prod"], {}, "product")]
    elif kind == "spatial":
        net.nodes[i] = ("MatMul", ["op0", "s"], ["prod"], {}, "product")
    elif kind == "flat":
        net.nodes[i] = ("MatMul", ["op0", "gpf"], ["prod"], {}, "product")
        net.nodes.sort(key=lambda n: n[4] not in ("s", "gap", "gflat"))  # the mean before its reader
    elif kind == "inner":  # [N,81,16] x [N,81,16]: 16 against 81
        net.nodes[i] = ("MatMul", ["op0", "op1"], ["prod"], {}, "product")
    elif kind == "inner_nt":  # [N,81,81] x [N,16,81]
        net.nodes[i:i + 1] = [wide, ("MatMul", ["wide", "bt"], ["prod"], {}, "product")]
    elif kind == "second_consumer":
        net.nodes[i:i + 1] = [net.nodes[i], ("MatMul", ["op0", "bt"], ["prod_again"], {}, "again"), ("Add", ["prod", "prod_again"], ["sum"], {}, "sum")]
        j = [n[4] for n in net.nodes].index("show")
        op, ins, outs, at, nm = net.nodes[j]
        net.nodes[j] = (op, ["sum"] + ins[1:], outs, at, nm)
    return net.data()


REFUSALS = {
    "transposed_first": ("product", ["[N,16,81]", "[N,81,81]", "first operand is transposed"]),
    "spatial": ("product", ["[N,81,16]", "[N,97,9,9]", "flat or spatial operand"]),
    "flat": ("product", ["[N,81,16]", "[N,97]", "flat or spatial operand"]),
    "inner": ("product", ["[N,81,16]", "inner dimensions disagree (16 and 81)"]),
    "inner_nt": ("product", ["[N,81,81]", "[N,16,81]", "inner dimensions disagree (81 and 16)"]),
    "second_consumer": ("product", ["[N,81,16]", "[N,16,81]", "'bt'", "second consumer"]),
}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refusals_name_the_node_both_shapes_and_the_reason(nsg, kind):
    node, words = REFUSALS[kind]
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(rewired(nsg, kind), 86)
    msg = str(e.value)
    assert f"node '{node}' (MatMul)" in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_a_softmax_on_the_result_stays_outside(nsg):
    case = bm.case(nsg, "nt_k16")
    net = case.net
    i = [n[4] for n in net.nodes].index("show")
    op, ins, outs, at, nm = net.nodes[i]
    net.nodes[i:i + 1] = [("Softmax", ["prod"], ["sm"], {"axis": -1}, "sm"), (op, ["sm"] + ins[1:], outs, at, nm)]
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(net.data(), 86)
    assert "node 'sm' (Softmax)" in str(e.value)


def test_the_attention_pattern_keeps_precedence_and_its_message(nsg):
    """A product of two 4-D run-time tensors that is neither q k^T nor probs x v (here probs x v^T) is still refused by
    the attention pattern, in its words."""
    case = rm.AttCase(nsg, 16, 4)
    net = case.net
    i = [n[4] for n in net.nodes].index("vh")
    net.nodes[i] = ("Transpose", ["v4"], ["vh"], {"perm": [0, 2, 3, 1]}, "vh")
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(net.data(), 86)
    assert "outside the attention pattern" in str(e.value)


@pytest.mark.parametrize("name", ["nt_k20_at4", "nn_m68_at20", "ntnn"])
def test_truncated_models_are_errors_not_crashes(nsg, name):
    data = bm.case(nsg, name).data
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)


@pytest.mark.parametrize("opset", [13, 17])
def test_the_exported_module_plans_with_three_products(nsg, tmp_path, opset):
    """The sigmoid attention is NT (with the scalar Div and the Sigmoid in it) and NN, the policy head NT with its Mul."""
    data = bm.export(bm.head_net(), tmp_path / "head.onnx", opset)
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["attention_launches"] == 0
    # stem, q, k, v, NT, NN, proj (with the Div and the residual: an elementwise launch more), from, to, NT, mean, value, draw
    F, d = 32, 16
    assert info["conv_launches"] == 1 + 4 + 2 + 2
    flops = 2 * 81 * 9 * 86 * F + 4 * 2 * 81 * F * F + 2 * 2 * 81 * F * d + 2 * 2 * F + 2 * 81 * 81 * (F + F + d)
    assert info["flops_per_position"] == flops
    assert info["launches"] - info["conv_launches"] - 2 in (4, 5), info  # three products, the mean, and at most one elementwise launch


# ---- the bounds ------------------------------------------------------------------------------------------------------
def all_parts():
    return [(n, p) for n in bm.CASES for p in bm.parts_of(n)]


@pytest.mark.parametrize("name,part", all_parts(), ids=[f"{n}-{p}" for n, p in all_parts()])
def test_the_emulation_is_inside_the_bound(nsg, planes, name, part):
    case = bm.case(nsg, name, part)
    inp, ref, bound = case.expected(planes)
    assert np.isfinite(ref).all() and np.isfinite(bound).all()
    got = case.select(case.emulate(inp))
    if case.exact and case.act in (None, "relu"):
        assert not bound.any()
        np.testing.assert_array_equal(got, ref.astype(np.float32))
        assert np.array_equal(ref, bm.em.f32(ref))
    r = ratio(got, ref, bound)
    print(name, part, "emulation error / bound", r, "largest bound", float(bound.max()), "largest |ref|", float(np.abs(ref).max()))
    assert r <= 1.0
    if case.act == "sigmoid":  # neither saturated nor flat: a sigmoid that ignored its argument would show
        assert 0.05 < float(ref.std()) and 0.02 < float(np.mean((ref > 0.1) & (ref < 0.9)))


@pytest.mark.parametrize("fault", list(bm.FAULTS))
def test_each_fault_falls_outside_the_bound(nsg, planes, fault):
    for name in bm.FAULTS[fault]:
        hit = False
        for part in bm.parts_of(name):
            case = bm.case(nsg, name, part)
            inp, ref, bound = case.expected(planes)
            assert ratio(case.select(case.emulate(inp)), ref, bound) <= 1.0
            got = case.select(case.emulate(inp, fault))
            hit = hit or (not np.isfinite(got).all()) or ratio(got, ref, bound) > 1.0
        assert hit, (fault, name)


def test_the_rounded_cases_are_rounded(nsg, planes):
    """On the fine stem the float32 product differs from the float64 one: the bound is in use, not idle."""
    for name in bm.ROUNDED:
        case = bm.case(nsg, name)
        inp, ref, bound = case.expected(planes)
        got = case.select(case.emulate(inp))
        assert (got != ref.astype(np.float32)).mean() > 0.05 or case.act == "relu", name
        assert float(bound.max()) > 0.0
