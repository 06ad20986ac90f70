"""Token-mixing MLPs on the host ("token mixing"): the plans nsg_inspect_onnx reports for the
models of tests/mix_models.py, the refusals, and the honesty of the bounds that tests/test_gpu_onnx_tokenmix.py holds
the device to.  No device needed.  Before kLaunchTokenMix every model here was refused at its first MatMul."""
import numpy as np
import pytest

import mix_models as mm
from reduction_models import ratio
from test_onnx_bmm import REFUSALS as BMM_REFUSALS, rewired as bmm_rewired


@pytest.fixture(scope="module")
def planes(nsg):
    """Five of the seeded positions of the sibling files, as float64 planes."""
    bb = nsg.synth.random_batch(5, 86, seed=31)
    return nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def inspect(nsg, data):
    info = nsg.inspect_onnx(data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    return info


# ---- the plans -------------------------------------------------------------------------------------------------------
PLANS = ["one_c27", "one_c24_relu", "one_c65_at4", "one_c80_spatial", "one_c64_spatial_at4", "two_c27_d1", "two_c24_d16",
         "two_c64_d20_at4", "two_c65_d81", "two_c80_d100", "two_c27_d336", "r_two_c27_d100_gelu", "pad_two_exp_recip_d20"]


@pytest.mark.parametrize("name", PLANS)
def test_a_pattern_is_one_launch(nsg, name):
    """One launch more than the same model without the pattern (the baseline reads the same channels at offset 0: a view
    at a multiple of 4 costs the pattern nothing), whatever biases and activations it holds; the FLOPs are the formula's,
    2 * 81 * D * C per stage; the conv count is the baseline's."""
    case = mm.case(nsg, name)
    base = inspect(nsg, mm.case(nsg, name, pattern=False, off=0, width=case.C, src="tokens").data)
    info = inspect(nsg, case.data)
    assert info["launches"] == base["launches"] + 1, (info, base)
    assert info["conv_launches"] == base["conv_launches"]
    stem = (2 * 81 * 9 * 86 + 2 * 2) * (case.W - case.C)  # the wider stem and heads of a case that reads a view
    assert info["flops_per_position"] - base["flops_per_position"] - stem == 2 * 81 * case.D1 * case.C * (2 if case.two else 1)


def test_biases_and_activations_add_no_launch(nsg):
    bare = inspect(nsg, mm.MixCase(nsg, 24, D=20, bias=(False, False)).data)
    full = inspect(nsg, mm.MixCase(nsg, 24, D=20, act1="gelu", act2="sigmoid").data)
    assert full["launches"] == bare["launches"] and full["flops_per_position"] == bare["flops_per_position"]
    one = inspect(nsg, mm.MixCase(nsg, 24, bias=(False, False)).data)
    assert inspect(nsg, mm.MixCase(nsg, 24, act1="relu").data)["launches"] == one["launches"] == bare["launches"]


def test_a_view_off_the_multiples_of_four_is_copied_first(nsg):
    for a, b in (("two_c64_d20_at4", dict(off=2)), ("one_c65_at4", dict(off=6)), ("one_c64_spatial_at4", dict(off=3, width=72))):
        at4, off = mm.case(nsg, a), mm.case(nsg, a, **b)
        i4, io = inspect(nsg, at4.data), inspect(nsg, off.data)
        assert io["launches"] == i4["launches"] + 1, (a, i4, io)
        stem = 2 * 81 * 9 * 86 + 2 * 2
        assert io["flops_per_position"] - stem * off.W == i4["flops_per_position"] - stem * at4.W


@pytest.mark.parametrize("tail", ["layer_scale", "residual", "gate"])
def test_what_does_not_fold_stays_a_launch(nsg, tail):
    """A per-channel Mul (LayerScale), a residual and a gate behind the Transpose back are one elementwise launch."""
    plain = inspect(nsg, mm.MixCase(nsg, 64, back="tokens").data)["launches"]
    case = mm.MixCase(nsg, 64, back="tokens")
    net = case.net
    i = [n[4] for n in net.nodes].index("select")
    op, ins, outs, at, nm = net.nodes[i]
    if tail == "layer_scale":
        extra = ("Mul", ["ytok", net.const("per_channel", np.arange(64) / 8.0)], ["tail"], {}, "tail")
    else:
        extra = ("Add" if tail == "residual" else "Mul", ["tok", "ytok"], ["tail"], {}, "tail")
    net.nodes[i:i + 1] = [extra, (op, ["tail"] + ins[1:], outs, at, nm)]
    assert inspect(nsg, net.data())["launches"] == plain + 1


# ---- the refusals ----------------------------------------------------------------------------------------------------
def rewired(nsg, kind):
    case = mm.MixCase(nsg, 27, D=337 if kind == "too_wide" else None if kind == "second_reader_of_x" else 20)
    net = case.net
    names = [n[4] for n in net.nodes]

    def at(name):
        return names.index(name)

    def feed(name, old, new):  # the node `name` reads `new` where it read `old`
        op, ins, outs, a, nm = net.nodes[at(name)]
        net.nodes[at(name)] = (op, [new if i == old else i for i in ins], outs, a, nm)

    if kind == "first_dimension":
        net.consts["w1"] = np.zeros((80, 20), np.float32)
    elif kind == "second_first_dimension":
        net.consts["w2"] = np.zeros((21, 81), np.float32)
    elif kind == "second_not_to_81":
        net.consts["w2"] = np.zeros((20, 80), np.float32)
    elif kind == "bias_along_c":
        net.consts["b1"] = np.ones((27, 1), np.float32)
    elif kind == "bias_at_run_time":  # the bias of the first stage is another [N,27,81] tensor (D = 81 here)
        net.consts["w1"] = np.zeros((81, 81), np.float32)
        net.consts["w2"] = np.zeros((81, 81), np.float32)
        net.consts["b2"] = np.zeros(81, np.float32)
        net.nodes.insert(at("mm1"), ("Reshape", ["s", net.const("again3", [-1, 27, 81], np.int64)], ["xr"], {}, "x_again"))
        names.insert(at("mm1"), "x_again")
        feed("bias1", "b1", "xr")
    elif kind == "leaky":
        net.nodes.insert(at("mm2"), ("LeakyRelu", ["biased1"], ["leaky"], {"alpha": 0.1}, "leaky"))
        names.insert(at("mm2"), "leaky")
        feed("mm2", "biased1", "leaky")
    elif kind == "second_consumer":
        net.nodes.insert(at("mm2"), ("Relu", ["biased1"], ["aside"], {}, "aside"))
    elif kind == "hidden_read_outside":
        net.nodes[at("mm2")] = ("Transpose", ["biased1"], ["mm2"], {"perm": [0, 2, 1]}, "mm2")
    elif kind == "third_matmul":
        net.nodes.insert(at("bias2") + 1, ("MatMul", ["biased2", net.const("w3", np.zeros((81, 81), np.float32))], ["mm3"], {}, "mm3"))
        names.insert(at("bias2") + 1, "mm3")
        feed("pflat", "biased2", "mm3")
    elif kind == "second_reader_of_x":
        net.nodes.insert(at("mm1") + 1, ("Transpose", ["x3"], ["xt_again"], {"perm": [0, 2, 1]}, "xt_again"))
    else:
        assert kind == "too_wide"
    return net.data()


REFUSALS = {
    "too_wide": ("mm1", "MatMul", ["[N,27,81]", "[81,337]", "D = 337", "1 to 336"]),
    "first_dimension": ("mm1", "MatMul", ["[N,27,81]", "[80,20]", "first dimension is 80", "last one is 81"]),
    "second_first_dimension": ("mm2", "MatMul", ["[N,27,20]", "[21,81]", "first dimension is 21", "last one is 20"]),
    "second_not_to_81": ("mm2", "MatMul", ["[N,27,20]", "[20,80]", "goes back to the 81 squares"]),
    "bias_along_c": ("bias1", "Add", ["[27,1]", "[N,27,20]", "varies along C"]),
    "bias_at_run_time": ("bias1", "Add", ["'xr'", "[N,27,81]", "computed at run time"]),
    "leaky": ("leaky", "LeakyRelu", ["[N,27,20]", "activation with a parameter"]),
    "second_consumer": ("bias1", "Add", ["'biased1'", "[N,27,20]", "2 consumers"]),
    "hidden_read_outside": ("mm2", "Transpose", ["'biased1'", "[N,27,20]", "D = 20, not 81", "second stage's nodes only"]),
    "third_matmul": ("mm3", "MatMul", ["[N,27,81]", "[81,81]", "third MatMul"]),
    "second_reader_of_x": ("mm1", "MatMul", ["'x3'", "[N,27,81]", "second consumer"]),
}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refusals_name_the_node_the_shapes_and_the_reason(nsg, kind):
    node, op, words = REFUSALS[kind]
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(rewired(nsg, kind), 86)
    msg = str(e.value)
    assert f"node '{node}' ({op})" in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_two_run_time_operands_keep_their_message(nsg):
    """[N,K,81] x [N,81,M], both computed at run time, is still the run-time product's refusal, in its words."""
    node, words = BMM_REFUSALS["transposed_first"]
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(bmm_rewired(nsg, "transposed_first"), 86)
    assert f"node '{node}' (MatMul)" in str(e.value)
    for w in words:
        assert w in str(e.value)


@pytest.mark.parametrize("name", ["one_c65_at4", "two_c27_d20_at2", "two_c80_d100"])
def test_truncated_models_are_errors_not_crashes(nsg, name):
    data = mm.case(nsg, name).data
    for cut in np.linspace(1, len(data) - 1, 20).astype(int):
        with pytest.raises(nsg.NsgError):
            nsg.inspect_onnx(data[:cut], 86)


# F = 32 channels.  conv launches: stem, policy, value, draw, and the block's channel Linears (mixer 2, resmlp 2, gmlp 2).
# The others: the mean, one token-mixing launch, the block's LayerNorms (mixer 2, gmlp 1), and the elementwise launches no
# epilogue takes: the residual behind the Transpose back (mixer), ResMLP's Affine in front and its LayerScale with the residual behind (resmlp), the gate (gmlp).
# A channel Linear's residual folds into its epilogue; the GELU behind a Linear folds too.
EXPORTS = {"mixer": (6, 1 + 1 + 2 + 1, 2 * 81 * 100 * 32 * 2), "resmlp": (6, 1 + 1 + 2, 2 * 81 * 81 * 32), "gmlp": (6, 1 + 1 + 1 + 1, 2 * 81 * 81 * 32)}


@pytest.mark.parametrize("opset", [13, 17])
@pytest.mark.parametrize("kind", list(EXPORTS))
def test_the_exported_modules_plan(nsg, tmp_path, kind, opset):
    data = mm.export(mm.torch_net(kind), tmp_path / "m.onnx", opset)
    info = inspect(nsg, data)
    convs, others, mix_flops = EXPORTS[kind]
    F = 32
    linear = {"mixer": 2 * 81 * F * 2 * F * 2, "resmlp": 2 * 81 * F * 2 * F * 2, "gmlp": 2 * 81 * F * 2 * F + 2 * 81 * F * F}[kind]
    assert info["conv_launches"] == convs, info
    assert info["launches"] - info["conv_launches"] - 2 == others, info  # (the plane expansion and the outputs are two)
    assert info["flops_per_position"] == 2 * 81 * 9 * 86 * F + 2 * 81 * F * mm.WIN + 2 * 2 * F + linear + mix_flops


# ---- the bounds ------------------------------------------------------------------------------------------------------
ALL = mm.all_parts(mm.CASES)


@pytest.mark.parametrize("name,part", ALL, ids=[f"{n}-{p}" for n, p in ALL])
def test_the_emulation_is_inside_the_bound(nsg, planes, name, part):
    case = mm.case(nsg, name, part)
    inp, ref, bound = case.expected(planes)
    assert np.isfinite(ref).all() and np.isfinite(bound).all()
    got = case.select(case.emulate(inp))
    if case.zero_bound():
        assert not bound.any()
        np.testing.assert_array_equal(got, ref.astype(np.float32))
        assert np.array_equal(ref, mm.em.f32(ref))
    r = ratio(got, ref, bound)
    print(name, part, "emulation error / bound", r, "largest bound", float(bound.max()), "largest |ref|", float(np.abs(ref).max()))
    assert r <= 1.0
    assert len(np.unique(ref)) > 50  # something to compare


@pytest.mark.parametrize("fault", list(mm.FAULTS))
def test_each_fault_falls_outside_the_bound(nsg, planes, fault):
    for name in mm.FAULTS[fault]:
        hit = False
        for part in mm.parts_of(name):
            case = mm.case(nsg, name, part)
            inp, ref, bound = case.expected(planes)
            assert ratio(case.select(case.emulate(inp)), ref, bound) <= 1.0
            got = case.select(case.emulate(inp, fault))
            hit = hit or (not np.isfinite(got).all()) or ratio(got, ref, bound) > 1.0
        assert hit, (fault, name)


def test_the_rounded_cases_are_rounded(nsg, planes):
    """On the fine stem the float32 result differs from the rounded float64 one: the bound is in use, not idle."""
    for name in mm.ROUNDED:
        case = mm.case(nsg, name)
        inp, ref, bound = case.expected(planes)
        got = case.select(case.emulate(inp))
        assert (got != ref.astype(np.float32)).mean() > 0.05, name
        assert float(bound.max()) > 0.0
