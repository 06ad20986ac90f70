"""The references, bounds and models of tests/reduction_models.py, checked on the host: no device needed.

  1. On every case of tests/test_gpu_reduction_edges.py the float32 numpy emulation of the definition lies within the
     derived bound of float64 (and equals it where the case asserts bits): the inputs and the bound are satisfiable.
  2. With one fault injected, the same emulation lies outside the bound, or is non-finite, on the case built for that
     fault: the bound is tight enough to see a kernel that is wrong in that way.
  3. Every model plans on the general graph path with exactly one attention or normalisation launch, and the plan's
     head width is the model's as far as the plan shows it: nsg_inspect_onnx reports the attention FLOPs,
     4 * 81 * 81 * H * d, and for H >= 2 the planner accepts a bias of [H,81,81] for H heads only, so F = H d and H
     together give d.  A bias of [1,81,81] is accepted for any head count, so for H = 1 (d = 40, 48, 64) the refusal
     of [2,81,81] excludes two heads only and d is otherwise inferred from H d; a wrong split (F = 40 run as two
     heads of 20, say) is what the device test's numerics catch."""
import numpy as np
import pytest

import reduction_models as rm


@pytest.fixture(scope="module")
def planes(nsg):
    """The 19 seeded positions of the sibling files, as float64 planes."""
    bb = nsg.synth.random_batch(19, 86, seed=31)
    return nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


ATT, ROWS, GN, ratio, exact_where_unbounded = rm.ATT, rm.ROWS, rm.GN, rm.ratio, rm.exact_where_unbounded


@pytest.mark.parametrize("name,start", ATT, ids=[f"{n}-{s}" for n, s in ATT])
def test_attention_emulation_is_inside_the_bound(nsg, planes, name, start):
    case = rm.att_case(nsg, name, start)
    inp, ref, bound = case.expected(planes)
    assert np.isfinite(ref).all() and np.isfinite(bound).all()
    got = case.select(case.emulate(inp))
    r = ratio(got, ref, bound)
    print(name, start, "emulation error / bound", r, "largest bound", float(bound.max()))
    assert r <= 1.0
    s = case.scores(inp["q"], inp["k"])
    fin = np.where(np.isfinite(s) & (s > -1e8), s, np.nan)
    if name == "big_scores":  # every board has rows whose largest score exceeds 100, and scores of both signs
        top = np.nanmax(fin, axis=-1)
        assert (top.reshape(len(planes), -1).max(axis=1) > 100).all() and (np.nanmin(fin.reshape(len(planes), -1), axis=1) < -100).all()
    elif case.bias_kind == "grid":  # neither uniform nor one-hot: a softmax that ignored the scores would show
        sd = float(np.nanstd(fin - np.nanmean(fin, axis=-1, keepdims=True)))
        assert 0.5 < sd < 8.0, sd
    if case.bias_kind in ("causal_inf", "causal_1e9"):
        opened = rm.open_keys(case.bias)
        assert opened.min() == 1 and (opened == 1).sum() >= 9 * case.H and opened.max() > 40
        one, key = case.single_rows()
        assert one.any()
        # the reference of a row with one open key is that key's V row
        vk = inp["v"].reshape(len(planes), 81, case.F)[:, :, case.ch]  # [N,81,27]
        exp = vk[:, key.reshape(rm.WIN, 81), np.arange(rm.WIN)[:, None]].reshape(len(planes), -1)
        np.testing.assert_array_equal(ref[:, one], exp[:, one])
        np.testing.assert_array_equal(got[:, one], exp[:, one].astype(np.float32))


@pytest.mark.parametrize("op,domain,C,variant", ROWS, ids=["-".join(map(str, r)) for r in ROWS])
def test_row_norm_emulation_is_inside_the_bound(nsg, planes, op, domain, C, variant):
    for start in (rm.starts(C) if domain == "token" else [0]):
        case = rm.row_case(nsg, op, domain, C, variant, start)
        inp, ref, bound = case.expected(planes)
        got = case.select(case.emulate(inp))
        assert np.isfinite(got).all() and np.isfinite(ref).all()
        exact_where_unbounded(case, got, ref, bound)
        if variant.startswith("constant") and op == "layernorm":
            assert not np.isfinite(bound).any() or np.array_equal(ref[np.isfinite(bound)], case.select(np.broadcast_to(case.b, case.ref(inp).shape))[np.isfinite(bound)])
            np.testing.assert_array_equal(got, case.select(np.broadcast_to(case.b, case.ref(inp).shape)).astype(np.float32))
        r = ratio(got, ref, bound)
        print(op, domain, C, variant, start, "emulation error / bound", r)
        assert r <= 1.0


@pytest.mark.parametrize("name,start", GN, ids=[f"{n}-{s}" for n, s in GN])
def test_groupnorm_emulation_is_inside_the_bound(nsg, planes, name, start):
    case = rm.gn_case(nsg, name, start)
    inp, ref, bound = case.expected(planes)
    got = case.select(case.emulate(inp))
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    exact_where_unbounded(case, got, ref, bound)
    if case.constant is not None:
        m, want = case.constant_mask()
        np.testing.assert_array_equal(ref[:, m], np.broadcast_to(want[m], ref[:, m].shape))
        np.testing.assert_array_equal(got[:, m], np.broadcast_to(want[m].astype(np.float32), got[:, m].shape))
        assert np.isfinite(bound[:, ~m]).all()
    else:
        assert np.isfinite(bound).all()
    r = ratio(got, ref, bound)
    print(name, start, "emulation error / bound", r, "largest bound", float(bound[np.isfinite(bound)].max()))
    assert r <= 1.0


def caught(case, planes, fault):
    inp, ref, bound = case.expected(planes)
    got = case.select(case.emulate(inp, fault))
    return (not np.isfinite(got).all()) or ratio(got, ref, bound) > 1.0


@pytest.mark.parametrize("fault", list(rm.ATT_FAULTS))
def test_attention_faults_fall_outside_the_bound(nsg, planes, fault):
    case = rm.att_case(nsg, rm.ATT_FAULTS[fault])
    assert caught(case, planes, fault), fault
    assert not caught(case, planes, None)


# fault -> the row-norm and GroupNorm cases built for it
NORM_FAULT_CASES = {
    "one_pass_variance": [("layernorm", "token", 24, "offset"), ("layernorm", "flat", 136, "offset"), "24x3", "72x8", "24x24", "24x1", "200x1"],
    "unbiased_variance": [("layernorm", "token", 136, "centred"), ("layernorm", "flat", 4, "centred"), "72x8", "24x3_centred"],
    "neighbour_group": ["24x3", "24x24", "27x3", "72x8", "24x3_at6"],
    "eps_outside_sqrt": [("layernorm", "token", 24, "centred"), ("rmsnorm", "token", 24, "centred"), ("rmsnorm", "flat", 65, "constant_eps5"),
                         "24x3_centred"],
}


@pytest.mark.parametrize("fault", rm.NORM_FAULTS)
def test_norm_faults_fall_outside_the_bound(nsg, planes, fault):
    assert sorted(NORM_FAULT_CASES) == sorted(rm.NORM_FAULTS)
    for c in NORM_FAULT_CASES[fault]:
        case = rm.gn_case(nsg, c) if isinstance(c, str) else rm.row_case(nsg, *c)
        assert caught(case, planes, fault), (fault, c)


def test_the_wide_group_takes_the_largest_offset_that_leaves_a_bound(nsg, planes):
    """(200,1) at the issue's offset of 512, and at 128, has elements without a bound (the any-order error of a mean
    over 16200 elements exceeds sigma / 2); at 64, the offset the case uses, every element has one."""
    assert rm.GN_SHAPES["200x1"] == dict(C=200, G=1, relu=True, shift=64.0)
    for shift, finite in ((512.0, False), (128.0, False), (64.0, True)):
        case = rm.GroupNormCase(nsg, 200, 1, relu=True, shift=shift)
        assert bool(np.isfinite(case.expected(planes)[2]).all()) == finite, shift


def test_every_device_case_catches_a_fault_or_says_why(nsg, planes):
    """The cases that catch no listed fault are the constant LayerNorm rows (their output is beta whatever the
    statistics are: x - mean is exactly 0, which is the property they assert) and the RMSNorm rows where eps vanishes
    against the mean square (offset by 512, or eps = 1e-12).  Every other case catches at least one."""
    for name in rm.ATT_SHAPES:
        case = rm.att_case(nsg, name)
        faults = [f for f in rm.ATT_FAULTS if not (f == "bias_transposed" and case.bias is None)]
        assert any(caught(case, planes, f) for f in faults), name
    for op, dom, C, v in ROWS:
        if op == "layernorm" and v.startswith("constant"):
            continue
        faults = ["eps_outside_sqrt"] if op == "rmsnorm" else ["one_pass_variance", "unbiased_variance", "eps_outside_sqrt"]
        if op == "rmsnorm" and v in ("constant_eps12", "offset"):
            continue  # of the listed faults only the place of eps bears on RMSNorm, and eps vanishes here: see the device test
        assert any(caught(rm.row_case(nsg, op, dom, C, v), planes, f) for f in faults), (op, dom, C, v)
    for name in rm.GN_SHAPES:
        assert any(caught(rm.gn_case(nsg, name), planes, f) for f in rm.NORM_FAULTS), name


# ---- the plans -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,start", ATT, ids=[f"{n}-{s}" for n, s in ATT])
def test_attention_models_plan_with_one_launch_and_their_head_width(nsg, name, start):
    case = rm.att_case(nsg, name, start)
    info = nsg.inspect_onnx(case.data, 86)
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 1
    # stem, attention, selection, mean, value, draw; planes and outputs
    assert info["conv_launches"] == 4 and info["launches"] == 6 + 2
    stem = 2 * 81 * 9 * 86 * 64 + 2 * 81 * case.F * rm.WIN + 2 * 2 * 64
    assert info["flops_per_position"] == stem + 4 * 81 * 81 * case.H * case.d
    assert case.bias is not None and case.bias.shape == (case.H, 81, 81) and case.H * case.d == case.F
    # a bias for another head count is refused: the plan's H is the model's, and with F = H d so is its d
    other = rm.AttCase(nsg, case.F, case.H, start=start)
    other.net.consts["rel"] = np.zeros((case.H + 1, 81, 81), np.float32)
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(other.net.data(), 86)
    assert "attention bias of shape" in str(e.value)


def test_a_head_width_outside_the_kernel_is_refused(nsg):
    case = rm.AttCase(nsg, 60, 10)  # d = 6
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(case.data, 86)
    assert "head dimension 6" in str(e.value)


@pytest.mark.parametrize("op,domain,C,variant", ROWS, ids=["-".join(map(str, r)) for r in ROWS])
def test_row_norm_models_plan_with_one_launch(nsg, op, domain, C, variant):
    case = rm.row_case(nsg, op, domain, C, variant)
    info = nsg.inspect_onnx(case.data, 86)
    assert info["path"] == "graph" and info["attention_launches"] == 0
    # stem, [global max,] the normalisation, selection, mean, value, draw; planes and outputs
    assert info["conv_launches"] == 4 and info["launches"] == (7 if domain == "flat" else 6) + 2


@pytest.mark.parametrize("name,start", GN, ids=[f"{n}-{s}" for n, s in GN])
def test_groupnorm_models_plan_with_one_launch(nsg, name, start):
    case = rm.gn_case(nsg, name, start)
    info = nsg.inspect_onnx(case.data, 86)
    assert info["path"] == "graph" and info["attention_launches"] == 0
    # stem, GroupNorm (gamma, beta and the ReLU ride in it), [selection,] mean, value, draw; planes and outputs
    flat = case.C == rm.WIN
    assert info["conv_launches"] == (3 if flat else 4) and info["launches"] == (5 if flat else 6) + 2
