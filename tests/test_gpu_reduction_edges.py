"""The general graph path's reduction kernels (graphAttention, graphLayerNorm, graphRmsNorm, graphGroupNorm) on the
device, almost directly: every model of tests/reduction_models.py is an exact stem, views of it, one launch of the
kernel under test and a policy that selects 27 of its output channels with 0/1 weights, so the kernel's output reaches
the test unmixed and its inputs are known bit for bit.

Each element is compared with the float64 definition against the bound that reduction_models derives from the same
inputs (its docstring and DESIGN.md 13.6 hold the derivation; tests/test_reduction_reference.py shows on the host that a
float32 evaluation fits the bound and that the listed faults do not).  Where the result is known exactly -- a query row
with one open key, a constant LayerNorm row or GroupNorm group -- bits are asserted.  Batches 1 and 19 must agree bit
for bit, and value and draw are held to the siblings' 1e-4.

The pad channels behind H d (d = 12: 24 of 32, d = 20 and 40: 40 of 48) cannot be selected: the planner gives a consumer
the launch's C = H d channels and nothing else.  The selection's launch does read whole 16-channel chunks against
zero weights, so a pad that held a NaN or an infinity would turn the policy into NaN, which the tests would see; a
finite non-zero pad would not show.

Stems are 64 channels wide or narrower wherever the case allows; a normalisation over 65, 72, 136 or 200 channels
needs that many (plus the Split offset).

Largest error / bound, measured on an MI355X (a record, not an assertion; the bounds are worst cases over every order
of summation, the kernels' butterflies and MFMA chains err far less):
#   attention   d4 0.049  d12 0.043  d20 0.038  d24 0.034  d40 0.023  d48 0.022  d16 0.057  d64_same_view 0.059
#               big_scores 0.032  masked_inf 0.043  masked_1e9 0.043  views 0.048
#   C =                        4      24     64     65     72     136
#   layernorm token centred    0.186  0.102  0.040  0.042  0.051  0.023
#   layernorm token offset     0      0.027  0      0.015  0.012  0.007
#   layernorm flat  centred    0.113  0.068  0.024  0.029  0.031  0.016
#   layernorm flat  offset     0      0.026  0      0.015  0.012  0.007
#   rmsnorm   token centred    0.399  0.178  0.089  0.087  0.081  0.047
#   rmsnorm   token offset     0.439  0.209  0.097  0.108  0.093  0.055
#   rmsnorm   token const 1e-5 0.322  0.129  0.067  0.062  0.060  0.034
#   rmsnorm   flat  centred    0.242  0.158  0.063  0.074  0.061  0.036
#   rmsnorm   flat  offset     0.279  0.154  0.087  0.094  0.076  0.039
#   rmsnorm   flat  const 1e-5 0.322  0.129  0.067  0.040  0.060  0.034
#   (constant LayerNorm rows: beta bit for bit; constant RMSNorm rows at eps = 1e-12: error 0)
#   groupnorm   24x3 0.0032  24x24 0.024  24x1 0.0003  27x3 0.0028  72x8 0.0033  200x1 0.00005  24x3_at6 0.0025
#               24x3_const_eps5 0.0023  24x3_const_eps12 0.0028  72x8_const_eps12 0.0034  24x3_centred 0.0033
"""
import numpy as np
import pytest

import reduction_models as rm
from test_gpu_onnx_elementwise import device, heads_close
from reduction_models import ATT, GN, ROWS, exact_where_unbounded, ratio


@pytest.fixture(scope="module")
def boards(nsg):
    """The 19 seeded positions of the sibling test files and their planes in float64."""
    bb = nsg.synth.random_batch(19, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def run(nsg, case, boards, tmp_path):
    """Loads the case, runs batches 1 and 19 and returns the policy of the 19 with the reference and the bound.  The
    board of the batch of one equals its row in the batch of 19 bit for bit, and the heads are within 1e-4."""
    bb, x = boards
    inp, ref, bound = case.expected(x)
    info, outs = device(nsg, case.data, bb, tmp_path)
    (_, one), (_, whole) = outs
    for a, b in zip(one, whole):
        np.testing.assert_array_equal(a[0], b[0])
    heads_close(outs, inp["env"])
    return info, inp, whole[0], ref, bound


@pytest.mark.gpu
@pytest.mark.parametrize("name,start", ATT, ids=[f"{n}-{s}" for n, s in ATT])
def test_attention(nsg, boards, tmp_path, name, start):
    """d4 .. d64: every head width and all four graphAttention<D16> instantiations (d40 and d48: <3>), a bias on
    every one; d4, d16 and d64 have exact scores (no score term in the bound), d64 reads q, k and v from one view.
    big_scores: exact scores beyond +-100 on every board (inf / inf without the max subtraction).  masked_inf,
    masked_1e9: a causal-like bias of -inf and of -1e9, rows with one open key equal that key's V row bit for bit.
    views: v, q, k at channels 4, 24, 44 of the 64-wide row."""
    case = rm.att_case(nsg, name, start)
    info, inp, got, ref, bound = run(nsg, case, boards, tmp_path)
    assert info["attention_launches"] == 1 and info["flops_per_position"] == 2 * 81 * 9 * 86 * 64 + 2 * 81 * case.F * rm.WIN + 2 * 2 * 64 + 4 * 81 * 81 * case.H * case.d
    assert np.isfinite(got).all()
    if case.bias_kind in ("causal_inf", "causal_1e9"):
        one, key = case.single_rows()
        vk = inp["v"].reshape(len(got), 81, case.F)[:, :, case.ch]
        exp = vk[:, key.reshape(rm.WIN, 81), np.arange(rm.WIN)[:, None]].reshape(len(got), -1)
        np.testing.assert_array_equal(got[:, one], exp[:, one].astype(np.float32))
    r = ratio(got, ref, bound)
    print("attention", name, start, "error / bound", r, "largest bound", float(bound.max()))
    assert r <= 1.0, r


@pytest.mark.gpu
@pytest.mark.parametrize("op,domain,C,variant", ROWS, ids=["-".join(map(str, r)) for r in ROWS])
def test_layernorm_and_rmsnorm(nsg, boards, tmp_path, op, domain, C, variant):
    """C = 4 .. 136 read at channel 3 of the stem's rows (token rows, or the flat global max).  centred: eps = 1e-2,
    which tells eps inside the square root from eps outside; offset: every channel + 512, |mean| / sigma >= 2^9
    (asserted), which tells the two-pass variance from E[x^2] - mean^2; constant rows with eps = 1e-5 and 1e-12: a
    LayerNorm row is beta bit for bit (it catches none of the listed faults: x - mean is exactly 0 whatever the
    statistics, which is the property asserted), an RMSNorm row is within the bound, a few ulps, of float64 (with
    eps = 1e-12, below half an ulp of every mean square on the grid, it tells no listed fault apart either: it shows
    that inv stays finite and the row exact to the bound when eps vanishes)."""
    worst = 0.0
    for start in (rm.starts(C) if domain == "token" else [0]):
        case = rm.row_case(nsg, op, domain, C, variant, start)
        info, inp, got, ref, bound = run(nsg, case, boards, tmp_path)
        assert np.isfinite(got).all()
        exact_where_unbounded(case, got, ref, bound)
        if variant.startswith("constant") and op == "layernorm":
            np.testing.assert_array_equal(got, case.select(np.broadcast_to(case.b, case.ref(inp).shape)).astype(np.float32))
        worst = max(worst, ratio(got, ref, bound))
    print(op, domain, C, variant, "error / bound", worst)
    assert worst <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,start", GN, ids=[f"{n}-{s}" for n, s in GN])
def test_groupnorm(nsg, boards, tmp_path, name, start):
    """(24,3): one slab; (24,24): an instance norm; (24,1): the block team; (27,3): odd widths, policy = Flatten;
    (72,8): two workgroups per board; (200,1): the unstaged path; 24x3_at6: read at channel 6 of the stem.  The odd
    groups (the one group where G = 1) are offset by 512, so a statistic that leaked from a neighbour would show; the
    one group of 200 channels by 64, the largest power of two at which the any-order bound of a mean over 16200
    elements leaves a bound on y on every board (reduction_models.GroupNormCase); E[x^2] - mean^2 falls outside it.
    On the shifted groups the bound is 0.3 to 1.4 on outputs of order 1, a check against gross faults; the unshifted
    groups carry the precision.  The constant group gives act(beta) bit for bit at eps = 1e-5 and 1e-12."""
    case = rm.gn_case(nsg, name, start)
    info, inp, got, ref, bound = run(nsg, case, boards, tmp_path)
    assert np.isfinite(got).all()
    exact_where_unbounded(case, got, ref, bound)
    if case.constant is not None:
        m, want = case.constant_mask()
        np.testing.assert_array_equal(got[:, m], np.broadcast_to(want[m].astype(np.float32), got[:, m].shape))
    r = ratio(got, ref, bound)
    print("groupnorm", name, start, "error / bound", r)
    assert r <= 1.0, r
