"""The general graph path's dense conv, dense layer, depthwise and pooling kernels (graphConv<9>, graphConv<1>,
graphConvGeo, graphDepthwise, graphPool) on the device, almost directly: every model of tests/conv_models.py is an exact
stem, views of it, one launch of the kernel under test and a policy that does not round, so the kernel's output reaches
the test unmixed and its operands are known bit for bit.

Exact cases (integer weights, bias and residual; average pooling, whose one division is correctly rounded; max pooling)
equal the float64 reference bit for bit.  Rounded cases stay inside the any-order bound that conv_models derives from
the operands (its docstring and DESIGN.md 13.6.1; tests/test_conv_reference.py shows on the host that a float32
evaluation fits it, that each named fault does not, and that each model is one launch of the kernel it names).  A board
alone equals the same board in the larger batch bit for bit, value and draw are held to the siblings' 1e-4, and a board
between neighbours of about 1e30 keeps its bits.

Largest error / bound per rounded case, measured on an MI355X (a record, not an assertion; the bound is the worst case
over every order of summation):
#   graphConv<9>    r_t9_40x72_at27       0.010      graphConv<1>    r_t1_136x129_bare     0.031
#   graphConvGeo    r_g3x5d1x1            0.0032     graphConvGeo    r_g3x3d2x1_40x72_own  0.012
#   graphDepthwise  r_dw30_9x9d1x1_bare   0.044      graphDepthwise  r_dw65_3x5d1x1_at27   0.38
#   dense layer     r_d130                0.036
#   (largest bound per case 7e-5 .. 8e-4 on outputs of order 1; r_dw65_3x5d1x1_at27, 15 products: 9e-6, largest error
#   7.1e-7.  Every exact case -- 48 tile, 19 geo, 45 depthwise, 36 pooling, 4 dense -- passed on its first device run.)
"""
import numpy as np
import pytest

import conv_models as cm
from reduction_models import ratio
from test_gpu_onnx_elementwise import heads_close


def planes_of(nsg, bb):
    return nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


@pytest.fixture(scope="module")
def boards(nsg):
    """The 19 seeded positions of the sibling test files and their planes in float64."""
    bb = nsg.synth.random_batch(19, 86, seed=31)
    return bb, planes_of(nsg, bb)


@pytest.fixture(scope="module")
def dense_boards(nsg):
    """163 seeded positions: two groups of 81 dense rows and one row of a third."""
    bb = nsg.synth.random_batch(163, 86, seed=31)
    return bb, planes_of(nsg, bb)


@pytest.fixture(scope="module")
def huge(nsg):
    """A board with every plane set on every square, with the value 1e30."""
    return nsg.synth.pack(np.ones((1, 86, 81), bool), np.zeros((1, 86), bool), np.full((1, 86), 1e30, np.float32))


def device(nsg, data, bb, tmp_path, batches, size=32):
    path = tmp_path / "m.onnx"
    path.write_bytes(data)
    ev = nsg.Evaluator(0, size, 86)
    ev.load(str(path))
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    ev.close()
    return outs


def check(nsg, name, boards, tmp_path, batches, size=32):
    """Every window of the case at every batch: a board's bits do not depend on its batch, the heads are within 1e-4, an
    exact case equals float64 bit for bit; returns the largest error / bound of a rounded one."""
    bb, x = boards
    case = cm.case(nsg, name)
    inp = case.inputs(x[:batches[-1]])  # (an exact case asserts here that every partial sum is exact in float32)
    ref, bound = case.ref(inp), case.bound(inp)
    case.every_channel_shows(ref)
    worst = 0.0
    for part in case.parts:
        outs = device(nsg, case.model(part), bb, tmp_path, batches, size)
        whole = outs[-1][1]
        for n, o in outs[:-1]:
            for a, b in zip(o, whole):
                np.testing.assert_array_equal(a, b[:n], err_msg=f"{name}: batch {n} against batch {batches[-1]}")
        heads_close(outs, inp["env"])
        got, want, bnd = whole[0], case.select(ref, part), case.select(bound, part)
        assert np.isfinite(got).all()
        if case.exact:
            assert not bnd.any() and np.array_equal(want, cm.em.f32(want))
            np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=f"{name}: window {part}")
        else:
            r = ratio(got, want, bnd)
            print(name, part, "error / bound", r, "largest bound", float(bnd.max()), "largest error", float(np.abs(got - want).max()))
            worst = max(worst, r)
    return worst


def batches_of(name):
    return (1, 3) if name in cm.INDEXING else (1, 19)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cm.TILE))
def test_tile_conv_exact(nsg, boards, tmp_path, name):
    """graphConv<9> and graphConv<1>: cin 4 (a quarter of a chunk), 17 (a chunk with one real channel), 136; cout 65 (a
    second tile with one real channel: three of its waves leave), 72, 129 (three tiles); bare, and with a fused residual
    and ReLU read from a tensor of the conv's width and from Split views at channels 27 and 16 of a wider one."""
    check(nsg, name, boards, tmp_path, batches_of(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cm.GEO))
def test_geo_conv_exact(nsg, boards, tmp_path, name):
    """graphConvGeo on rectangular kernels with both sides above 1 and on dh != dw: 15 taps (8 + 7, a group boundary
    inside a kernel row), 21, 27, 35, 45 and 63 (eight full groups), straight from the 86 planes, and two geometries
    again at 40 -> 72 channels with a residual and ReLU."""
    check(nsg, name, boards, tmp_path, batches_of(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cm.DW))
def test_depthwise_exact(nsg, boards, tmp_path, name):
    """graphDepthwise at C = 27, 30 and 65 (C % 4 != 0: the c0 + j < C paths), 81 taps (sW filled exactly), rectangular
    and unevenly dilated kernels; the residual through the float4 branch (a view at channel 16) and the scalar one (27)."""
    check(nsg, name, boards, tmp_path, batches_of(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cm.POOL))
def test_pooling_exact(nsg, boards, tmp_path, name):
    """graphPool: both averages are the exact window sum and ONE correctly rounded division, bit for bit; the max is the
    exact max.  On 18 channels at channel 6 of the stem's rows (scalar and float4 pieces, a ragged end) and on 64."""
    check(nsg, name, boards, tmp_path, batches_of(name))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cm.ROUNDED))
def test_rounded_convs_stay_inside_the_bound(nsg, boards, tmp_path, name):
    worst = check(nsg, name, boards, tmp_path, batches_of(name))
    print(name, "error / bound", worst)
    assert worst <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cm.DENSE))
def test_dense_layer_in_groups_of_81_rows(nsg, dense_boards, tmp_path, name):
    """K -> 2187 (35 output tiles, the last with 11 channels) at batches 1, 80, 81, 82 and 163: rows 81..95 of a group
    repeat row 80 and rows at or past the batch are skipped."""
    worst = check(nsg, name, dense_boards, tmp_path, cm.DENSE_BATCHES, size=163)
    if not cm.DENSE[name].get("exact", True):
        print(name, "error / bound", worst)
        assert worst <= 1.0, worst


ISOLATED = ["t9_24x65_at27", "t1_17x27_own", "g5x9d1x1", "g3x5d1x1_40x72_own", "dw65_9x9d1x1_at27", "dw30_3x3d4x1_at16",
            "p_avg_exclude_9x9d1x1_view18", "p_max_3x3d4x1_w64", "r_t9_40x72_at27"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ISOLATED)
def test_a_board_does_not_depend_on_its_neighbours(nsg, boards, huge, tmp_path, name):
    """One board alone, and as the first, middle and last of three whose other two boards feed the kernel values of
    about +-1e30: equal bits.  A square, a halo or a residual read from a neighbour would be 1e30 or, summed, inf."""
    bb, x = boards
    case = cm.case(nsg, name)
    hx = planes_of(nsg, huge)
    s = np.abs(hx[:, :82] if getattr(case, "planes", False) else case.net.known(hx)["s"])  # what the kernel reads there
    assert float(np.median(s)) > 1e29, float(np.median(s))
    path = tmp_path / "m.onnx"
    path.write_bytes(case.model(case.parts[-1]))
    ev = nsg.Evaluator(0, 8, 86)
    ev.load(str(path))
    alone = ev.compute_blocking(bb[:1])[0][0].copy()
    assert np.isfinite(alone).all() and len(np.unique(alone)) > 5
    for place in range(3):
        batch = np.concatenate([huge] * place + [bb[:1]] + [huge] * (2 - place))
        with np.errstate(all="ignore"):
            got = ev.compute_blocking(batch)[0][place].copy()
        np.testing.assert_array_equal(got, alone, err_msg=f"{name}: the board at place {place} of three")
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["d130", "d64_h65"])
def test_a_dense_row_does_not_depend_on_its_neighbours(nsg, boards, huge, tmp_path, name):
    """A real board at row 80, 81 or 82 of a batch of 163 whose other rows are the board of 1e30: the bits of the board
    alone.  Row 80 is the row that the pad rows of its group repeat, 81 and 82 open the next group."""
    bb, x = boards
    case = cm.case(nsg, name)
    s = np.abs(case.net.known(planes_of(nsg, huge))["s"])
    assert float(np.median(s)) > 1e29, float(np.median(s))
    path = tmp_path / "m.onnx"
    path.write_bytes(case.model())
    ev = nsg.Evaluator(0, 163, 86)
    ev.load(str(path))
    alone = ev.compute_blocking(bb[:1])[0][0].copy()
    assert np.isfinite(alone).all() and len(np.unique(alone)) > 50
    for row in (80, 81, 82):
        batch = np.concatenate([huge] * row + [bb[:1]] + [huge] * (162 - row))
        with np.errstate(all="ignore"):
            got = ev.compute_blocking(batch)[0][row].copy()
        np.testing.assert_array_equal(got, alone, err_msg=f"{name}: the board at row {row} of 163")
    ev.close()
