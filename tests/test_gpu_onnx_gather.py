"""Gather with constant indices and board flips on the device (graphGather, DESIGN.md sections 13.3, 13.4), on the
models of tests/gather_models.py.

A gather moves bits: every hand-built case equals the float64 reference, rounded to float32, bit for bit, at batches
of 1, 2 and 3.  A board's bits do not depend on its batch, with neighbours of 1e30.  Pad channels stay zero next to a
source that holds +inf in front of the view.  The exported torch module against float64 at the tolerance of
test_gpu_onnx_bmm.py, its opset 13 and 17 exports bit for bit."""
import numpy as np
import pytest

import gather_models as gm
from reduction_models import ratio
from test_gpu_onnx_bmm import run_batches
from test_gpu_onnx_elementwise import heads_close


@pytest.fixture(scope="module")
def boards(nsg):
    """Three of the seeded positions of the sibling files and their planes in float64."""
    bb = nsg.synth.random_batch(3, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def device(nsg, case, boards, tmp_path):
    bb, x = boards
    inp, ref, bound = case.expected(x)
    path = tmp_path / "m.onnx"
    path.write_bytes(case.data)
    info, outs = run_batches(nsg, path, bb)  # (asserts that a board's bits are the same at every batch)
    heads_close(outs, inp["env"])
    return outs[-1][1][0], ref, bound


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gm.CASES))
def test_a_gather_equals_float64_bit_for_bit(nsg, boards, tmp_path, name):
    case = gm.case(nsg, name)
    got, ref, bound = device(nsg, case, boards, tmp_path)
    assert not bound.any() and np.array_equal(ref, gm.em.f32(ref))
    assert len(np.unique(ref)) > 50  # something to compare
    np.testing.assert_array_equal(got, ref.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", gm.NEIGHBOURS)
def test_a_board_does_not_depend_on_its_neighbours(nsg, boards, tmp_path, name):
    """One board alone, and as the first, middle and last of three whose other two boards have a stem output of about
    +-1e30 (every plane that the stem reads set on every square, with the value 1e30): equal bits.  An element read from
    a neighbour's block would be 1e30."""
    bb, x = boards
    case = gm.case(nsg, name)
    huge = nsg.synth.pack(np.ones((1, 86, 81), bool), np.zeros((1, 86), bool), np.full((1, 86), 1e30, np.float32))
    hx = nsg.synth.expand_reference(huge, True).reshape(-1, 86, 9, 9).astype(np.float64)
    s = np.abs(case.net.known(hx)["s"])
    assert float(np.median(s)) > 1e29, float(np.median(s))
    path = tmp_path / "m.onnx"
    path.write_bytes(case.data)
    ev = nsg.Evaluator(0, 8, 86)
    ev.load(str(path))
    alone = ev.compute_blocking(bb[:1])[0][0].copy()
    assert np.isfinite(alone).all() and float(np.abs(alone).max()) < 1e6
    for place in range(3):
        batch = np.concatenate([huge] * place + [bb[:1]] + [huge] * (2 - place))
        with np.errstate(all="ignore"):
            got = ev.compute_blocking(batch)[0][place].copy()
        np.testing.assert_array_equal(got, alone, err_msg=f"{name}: the board at place {place} of three")
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gm.PADS))
def test_pad_channels_stay_zero(nsg, boards, tmp_path, name):
    """The gathered tensor's whole rows go through a 1x1 conv that selects 27 channels, and a Reciprocal: a pad channel
    that held the +inf in front of the view (or anything not finite) would make every output NaN; the real channels are
    held to the two divisions' 2.5 ulps."""
    case = gm.pad_case(nsg, name)
    got, ref, bound = device(nsg, case, boards, tmp_path)
    assert np.isfinite(got).all()
    r = ratio(got, ref, bound)
    print("gather pad", name, "error / bound", r)
    assert r <= 1.0, r


@pytest.mark.gpu
def test_the_two_heads_read_by_integer_index_match_their_slice_twin(nsg, boards, tmp_path):
    bb, x = boards
    outs = {}
    for how in ("gather", "slice"):
        path = tmp_path / f"{how}.onnx"
        path.write_bytes(gm.two_heads(nsg, how).data())
        outs[how] = run_batches(nsg, path, bb)[1][-1][1]
    for a, b in zip(outs["gather"], outs["slice"]):
        np.testing.assert_array_equal(a.reshape(-1), b.reshape(-1))
    assert len(np.unique(outs["gather"][1])) == 3 and not np.array_equal(outs["gather"][1], outs["gather"][2])


@pytest.mark.gpu
def test_the_exported_module_matches_float64_and_its_two_opsets_agree(nsg, tmp_path):
    import torch
    bb = nsg.synth.random_batch(19, 86, seed=31)
    x = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64))
    net = gm.gather_net()
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(x)]
    assert float(ref[0].std()) > 0.05, float(ref[0].std())  # logits that differ by far more than the tolerance
    net.float()
    outs = {}
    for opset in (13, 17):
        path = tmp_path / f"g{opset}.onnx"
        gm.export(net, path, opset)
        ev = nsg.Evaluator(0, 32, 86)
        ev.load(str(path))
        assert ev.graph_info()["path"] == "graph"
        outs[opset] = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in (1, 19)]
        ev.close()
        for n, o in outs[opset]:
            err = max(float(np.abs(np.asarray(a, np.float64).reshape(-1) - r[:n].reshape(-1)).max()) for a, r in zip(o, ref))
            print("gather net opset", opset, "batch", n, "max abs err", err)
            assert err < 1e-4, (opset, n, err)
    for (_, a), (_, b) in zip(outs[13], outs[17]):
        for p, q in zip(a, b):
            np.testing.assert_array_equal(p, q)
