"""Token-mixing MLPs on the device (graphTokenMix, DESIGN.md sections 13.3, 13.4), on the models of tests/mix_models.py.

Exact cases: the device gives the float64 result bit for bit, at batches of 1, 2 and 3.  Rounded cases: inside the bound
derived in mix_models from the operands.  A board's bits do not depend on its batch, with neighbours of 1e30.  Pad
channels and hidden pad units behind Exp, Reciprocal and Sqrt, the whole rows read by a selecting conv.  The exported
Mixer, ResMLP and gMLP modules against float64 at the sibling tests' 1e-4, their opset 13 and 17 exports bit for bit.
Figures, where a case is not exact, are printed before they are asserted."""
import numpy as np
import pytest

import mix_models as mm
from reduction_models import ratio
from test_gpu_onnx_elementwise import heads_close


@pytest.fixture(scope="module")
def boards(nsg):
    """Three of the seeded positions of the sibling files and their planes in float64."""
    bb = nsg.synth.random_batch(3, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def run_batches(nsg, path, bb, batches=(1, 2, 3)):
    ev = nsg.Evaluator(0, 8, 86)
    ev.load(str(path))
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] == 0
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    ev.close()
    whole = outs[-1][1]
    for n, o in outs[:-1]:  # a board does not depend on its batch
        for a, b in zip(o, whole):
            np.testing.assert_array_equal(a, b[:n])
    return info, outs


def device(nsg, case, boards, tmp_path):
    bb, x = boards
    inp, ref, bound = case.expected(x)
    path = tmp_path / "m.onnx"
    path.write_bytes(case.data)
    info, outs = run_batches(nsg, path, bb)
    heads_close(outs, inp["env"])
    return outs[-1][1][0], ref, bound


EXACT = mm.all_parts(mm.EXACT)
ROUNDED = mm.all_parts(mm.ROUNDED)
PADS = mm.all_parts(mm.PADS)


@pytest.mark.gpu
@pytest.mark.parametrize("name,part", EXACT, ids=[f"{n}-{p}" for n, p in EXACT])
def test_exact_cases_equal_float64_bit_for_bit(nsg, boards, tmp_path, name, part):
    case = mm.case(nsg, name, part)
    assert case.zero_bound()
    got, ref, bound = device(nsg, case, boards, tmp_path)  # (inputs asserts that every partial sum is exact in float32)
    assert not bound.any() and np.array_equal(ref, mm.em.f32(ref))
    assert len(np.unique(ref)) > 50  # something to compare
    np.testing.assert_array_equal(got, ref.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("name,part", ROUNDED, ids=[f"{n}-{p}" for n, p in ROUNDED])
def test_rounded_cases_stay_inside_the_bound(nsg, boards, tmp_path, name, part):
    case = mm.case(nsg, name, part)
    got, ref, bound = device(nsg, case, boards, tmp_path)
    assert np.isfinite(got).all()
    r = ratio(got, ref, bound)
    print("tokenmix", name, part, "error / bound", r, "largest bound", float(bound.max()), "largest error", float(np.abs(got - ref).max()))
    assert r <= 1.0, r


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_c24_relu", "one_c65_at4", "two_c64_d20_at4", "two_c27_d20_at2", "r_two_c27_d100_gelu"])
def test_a_board_does_not_depend_on_its_neighbours(nsg, boards, tmp_path, name):
    """One board alone, and as the first, middle and last of three whose other two boards have a stem output of about
    +-1e30 (every plane that the stem reads set on every square, with the value 1e30): equal bits.  A row read from a
    neighbour would be 1e30 or, multiplied, inf."""
    bb, x = boards
    case = mm.case(nsg, name)
    huge = nsg.synth.pack(np.ones((1, 86, 81), bool), np.zeros((1, 86), bool), np.full((1, 86), 1e30, np.float32))
    hx = nsg.synth.expand_reference(huge, True).reshape(-1, 86, 9, 9).astype(np.float64)
    s = np.abs(case.net.known(hx)["s"])
    assert float(np.median(s)) > 1e29, float(np.median(s))
    path = tmp_path / "m.onnx"
    path.write_bytes(case.data)
    ev = nsg.Evaluator(0, 8, 86)
    ev.load(str(path))
    alone = ev.compute_blocking(bb[:1])[0][0].copy()
    assert np.isfinite(alone).all()
    for place in range(3):
        batch = np.concatenate([huge] * place + [bb[:1]] + [huge] * (2 - place))
        with np.errstate(all="ignore"):
            got = ev.compute_blocking(batch)[0][place].copy()
        np.testing.assert_array_equal(got, alone, err_msg=f"{name}: the board at place {place} of three")
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,part", PADS, ids=[f"{n}-{p}" for n, p in PADS])
def test_pads_stay_zero_behind_exp_reciprocal_and_sqrt(nsg, boards, tmp_path, name, part):
    """The result's whole rows go through a 1x1 conv that selects 27 channels: 1 / 0 = inf in a pad channel or a hidden
    pad unit, or the square root of a pad that received a negative bias, times a zero weight would be NaN in every
    output; the real channels are held to expf's 2 ulps and the half ulp of the division and the square root."""
    case = mm.case(nsg, name, part)
    got, ref, bound = device(nsg, case, boards, tmp_path)
    assert np.isfinite(got).all()
    r = ratio(got, ref, bound)
    print("tokenmix pad", name, part, "error / bound", r)
    assert r <= 1.0, r


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mixer", "resmlp", "gmlp"])
def test_the_exported_modules_match_float64_and_their_two_opsets_agree(nsg, tmp_path, kind):
    import torch
    bb = nsg.synth.random_batch(19, 86, seed=31)
    x = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64))
    net = mm.torch_net(kind)
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(x)]
    assert float(ref[0].std()) > 0.05, float(ref[0].std())  # logits that differ by far more than the tolerance
    net.float()
    outs = {}
    for opset in (13, 17):
        path = tmp_path / f"{kind}{opset}.onnx"
        mm.export(net, path, opset)
        ev = nsg.Evaluator(0, 32, 86)
        ev.load(str(path))
        assert ev.graph_info()["path"] == "graph"
        outs[opset] = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in (1, 19)]
        ev.close()
        for n, o in outs[opset]:
            err = max(float(np.abs(np.asarray(a, np.float64).reshape(-1) - r[:n].reshape(-1)).max()) for a, r in zip(o, ref))
            print(kind, "opset", opset, "batch", n, "max abs err", err)
            assert err < 1e-4, (opset, n, err)
    for (_, a), (_, b) in zip(outs[13], outs[17]):
        for p, q in zip(a, b):
            np.testing.assert_array_equal(p, q)
