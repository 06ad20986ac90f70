"""One-channel maps on the device: the reduction over the channels of a row (graphChanReduce) and the broadcast of a
one-channel tensor inside the elementwise launch (kSrcRowOne, kSrcBoardOne, kSrcSquare), almost directly.  Every model
of tests/gate_models.py is an exact stem, views of it, the ops under test and a policy that shows 27 channels through
nothing that rounds, so what the kernels write reaches the test unmixed and their inputs are known bit for bit.

Max, min, sums on the coarse grid (every partial sum an integer below 2^24 quanta, asserted on the float64 side) and every
broadcast of an exact gate equal float64 bit for bit.  Sums on the 2^-11 grid with offsets up to 2^12 are held to
gamma(C) sum|x| (the mean: over C, plus one u |mean| for its factor), the ratio printed before it is asserted.  Batches 1, 2 and 3
agree bit for bit board by board, also between neighbours at 1e30.  tests/test_onnx_gate.py shows on the host that a
float32 evaluation fits these bounds and that the listed faults do not.

Largest error / bound of the rounding sums, measured on an MI355X (a record, not an assertion): 0 at C <= 4, 0.02 to 0.1
at C = 16 .. 27, below 0.01 at C = 64 and 100, sums and means alike; the butterfly errs far less than the any-order bound."""
import numpy as np
import pytest

import elt_models as em
import gate_models as gm
from test_gpu_onnx_elementwise import device, heads_close

F = gm.F
BATCHES = (1, 2, 3)


@pytest.fixture(scope="module")
def boards(nsg):
    bb = nsg.synth.random_batch(3, 86, seed=31)
    return bb, nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)


def shown(policy, kind):
    """The 27 shown channels of a policy [N,2187]: [N,27,81] for spatial and token rows, [N,27] for flat rows."""
    return policy[:, :F] if kind == "flat" else policy.reshape(len(policy), F, 81)


def check_exact(nsg, net, data, boards, tmp_path):
    """The policy of batches 1, 2, 3 equals the float64 reference rounded per op, bit for bit; the heads are within 1e-4."""
    bb, x = boards
    ref = net.run(x, rounded=True)
    assert np.isfinite(ref["policy"]).all()
    info, outs = device(nsg, data, bb, tmp_path, BATCHES)
    for n, o in outs:
        np.testing.assert_array_equal(o[0], ref["policy"][:n].astype(np.float32))
    heads_close(outs, net.run(x, rounded=False))
    return info, outs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["spatial", "token", "flat", "board"])
@pytest.mark.parametrize("op", gm.BINARY)
def test_every_broadcast_of_an_exact_gate(nsg, boards, tmp_path, kind, op):
    """x op g and g op x, the gate |channel 5| + 1 of the same rows (kSrcRowOne) or of the board's flat row
    (kSrcBoardOne); then the bare Slice, a one-channel view at channel offset 5, and the gate behind an Expand."""
    for side, plain, expand in (("right", False, False), ("left", False, True), ("left", True, False)):
        if op == "Div" and plain:  # the bare channel has zeros
            continue
        net, data = gm.bcast_model(nsg, kind, op, side, plain_gate=plain, expand=expand)
        check_exact(nsg, net, data, boards, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["spatial", "token"])
def test_a_constant_per_square(nsg, boards, tmp_path, kind):
    for op in ("Mul", "Add", "Sub"):
        net, data = gm.square_const_model(nsg, kind, op)
        check_exact(nsg, net, data, boards, tmp_path)


@pytest.mark.gpu
def test_a_token_score_from_a_dense_launch(nsg, boards, tmp_path):
    """tok * (tok @ w[27,1]): the score is written by the dense launch and read at channel 0 of its row.  Without the
    Sigmoid every sum and product is on the grid: bit for bit.  With it (riding in the dense launch) the gate is within
    1.28 ulps of a value below 1, so |err| <= |tok| 2 * 1.28 u + u |y|."""
    net, data = gm.score_model(nsg)
    env = net.run(boards[1], rounded=False)
    assert gm.rm.on_grid(env["score"], -5) and gm.rm.on_grid(env["y"], -8)
    check_exact(nsg, net, data, boards, tmp_path)
    bb, x = boards
    net, data = gm.score_model(nsg, sigmoid=True)
    env = net.run(x, rounded=False)
    tok = np.abs(env["tok"]).transpose(0, 2, 1).reshape(3, -1)
    bound = tok * 2 * 1.28 * gm.U + gm.U * np.abs(env["policy"])
    _, outs = device(nsg, data, bb, tmp_path, BATCHES)
    for n, o in outs:
        err = np.abs(o[0].astype(np.float64) - env["policy"][:n])
        assert (err <= bound[:n]).all(), float((err / np.maximum(bound[:n], 1e-300)).max())
    heads_close(outs, env)


@pytest.mark.gpu
def test_the_value_head_as_a_gate(nsg, boards, tmp_path):
    """kSrcBoardOne reading the [N,1] value tensor: policy = s * value, with the value the device itself returned."""
    bb, x = boards
    net, data = gm.value_gate_model(nsg)
    s = net.run(x, rounded=False)["s"]
    _, outs = device(nsg, data, bb, tmp_path, BATCHES)
    for n, o in outs:
        want = em.f32(s[:n] * o[1].astype(np.float64).reshape(n, 1, 1, 1)).reshape(n, -1)
        np.testing.assert_array_equal(o[0], want.astype(np.float32))
    heads_close(outs, net.run(x, rounded=False))


@pytest.mark.gpu
@pytest.mark.parametrize("off", gm.OFFSETS)
@pytest.mark.parametrize("kind", ["spatial", "token", "flat"])
def test_max_min_and_exact_sums(nsg, boards, tmp_path, kind, off):
    """C in {1, 3, 4, 16, 17, 27, 64, 100} at the offset, 24 launches in one model, the channel behind the widest view at
    1e30: a read past offset + C would show in the C = 100 results, a read of a neighbouring row nowhere else."""
    net, data, names = gm.reduce_model(nsg, kind, off)
    rows = gm.reduce_inputs(net, boards[1], kind, off, 100)
    assert gm.sums_exact(rows, -3)
    info, outs = check_exact(nsg, net, data, boards, tmp_path)
    got = shown(outs[-1][1][0], kind)
    for i, (op, C) in enumerate(names):  # and directly, against numpy on the float64 rows
        v = rows[..., :C]
        want = {"ReduceMax": v.max, "ReduceMin": v.min, "ReduceSum": v.sum}[op](axis=-1)
        np.testing.assert_array_equal(got[:, i], want.astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["token", "flat"])
def test_exact_means(nsg, boards, tmp_path, kind):
    """ReduceMean over token and flat channels: the exact sum times float32(1 / C), rounded once."""
    net, data, names = gm.reduce_model(nsg, kind, 1, ops=["ReduceMean"])
    assert gm.sums_exact(gm.reduce_inputs(net, boards[1], kind, 1, 100), -3)
    check_exact(nsg, net, data, boards, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("kind", ["spatial", "token", "flat"])
def test_sums_that_round_are_inside_the_bound(nsg, boards, tmp_path, kind, off):
    """The 2^-11 grid with channel offsets of 4096 and -1024: |err| <= gamma(C) sum|x|, the mean's over C plus u |mean|."""
    bb, x = boards
    ops = ["ReduceSum"] + (["ReduceMean"] if kind != "spatial" else [])
    net, data, names = gm.reduce_model(nsg, kind, off, ops=ops, exp=-11, fine=True)
    rows = gm.reduce_inputs(net, x, kind, off, 100)
    assert not gm.sums_exact(rows, -11)
    _, outs = device(nsg, data, bb, tmp_path, BATCHES)
    for (_, one), (_, whole) in zip(outs, outs[1:]):
        np.testing.assert_array_equal(one[0], whole[0][:len(one[0])])
    got = shown(outs[-1][1][0], kind).astype(np.float64)
    worst = 0.0
    for i, (op, C) in enumerate(names):
        v = rows[..., :C]
        mean = op == "ReduceMean"
        ref, bound = v.sum(axis=-1) / (C if mean else 1), gm.sum_bound(v, mean)
        g = got[:, i]
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(np.abs(g - ref) == 0, 0.0, np.abs(g - ref) / bound)
        print(kind, off, op, C, "error / bound", float(r.max()))
        worst = max(worst, float(r.max()))
    assert worst <= 1.0, worst


def lone_board(nsg):
    """Three positions and a plane that is zero on every square of the first and positive on every square of the others:
    a centre tap of 1e30 on that plane puts the neighbours' whole stem at 1e30 and leaves the first board's bits alone."""
    bb = nsg.synth.random_batch(19, 86, seed=31)
    x = nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9)
    for p in range(86):
        zero = [b for b in range(19) if not x[b, p].any()]
        full = [b for b in range(19) if x[b, p].min() > 0]
        if zero and len(full) >= 2:
            return bb, p, zero[0], full[:2]
    raise AssertionError("no plane tells one position from two others on every square")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["spatial", "flat"])
def test_a_board_between_neighbours_at_1e30(nsg, tmp_path, kind):
    """A board alone, and as the first, middle and last of three whose other boards hold 1e30 in every stem channel: equal
    bits.  The reduce at C = 17, offset 1 (spatial rows: read back through kSrcRowOne; the flat global max: through
    kSrcBoardOne)."""
    bb, p, me, others = lone_board(nsg)
    net = gm.GNet(nsg)
    net.stem(F)
    net.consts["s_w"][:, p, 1, 1] = gm.POISON
    x, axis = gm.rows_of(net, kind, F)
    r = net.reduce("ReduceSum", net.slice(x, 1, 18, axis, "v"), "r", 1)
    if kind == "flat":
        r = net.node("Reshape", [r, net.const("to4", [-1, 1, 1, 1], np.int64)], "r4")
    net.show(net.node("Mul", ["s", r], "y"), "spatial")
    net.heads_of("s", F)
    path = tmp_path / "m.onnx"
    path.write_bytes(net.data())
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    alone = ev.compute_blocking(bb[[me]])[0][0].copy()
    assert np.isfinite(alone).all() and float(np.abs(alone).max()) < 1e6
    for pos in range(3):
        order = others[:pos] + [me] + others[pos:]
        whole = ev.compute_blocking(bb[order])[0].copy()
        assert not np.isfinite(whole[(pos + 1) % 3]).all() or float(np.abs(whole[(pos + 1) % 3]).max()) > 1e29
        np.testing.assert_array_equal(whole[pos], alone)
    ev.close()


@pytest.mark.gpu
def test_the_pad_channels_of_a_reduced_row_are_zero(nsg, boards, tmp_path):
    """A 1x1 conv of ones reads the reduced row's whole 16-channel chunk against zero pad weights, directly and behind an
    Exp (one more one-channel row): a pad that held a NaN or an infinity would come out as NaN, and the product by the
    weight 1 is exact, so the policy is the reduction (its Exp within 2 ulps) on all 27 channels.  A finite value in a pad
    is multiplied by zero and cannot show here or anywhere: every reader of a row takes its C channels or meets the pad
    with a zero weight.  So the last case makes the result itself infinite (two channels at 3e38, their sum overflows): a
    kernel that wrote its result to every channel of the row would turn inf * 0 into NaN; with zero pads the policy is inf."""
    bb, x = boards
    for op, through_exp, overflow in (("ReduceMax", False, False), ("ReduceSum", False, False), ("ReduceMin", True, False),
                                      ("ReduceSum", False, True)):
        net = gm.GNet(nsg)
        net.stem(F + 1)
        net.consts["s_w"][F], net.consts["s_b"][F] = 0.0, gm.POISON  # the channel behind the view
        if overflow:
            net.consts["s_w"][:2], net.consts["s_b"][:2] = 0.0, 3e38
        r = net.reduce(op, net.slice("s", 0, F, 1, "v"), "r", 1)
        if through_exp:
            r = net.node("Exp", [r], "e")
        net.node("Conv", [r, net.const("ones", np.ones((F, 1, 1, 1)))], "y", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
        net.show("y", "spatial")
        net.heads_of("s", F + 1)
        with np.errstate(over="ignore"):
            ref = net.run(x, rounded=True)["policy"]
        _, outs = device(nsg, net.data(), bb, tmp_path, BATCHES)
        for n, o in outs:
            if overflow:
                assert np.isposinf(ref).all() and np.isposinf(o[0]).all()
                continue
            assert np.isfinite(o[0]).all()
            if through_exp:
                assert float(np.abs(o[0] / ref[:n] - 1).max()) <= 2 * 2.0 ** -23
            else:
                np.testing.assert_array_equal(o[0], ref[:n].astype(np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("block,expand", [("scse", False), ("scse", True), ("cbam", False)])
def test_exported_gate_blocks_against_torch_float64(nsg, boards, tmp_path, block, expand):
    """scSE and CBAM-with-sum within the siblings' 1e-4 of torch in float64; the opset 13 and 17 exports agree bit for bit."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_onnx_norm_golden as gen
    import torch
    bb, x = boards
    net = gm.randomize(gm.gate_net(block, expand=expand), 5)
    with torch.no_grad():
        want = [t.numpy() for t in net.double()(torch.from_numpy(x))]
    net.float()
    res = {}
    for opset in (13, 17):
        torch.manual_seed(1)
        data = gen.export_model(net.eval(), str(tmp_path / f"e{opset}.onnx"), fold=False, opset=opset)
        _, outs = device(nsg, data, bb, tmp_path, (3,))
        res[opset] = outs[0][1]
        for got, ref in zip(res[opset], want):
            assert float(np.abs(got.reshape(ref.shape).astype(np.float64) - ref).max()) < 1e-4
    for a, b in zip(res[13], res[17]):
        np.testing.assert_array_equal(a, b)
