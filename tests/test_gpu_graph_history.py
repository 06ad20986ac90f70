"""Buffer reuse and forward history of the general graph path on the device.

Topologies: every model of tests/topology_models.py at batches 1, 2 and 3 on an evaluator of batch_max 3.  The exact
cases equal their float64 reference bit for bit, the attention cases stay inside 1e-4, and a board's bits do not depend
on its batch.  tests/test_plan_lifetimes.py shows that these models reach every view field of the lifetime pass.

History: activation buffers are zeroed once at load; after the first forward each holds what its tenants left.  For the
13 golden models and every topology, evaluator A (fresh) runs the real boards at n = batch_max and n = 1; evaluator B
first runs batch_max poison boards -- every plane the stem reads set on every square with one large value -- then the
same two forwards: equal bits; then the poison once more and n = 1 again: still equal.  The poison scale is chosen per
model from a ladder, the largest at which the float64 reference of the poison forward is finite in every tensor with
room for float32 (ROOM, below).  The test asserts that, that the device's poison outputs are finite, and that the median
|stem output| of the poison boards is at least 1e3 times that of the real boards; on the topology models, whose only
activation is Relu, the same holds for the tensor the stem's launch stores, so the large values reach the buffers.
Figures are printed before they are asserted."""
import os

import numpy as np
import pytest

import onnx_ref64
import plan_check as pc
import topology_models as tm
from test_plan_lifetimes import GOLDEN_REFS, golden_case

SCALES = (1e30, 1e24, 1e18, 1e12, 1e9, 1e6, 1e5, 1e4)
# "finite throughout" for a float32 evaluation: every tensor of the float64 reference stays below 1e15, so that a
# kernel may square a value (a variance, a mean of squares) or sum 1e8 of them in any order and stay below 3.4e38
ROOM = 1e15


def planes_of(nsg, bb, planes):
    return nsg.synth.expand_reference(bb, True).reshape(-1, planes, 9, 9).astype(np.float64)


def poison_boards(nsg, n, planes, scale):
    one = nsg.synth.pack(np.ones((1, planes, 81), bool), np.zeros((1, planes), bool), np.full((1, planes), scale, np.float32))
    return np.concatenate([one] * n)


def stem_of(nsg, data, path, planes):
    """(the stem's own output, the tensor its launch stores): the output of the first node that computes with the planes
    (a Shape node reads no data), and the output of the last node that rides in launch 0 (an activation behind the stem
    is fused into its launch, so the stem's own output may never be stored)."""
    nodes = nsg.onnx_io.read_onnx(data)[0]
    first = next(nd for nd in nodes if "input" in nd.inputs and nd.op != "Shape")
    last = pc.dump([path], planes)[0].names[0].split("+")[-1]
    stored = next(nd for nd in nodes if nd.name == last)
    return first.outputs[0], stored.outputs[0]


def choose_poison(nsg, data, path, planes, real_x):
    """(scale, ratio of the median |stem output|, the same ratio on what the stem's launch stores, poison bitboards of
    one board): the largest scale of the ladder at which every tensor of the float64 reference of the poison forward is
    finite and below ROOM."""
    stem, stored = stem_of(nsg, data, path, planes)
    real = onnx_ref64.run(nsg, data, real_x)
    for scale in SCALES:
        bb = poison_boards(nsg, 1, planes, scale)
        with np.errstate(all="ignore"):
            env = onnx_ref64.run(nsg, data, planes_of(nsg, bb, planes))
        if all(np.isfinite(v).all() and float(np.abs(v).max(initial=0.0)) < ROOM for v in env.values() if v.dtype.kind == "f"):
            ratios = [float(np.median(np.abs(env[t]))) / max(float(np.median(np.abs(real[t]))), 1e-300) for t in (stem, stored)]
            return scale, ratios[0], ratios[1], bb
    raise AssertionError("no poison scale of the ladder keeps the float64 reference finite")


def forward(ev, bb):
    with np.errstate(all="ignore"):
        return [np.array(o, copy=True) for o in ev.compute_blocking(bb)]


def evaluator(nsg, path, batch_max, planes, force=False):
    ev = nsg.Evaluator(0, batch_max, planes)
    if force:  # the three family models too run on the general path
        ev.set_graph_mode("force")
    ev.load(str(path))
    assert ev.graph_info()["path"] == "graph"
    return ev


def same_bits(a, b, what):
    for x, y, nm in zip(a, b, ("policy", "value", "draw")):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{what}: {nm}")


def history(nsg, path, data, planes, batch_max, bb, label, force=False, stored_too=False):
    """stored_too: the ratio is asserted on the tensor the stem's launch stores as well (the topology models, whose
    activations are all Relu; a fixture's stem may carry a Tanh, whose output no poison can make 1e3 times larger)."""
    scale, ratio, stored, one = choose_poison(nsg, data, path, planes, planes_of(nsg, bb, planes))
    poison = np.concatenate([one] * batch_max)
    a = evaluator(nsg, path, batch_max, planes, force)
    a_full, a_one = forward(a, bb), forward(a, bb[:1])
    a.close()
    b = evaluator(nsg, path, batch_max, planes, force)
    p1 = forward(b, poison)
    b_full, b_one = forward(b, bb), forward(b, bb[:1])
    p2 = forward(b, poison)
    b_again = forward(b, bb[:1])
    b.close()
    finite = all(np.isfinite(o).all() for o in p1 + p2)
    equal = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a_full + a_one + a_one, b_full + b_one + b_again))
    print(f"history {label}: poison scale {scale:g}, stem ratio {ratio:.3g}, ratio of what the stem launch stores {stored:.3g}, "
          f"poison outputs finite {finite}, bits equal {equal}")
    assert ratio >= 1e3, ratio
    assert stored >= 1e3 or not stored_too, stored
    assert finite
    assert all(np.isfinite(o).all() for o in a_full)
    same_bits(a_full, b_full, f"{label}: n = {batch_max} after the poison")
    same_bits(a_one, b_one, f"{label}: n = 1 after the poison")
    same_bits(a_one, b_again, f"{label}: n = 1 after the second poison")
    same_bits(a_one, [y[:1] for y in a_full], f"{label}: n = 1 against n = {batch_max}")
    return a_full


@pytest.fixture(scope="module")
def boards(nsg):
    bb = nsg.synth.random_batch(3, 86, seed=31)
    return bb, planes_of(nsg, bb, 86)


_REF = {}


def topo_reference(nsg, name, x):
    if name not in _REF:
        _REF[name] = tm.reference(nsg, tm.build(nsg, name), x)
    return _REF[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", tm.NAMES)
def test_topologies_match_float64_at_every_batch(nsg, boards, tmp_path, name):
    bb, x = boards
    topo = tm.build(nsg, name)
    ref = topo_reference(nsg, name, x)
    path = tmp_path / "m.onnx"
    path.write_bytes(topo.data)
    ev = evaluator(nsg, path, 3, 86)
    outs = {n: forward(ev, bb[:n]) for n in (1, 2, 3)}
    ev.close()
    err = max(float(np.abs(np.asarray(o, np.float64).reshape(3, -1) - r.reshape(3, -1)).max()) for o, r in zip(outs[3], ref))
    print(f"topology {name}: exact case {topo.exact}, largest error against float64 {err:.3e}")
    for n in (1, 2):
        same_bits(outs[n], [whole[:n] for whole in outs[3]], f"{name}: batch {n} against batch 3")
    for o, r, nm in zip(outs[3], ref, ("policy", "value", "draw")):
        if topo.exact:
            np.testing.assert_array_equal(o.reshape(3, -1), r.reshape(3, -1).astype(np.float32), err_msg=f"{name}: {nm}")
        else:
            assert err < 1e-4, (name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("name", tm.NAMES)
def test_topologies_do_not_depend_on_what_their_buffers_held(nsg, boards, tmp_path, name):
    bb, x = boards
    topo = tm.build(nsg, name)
    path = tmp_path / "m.onnx"
    path.write_bytes(topo.data)
    got = history(nsg, path, topo.data, 86, 3, bb, name, stored_too=True)
    ref = topo_reference(nsg, name, x)
    for o, r in zip(got, ref):  # and A itself is right
        if topo.exact:
            np.testing.assert_array_equal(o.reshape(3, -1), r.reshape(3, -1).astype(np.float32))
        else:
            assert float(np.abs(o.reshape(3, -1) - r.reshape(3, -1)).max()) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLDEN_REFS))
def test_golden_models_do_not_depend_on_what_their_buffers_held(nsg, golden_dir, name):
    data, planes, bb, ref = golden_case(nsg, golden_dir, name, 8)
    idx = np.arange(8) % len(bb)  # (the three family models have six stored boards)
    got = history(nsg, os.path.join(golden_dir, name + ".onnx"), data, planes, 8, bb[idx], name, force=True)
    err = max(float(np.abs(np.asarray(o, np.float64).reshape(8, -1) - r[idx].reshape(8, -1)).max()) for o, r in zip(got, ref))
    print(f"fixture {name}: largest error against the stored float64 outputs {err:.3e}")
    assert err < 1e-4, (name, err)
