"""The general graph path on the device: models outside the ResNet family against their float64 PyTorch outputs,
batch independence, family models forced onto the general path against the specialised path and the oracle, and
the evaluator contract (gather, busy, sharing, precision, debug hooks) on a general graph."""
import numpy as np
import pytest

GRAPH_MODELS = [("net_graph_se", 86), ("net_graph_gpool93", 93), ("net_graph_softplus", 86), ("net_graph_views", 86)]
FAMILY_MODELS = ["net_torch_2x64", "net_torch_bn_1x64", "net_torch_sigtanh_eps_1x64"]
BATCH_MAX = 96


def load_golden(golden_dir):
    """net_graph.npz with each model's float64 policy joined from its two files (tests/golden/make_onnx_graph_golden.py)."""
    g = dict(np.load(f"{golden_dir}/net_graph.npz"))
    for name, _ in GRAPH_MODELS:
        g[f"{name}_policy"] = np.concatenate([np.load(f"{golden_dir}/{name}_policy_{h}.npz")["policy"] for h in range(2)])
    return g


def positions(g, planes, n):
    bb = g["bitboards86"] if planes == 86 else g["bitboards93"]
    idx = np.arange(n) % len(bb)
    return bb[idx], idx


def max_err(out, ref):
    return max(float(np.abs(np.asarray(o, np.float64) - r).max()) for o, r in zip(out, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("name,planes", GRAPH_MODELS)
def test_graph_models_match_pytorch(nsg, golden_dir, name, planes):
    g = load_golden(golden_dir)
    ref = [g[f"{name}_policy"], g[f"{name}_value"], g[f"{name}_draw"]]
    ev = nsg.Evaluator(0, BATCH_MAX, planes, precision="fp32")
    ev.load(f"{golden_dir}/{name}.onnx")
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["activation_bytes"] > 0
    for n in (1, 6, 17, 64, BATCH_MAX):
        bb, idx = positions(g, planes, n)
        out = ev.compute_blocking(bb)
        assert max_err(out, [r[idx] for r in ref]) < 1e-4, (name, n)
    assert ev.last_plan()["trunk_precision"] == "fp32"
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,planes", GRAPH_MODELS)
def test_a_board_does_not_depend_on_its_batch(nsg, golden_dir, name, planes):
    g = load_golden(golden_dir)
    ev = nsg.Evaluator(0, BATCH_MAX, planes)
    ev.load(f"{golden_dir}/{name}.onnx")
    bb, _ = positions(g, planes, 37)
    whole = [x.copy() for x in ev.compute_blocking(bb)]
    for b in range(37):
        one = ev.compute_blocking(bb[b:b + 1])
        for x, y in zip(one, whole):
            np.testing.assert_array_equal(x[0], y[b])
    ev.close()


@pytest.mark.gpu
def test_family_width_48_loads_on_the_general_path(nsg, oracle, tmp_path):
    """Trunk width 48 and value hidden width 32 are refused by the specialised loader (multiples of 64 only)."""
    w = nsg.weights.make_random(1, 48, value_channels=8, value_hidden=32, seed=3, bn="random")
    path = tmp_path / "w48.onnx"
    nsg.onnx_io.export_onnx(w, str(path))
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    assert ev.graph_info()["path"] == "graph"
    bb = nsg.synth.random_batch(32, 86, seed=11)
    assert max_err(ev.compute_blocking(bb), oracle.net(nsg.weights.to_blob(w)).evaluate(bb)) < 1e-4
    ev.close()


def family_cases(nsg, golden_dir, tmp_path):
    for name in FAMILY_MODELS:
        yield name, f"{golden_dir}/{name}.onnx"
    w = nsg.weights.make_random(6, 128, seed=9, bn="random")
    path = tmp_path / "r6x128.onnx"
    nsg.onnx_io.export_onnx(w, str(path))
    yield "random_6x128", str(path)


@pytest.mark.gpu
def test_family_models_forced_onto_the_general_path(nsg, oracle, golden_dir, tmp_path):
    bb = nsg.synth.random_batch(40, 86, seed=12)
    for name, path in family_cases(nsg, golden_dir, tmp_path):
        spec = nsg.Evaluator(0, 40, 86, precision="fp32")
        spec.load(path)
        assert spec.graph_info()["path"] == "specialised"
        gen = nsg.Evaluator(0, 40, 86)
        gen.set_graph_mode("force")
        gen.load(path)
        assert gen.graph_info()["path"] == "graph"
        a, b = spec.compute_blocking(bb), gen.compute_blocking(bb)
        for x, y in zip(a, b):
            scale = max(1.0, float(np.abs(x).max()))
            assert float(np.abs(x - y).max()) <= 1e-5 * scale, name
        with open(path, "rb") as f:
            blob = nsg.convert_onnx(f.read())
        assert max_err(b, oracle.net(blob).evaluate(bb)) < 1e-4, name
        spec.close()
        gen.close()


@pytest.mark.gpu
def test_gather_on_a_general_graph(nsg, golden_dir):
    g = load_golden(golden_dir)
    ev = nsg.Evaluator(0, 16, 86)
    ev.load(f"{golden_dir}/net_graph_se.onnx")
    bb, _ = positions(g, 86, 16)
    p, v, d = [x.copy() for x in ev.compute_blocking(bb)]
    rng = np.random.default_rng(4)
    counts = rng.integers(1, 40, size=16)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    idx = np.concatenate([rng.choice(2187, c, replace=False) for c in counts]).astype(np.uint16)
    vals, v2, d2 = ev.compute_gather_blocking(bb, idx, off)
    want = np.concatenate([p[b, idx[off[b]:off[b + 1]]] for b in range(16)])
    np.testing.assert_array_equal(vals, want)
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(d2, d)
    soft, _, _ = ev.compute_gather_blocking(bb, idx, off, softmax=True)
    for b in range(16):
        row = p[b, idx[off[b]:off[b + 1]]].astype(np.float64)
        e = np.exp(row - row.max())
        assert float(np.abs(soft[off[b]:off[b + 1]] - e / e.sum()).max()) < 1e-6
    ev.close()


@pytest.mark.gpu
def test_a_second_batch_in_flight_is_busy(nsg, tmp_path):
    # a forward of some milliseconds (6x128 forced onto the general path, 512 boards): the second call comes first
    w = nsg.weights.make_random(6, 128, seed=2)
    path = tmp_path / "r6x128.onnx"
    nsg.onnx_io.export_onnx(w, str(path))
    ev = nsg.Evaluator(0, 512, 86)
    ev.set_graph_mode("force")
    ev.load(str(path))
    bb = nsg.synth.random_batch(512, 86, seed=8)
    outs = [np.empty((512, 2187), np.float32), np.empty(512, np.float32), np.empty(512, np.float32)]
    lib = nsg.load_library()
    pinned = [bb] + outs  # page-locked, so that the copies of the call are asynchronous too
    for a in pinned:
        assert lib.nsg_host_register(a.ctypes.data, a.nbytes) == 0
    try:
        ev.compute_nonblocking(bb, policy=outs[0], win=outs[1], draw=outs[2])
        with pytest.raises(nsg.NsgError) as e:  # one batch in flight (trt.cc:237-238)
            ev.compute_nonblocking(bb)
        assert e.value.code == -5
        ev.await_()
        for x, y in zip(outs, ev.compute_blocking(bb)):
            np.testing.assert_array_equal(x, y)
    finally:
        for a in pinned:
            lib.nsg_host_unregister(a.ctypes.data)
    ev.close()


@pytest.mark.gpu
def test_evaluator_contract_on_a_general_graph(nsg, golden_dir):
    g = load_golden(golden_dir)
    path = f"{golden_dir}/net_graph_se.onnx"
    ref = [g["net_graph_se_policy"], g["net_graph_se_value"], g["net_graph_se_draw"]]
    bb, idx = positions(g, 86, 64)
    ev = nsg.Evaluator(0, 64, 86)
    ev.load(path)
    out = ev.compute_blocking(bb)
    # nsg_load_shared on the same device: identical outputs
    sh = nsg.Evaluator(0, 64, 86)
    sh.load_shared(ev)
    assert sh.graph_info()["path"] == "graph"
    for x, y in zip(sh.compute_blocking(bb), out):
        np.testing.assert_array_equal(x, y)
    # an f16m6 evaluator runs the general graph in fp32
    m6 = nsg.Evaluator(0, 64, 86, precision="f16m6")
    m6.load(path)
    info = m6.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    o6 = m6.compute_blocking(bb)
    assert m6.last_plan()["trunk_precision"] == "fp32"
    assert max_err(o6, [r[idx] for r in ref]) < 1e-4
    # launch queries report zeros for a general-graph forward
    lp = m6.last_plan()
    assert (lp["boards_per_group"], lp["fragments_per_wave"], lp["waves_per_group"], lp["chains"]) == (0, 0, 0, 0)
    # the debug hooks of the specialised layout refuse
    for call in (lambda: ev.download_trunk(4), lambda: ev.download_planes_raw(4), lambda: ev.time_planes(4, 2)):
        with pytest.raises(nsg.NsgError) as e:
            call()
        assert e.value.code == -1 and "general graph" in str(e.value)
    # profiling counts the conv launches as trunk launches
    ev.profile_enable(True)
    ev.compute_blocking(bb)
    prof = ev.profile_read()
    assert prof["forwards"] == 1 and prof["trunk_launches"] == ev.graph_info()["conv_launches"]
    assert 0 < prof["trunk_ms_total"] <= prof["forward_ms_total"]
    for x in (ev, sh, m6):
        x.close()
