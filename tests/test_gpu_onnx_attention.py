"""Token models on the device: the attention fixtures against their float64 PyTorch outputs, batch independence, a
sweep of small attention modules exported at test time (head dimensions 8 to 64, bias, where the scale stands, fused
or separate QKV), LayerNorm alone, and the evaluator contract on an attention model."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

ATT_MODELS = ["net_att_pre", "net_att_hybrid"]
BATCH_MAX = 96


@pytest.fixture(scope="module")
def gen():
    import make_onnx_attention_golden
    return make_onnx_attention_golden


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(f"{golden_dir}/net_att.npz"))
    g["bitboards"] = np.load(f"{golden_dir}/net_graph.npz")["bitboards86"]
    for name in ATT_MODELS:
        g[f"{name}_policy"] = np.concatenate([np.load(f"{golden_dir}/{name}_policy_{h}.npz")["policy"] for h in range(2)])
    return g


@pytest.fixture(scope="module")
def boards(nsg):
    """19 seeded positions and their planes as a float64 tensor, shared by the test-time models."""
    import torch
    bb = nsg.synth.random_batch(19, 86, seed=31)
    x = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64))
    return bb, x


def max_err(out, ref):
    return max(float(np.abs(np.asarray(o, np.float64).reshape(-1) - np.asarray(r).reshape(-1)).max()) for o, r in zip(out, ref))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ATT_MODELS)
def test_attention_fixtures_match_pytorch(nsg, golden_dir, golden, name):
    ref = [golden[f"{name}_policy"], golden[f"{name}_value"], golden[f"{name}_draw"]]
    ev = nsg.Evaluator(0, BATCH_MAX, 86, precision="fp32")
    ev.load(f"{golden_dir}/{name}.onnx")
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32" and info["attention_launches"] > 0
    for n in (1, 6, 17, 64, BATCH_MAX):
        idx = np.arange(n) % 64
        out = ev.compute_blocking(golden["bitboards"][idx])
        err = max_err(out, [r[idx] for r in ref])
        print(name, n, "max abs err", err)
        assert err < 1e-4, (name, n, err)
    assert ev.last_plan()["trunk_precision"] == "fp32"
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ATT_MODELS)
def test_a_board_does_not_depend_on_its_batch(nsg, golden_dir, golden, name):
    ev = nsg.Evaluator(0, BATCH_MAX, 86)
    ev.load(f"{golden_dir}/{name}.onnx")
    bb = golden["bitboards"][:37]
    whole = [x.copy() for x in ev.compute_blocking(bb)]
    for b in range(37):
        one = ev.compute_blocking(bb[b:b + 1])
        for x, y in zip(one, whole):
            np.testing.assert_array_equal(x[0], y[b])
    ev.close()


def run_against_float64(nsg, gen, net, boards, path, batches=(1, 19)):
    """Exports `net` with the shared recipe, runs it on the device and returns the largest error against the same
    module in float64 on the CPU."""
    import torch
    bb, x = boards
    gen.export_model(net, str(path))
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(x)]
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    assert ev.graph_info()["path"] == "graph"
    err = 0.0
    for n in batches:
        err = max(err, max_err(ev.compute_blocking(bb[:n]), [r[:n] for r in ref]))
    ev.close()
    return err, ref


@pytest.mark.gpu
@pytest.mark.parametrize("FH,bias,scale_on,fused", list(itertools.product(
    [(32, 4), (48, 3), (64, 2), (64, 1)], [False, True], ["q", "k", "scores"], [True, False])))
def test_attention_sweep(nsg, gen, boards, tmp_path, FH, bias, scale_on, fused):
    """Head dimensions 8, 16, 32 and 64 (8 is no multiple of the 16-wide fragment, 64 the largest allowed)."""
    import torch
    F, H = FH
    torch.manual_seed(F * 100 + H * 10 + bias * 4 + fused)
    net = gen.randomize(gen.AttNet(F, H, bias=bias, scale_on=scale_on, fused=fused), F + H).eval()
    x = boards[1]
    sds = gen.sharpen(net, x.float())
    assert all(1.0 < s < 4.0 for s in sds), sds
    # a kernel that ignored the scores, or let the padded keys 81..95 in, would not pass: uniform weights move the
    # float64 output by far more than the tolerance
    net.double()
    with torch.no_grad():
        sharp = net(x)
        net.att.uniform = True
        flat = net(x)
        net.att.uniform = False
    moved = max(float((a - b).abs().max()) for a, b in zip(sharp, flat))
    assert moved > 1e-3, moved
    err, _ = run_against_float64(nsg, gen, net.float(), boards, tmp_path / "att.onnx")
    print(F, H, bias, scale_on, fused, "max abs err", err, "uniform moves", moved)
    assert err < 1e-4, err


@pytest.mark.gpu
def test_a_scale_computed_from_size(nsg, gen, boards, tmp_path):
    """`q.size(-1) ** -0.5` (Shape / Gather / Cast / Pow in the file) folded on the host, with k transposed in one permute."""
    import torch
    torch.manual_seed(9)
    net = gen.randomize(gen.AttNet(32, 4, bias=True, k_perm=True, tweak="size_scale"), 9).eval()
    assert all(1.0 < s < 4.0 for s in gen.sharpen(net, boards[1].float()))
    err, _ = run_against_float64(nsg, gen, net, boards, tmp_path / "size.onnx")
    print("size-derived scale max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
def test_layernorm_alone(nsg, gen, boards, tmp_path):
    """C = 24 in rows of stride 32 (pad channels in play), eps = 1e-3, on token rows and on a flat [N,20] tensor."""
    import torch
    torch.manual_seed(5)
    net = gen.randomize(gen.LNNet(F=24, VH=20, eps=1e-3), 6).eval()
    err, _ = run_against_float64(nsg, gen, net, boards, tmp_path / "ln.onnx")
    print("layernorm max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
def test_evaluator_contract_on_an_attention_model(nsg, golden_dir, golden):
    path = f"{golden_dir}/net_att_pre.onnx"
    ref = [golden["net_att_pre_policy"], golden["net_att_pre_value"], golden["net_att_pre_draw"]]
    bb = golden["bitboards"][:16]
    ev = nsg.Evaluator(0, 16, 86)
    ev.load(path)
    p, v, d = [x.copy() for x in ev.compute_blocking(bb)]
    # gather
    rng = np.random.default_rng(4)
    counts = rng.integers(1, 40, size=16)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    idx = np.concatenate([rng.choice(2187, c, replace=False) for c in counts]).astype(np.uint16)
    vals, v2, d2 = ev.compute_gather_blocking(bb, idx, off)
    np.testing.assert_array_equal(vals, np.concatenate([p[b, idx[off[b]:off[b + 1]]] for b in range(16)]))
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(d2, d)
    # nsg_load_shared on the same device: identical outputs
    sh = nsg.Evaluator(0, 16, 86)
    sh.load_shared(ev)
    assert sh.graph_info()["path"] == "graph" and sh.graph_info()["attention_launches"] == 2
    for x, y in zip(sh.compute_blocking(bb), (p, v, d)):
        np.testing.assert_array_equal(x, y)
    # an f16m6 evaluator runs the general graph in fp32
    m6 = nsg.Evaluator(0, 16, 86, precision="f16m6")
    m6.load(path)
    info = m6.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    o6 = m6.compute_blocking(bb)
    assert m6.last_plan()["trunk_precision"] == "fp32"
    assert max_err(o6, [r[:16] for r in ref]) < 1e-4
    for x in (ev, sh, m6):
        x.close()
