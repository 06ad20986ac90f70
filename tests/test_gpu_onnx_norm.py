"""GroupNorm, InstanceNorm, decomposed and channel-last LayerNorm and RMSNorm on the device: the normalisation fixture
against its float64 PyTorch outputs, batch independence, a (C, G) sweep of GroupNorm bare and inside a residual block, a
GroupNorm on a Split output at an unaligned channel offset, the bit identities between forms that plan to the same
launch, an RMSNorm sweep on tokens and on a flat tensor, and the evaluator contract on the fixture."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

NAME = "net_graph_norm"


def gid(v):
    return str(v).replace(" ", "")


@pytest.fixture(scope="module")
def gen():
    import make_onnx_norm_golden
    return make_onnx_norm_golden


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(f"{golden_dir}/net_norm.npz"))
    g["bitboards"] = np.load(f"{golden_dir}/net_graph.npz")["bitboards86"]
    g[f"{NAME}_policy"] = np.concatenate([np.load(f"{golden_dir}/{NAME}_policy_{h}.npz")["policy"] for h in range(2)])
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


def device_outputs(nsg, path, bb, batches=(1, 19)):
    ev = nsg.Evaluator(0, 32, 86)
    ev.load(str(path))
    assert ev.graph_info()["path"] == "graph"
    outs = [(n, [o.copy() for o in ev.compute_blocking(bb[:n])]) for n in batches]
    ev.close()
    return outs


def run(nsg, gen, net, boards, path, opset=17):
    """Exports `net`, runs it on the device at batches 1 and 19 and returns [(n, outputs)] and the float64 reference of
    the same module on the CPU."""
    import torch
    bb, x = boards
    gen.export_model(net.float(), str(path), opset=opset)
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(x)]
    return device_outputs(nsg, path, bb), ref


def err_against_float64(nsg, gen, net, boards, path, opset=17):
    outs, ref = run(nsg, gen, net, boards, path, opset)
    return max(max_err(o, [r[:n] for r in ref]) for n, o in outs)


def same_bits(nsg, gen, boards, tmp_path, a, b):
    """Two exports that must plan to the same launches: equal outputs bit for bit at batches 1 and 19, and the first
    within the bound of its float64 reference."""
    (net_a, opset_a), (net_b, opset_b) = a, b
    outs_a, ref = run(nsg, gen, net_a, boards, tmp_path / "a.onnx", opset_a)
    gen.export_model(net_b.float(), str(tmp_path / "b.onnx"), opset=opset_b)
    outs_b = device_outputs(nsg, tmp_path / "b.onnx", boards[0])
    for (n, oa), (_, ob) in zip(outs_a, outs_b):
        for x, y in zip(oa, ob):
            np.testing.assert_array_equal(x, y)
        assert max_err(oa, [r[:n] for r in ref]) < 1e-4


@pytest.mark.gpu
def test_norm_fixture_matches_pytorch(nsg, golden_dir, golden):
    ref = [golden[f"{NAME}_policy"], golden[f"{NAME}_value"], golden[f"{NAME}_draw"]]
    ev = nsg.Evaluator(0, 64, 86, precision="fp32")
    ev.load(f"{golden_dir}/{NAME}.onnx")
    info = ev.graph_info()
    assert info["path"] == "graph" and info["precision"] == "fp32"
    for n in (1, 6, 17, 64):
        out = ev.compute_blocking(golden["bitboards"][:n])
        err = max_err(out, [r[:n] for r in ref])
        print(NAME, n, "max abs err", err)
        assert err < 1e-4, (n, err)
    assert ev.last_plan()["trunk_precision"] == "fp32"
    ev.close()


@pytest.mark.gpu
def test_a_board_does_not_depend_on_its_batch(nsg, golden_dir, golden):
    ev = nsg.Evaluator(0, 64, 86)
    ev.load(f"{golden_dir}/{NAME}.onnx")
    bb = golden["bitboards"][:37]
    whole = [x.copy() for x in ev.compute_blocking(bb)]
    for b in range(37):
        one = ev.compute_blocking(bb[b:b + 1])
        for x, y in zip(one, whole):
            np.testing.assert_array_equal(x[0], y[b])
    ev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["bare", "block"])
@pytest.mark.parametrize("C,G", [(24, 3), (24, 24), (24, 1), (30, 5), (27, 3), (40, 5), (72, 8), (64, 4)], ids=gid)
def test_groupnorm_sweep(nsg, gen, boards, tmp_path, C, G, full):
    """(24,3): pad channels and a group across the 16-channel chunk; (24,24): instance norm; (24,1): one group;
    (30,5) and (27,3): groups of 6 and 9 channels, no multiples of 4, (27,3) with an odd width; (40,5), (72,8):
    groups that straddle chunks, more than 64 channels and so more than one workgroup per board; (64,4): no pad
    channels, groups of a whole chunk.  bare: the normalisation alone, without gamma and beta; block: gamma and beta,
    a fused ReLU and a residual."""
    import torch
    torch.manual_seed(C * 7 + G)
    net = gen.randomize(gen.GNSweepNet(C, G, full), C + G).eval()
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "gn.onnx")
    print(C, G, full, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
@pytest.mark.parametrize("C,G,split", [(24, 3, 6), (30, 5, 6), (24, 24, 3), (24, 1, 8)], ids=gid)
def test_groupnorm_reads_a_split_output_where_it_lies(nsg, gen, boards, tmp_path, C, G, split):
    """The normalised part starts at channel 6 or 3 of the stem's rows, no multiples of 4 (scalar loads), or at 8."""
    import torch
    torch.manual_seed(C + G + split)
    net = gen.randomize(gen.GNSweepNet(C, G, True, split=split), C + split).eval()
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "s.onnx")
    print(C, G, split, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
@pytest.mark.parametrize("C,G", [(199, 1), (200, 1), (202, 1), (400, 2), (208, 1), (416, 2), (192, 1)], ids=gid)
def test_groupnorm_around_the_lds_threshold(nsg, gen, boards, tmp_path, C, G):
    """A group of 199 channels is the widest whose 81 rows, with the kernel's static LDS, fit 64 KB (65 004 bytes) and
    are staged; a group of 200 (65 652 bytes with a stride of 201) is the first that is not: its second and third pass
    re-read global memory.  202: the next even width; (400,2) and (416,2): two unstaged workgroups per board; 192 and
    208: the nearest widths that 16 divides, without pad channels."""
    import torch
    torch.manual_seed(C + G)
    net = gen.randomize(gen.GNSweepNet(C, G, True), C + G).eval()
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "w.onnx")
    print(C, G, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
def test_instancenorm_and_groupnorm_per_channel_give_equal_bits(nsg, gen, boards, tmp_path):
    import torch
    import torch.nn as nn
    C = 24
    torch.manual_seed(3)
    a = gen.randomize(gen.NormNet(C, nn.InstanceNorm2d(C, affine=True), act=True), 9).eval()
    b = gen.NormNet(C, nn.GroupNorm(C, C), act=True).eval()
    b.load_state_dict(a.state_dict())
    assert float((b.mid.weight - 1).abs().min()) > 0 and float(b.mid.bias.abs().min()) > 0
    same_bits(nsg, gen, boards, tmp_path, (a, 17), (b, 17))


@pytest.mark.gpu
@pytest.mark.parametrize("domain", ["token", "spatial"], ids=["tokens", "channel_last"])
def test_opset_13_and_17_layernorm_give_equal_bits(nsg, gen, boards, tmp_path, domain):
    import torch
    import torch.nn as nn
    C = 24
    torch.manual_seed(4)
    net = gen.randomize(gen.NormNet(C, nn.LayerNorm(C) if domain == "token" else gen.ChanLastLN(C), domain), 11).eval()
    same_bits(nsg, gen, boards, tmp_path, (net, 13), (net, 17))


@pytest.mark.gpu
def test_the_two_written_rmsnorm_forms_give_equal_bits(nsg, gen, boards, tmp_path):
    import torch
    C = 24
    torch.manual_seed(5)
    a = gen.randomize(gen.NormNet(C, gen.RMSNorm(C, form="rsqrt"), "token"), 13).eval()
    b = gen.NormNet(C, gen.RMSNorm(C, form="div"), "token").eval()
    b.load_state_dict(a.state_dict())
    same_bits(nsg, gen, boards, tmp_path, (a, 17), (b, 17))


@pytest.mark.gpu
@pytest.mark.parametrize("domain", ["token", "flat"])
@pytest.mark.parametrize("C", [24, 64, 72])
def test_rmsnorm_sweep(nsg, gen, boards, tmp_path, C, domain):
    """24: pad channels, fewer channels than lanes; 64: one channel per lane; 72: a second pass of the lanes."""
    import torch
    torch.manual_seed(C)
    net = gen.randomize(gen.NormNet(C, gen.RMSNorm(C, form="rsqrt" if C != 64 else "div"), domain), C).eval()
    err = err_against_float64(nsg, gen, net, boards, tmp_path / "rms.onnx")
    print(C, domain, "max abs err", err)
    assert err < 1e-4, err


@pytest.mark.gpu
def test_evaluator_contract_on_the_norm_fixture(nsg, golden_dir, golden):
    path = f"{golden_dir}/{NAME}.onnx"
    ref = [golden[f"{NAME}_policy"], golden[f"{NAME}_value"], golden[f"{NAME}_draw"]]
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
    assert sh.graph_info()["path"] == "graph" and sh.graph_info()["conv_launches"] == 13
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
