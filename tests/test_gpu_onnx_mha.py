"""PyTorch's stock transformer modules on the device ("stock transformer modules").

A module and its hand-written twin (tests/mha_models.py) plan to the same launches, so at head dimension 16, where
the scale 16^-1/2 = sqrt(1/4) * sqrt(1/4) = 1/4 is exact however the exporter splits it, the two models must agree
bit for bit; the plans' scales are compared first, so that a mismatch there is reported as what it is.  At other head
dimensions the folded scale may differ by an f32 ulp, and the module is held against itself in float64 on the CPU with
the bound of the other exported attention models (tests/test_gpu_onnx_attention.py: 1e-4).  Batches of 1, 2 and 3 real
positions of net_graph.npz; a board's bits do not depend on its batch."""
import os
import re
import subprocess

import numpy as np
import pytest

import mha_models as mm

PLAN_DUMP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nshogi-engine_amd", "csrc", "plan_dump")
BATCHES = (1, 2, 3)
TOL = 1e-4  # test_gpu_onnx_attention.py's bound for an exported attention model against float64


@pytest.fixture(scope="module")
def boards(nsg, golden_dir):
    import torch
    bb = np.load(f"{golden_dir}/net_graph.npz")["bitboards86"][:3]
    x = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64))
    return bb, x


def scales(path):
    """(heads, head dimension, scale as printed bit for bit) of every attention launch of the model's plan."""
    out = subprocess.run([PLAN_DUMP, str(path)], check=True, capture_output=True, text=True).stdout
    assert "ERROR" not in out, out
    return re.findall(r"heads=([1-9]\d*) headDim=(\d+) scale=(\S+)", out)


def run(nsg, path, bb):
    """The outputs for the first 1, 2 and 3 boards."""
    ev = nsg.Evaluator(0, 4, 86)
    ev.load(str(path))
    assert ev.graph_info()["path"] == "graph"
    outs = [[np.array(o, copy=True) for o in ev.compute_blocking(bb[:n])] for n in BATCHES]
    ev.close()
    return outs


def max_err(out, ref, n):
    return max(float(np.abs(np.asarray(o, np.float64).reshape(n, -1) - np.asarray(r)[:n].reshape(n, -1)).max()) for o, r in zip(out, ref))


def same_board_in_every_batch(outs):
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            np.testing.assert_array_equal(a[0], b[0])


EXACT = [("mha", 32, 2, dict(need_weights=False)), ("mha", 48, 3, dict(need_weights=False)),
         ("mha", 32, 2, dict(need_weights=True, batch_first=False)),  # the 3-D form on [N*H,81,d]
         ("enc", 32, 2, dict(ffn=64, norm_first=True, activation="relu"))]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,E,H,kw", EXACT, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_a_module_and_its_twin_agree_bit_for_bit(nsg, boards, tmp_path, kind, E, H, kw):
    bb, _ = boards
    net = mm.make(kind, E, H, seed=E + H, **kw)
    mm.export(net, tmp_path / "module.onnx")
    mm.export(mm.twin(net), tmp_path / "twin.onnx")
    got, want = scales(tmp_path / "module.onnx"), scales(tmp_path / "twin.onnx")
    assert got == want == [(str(H), "16", "0x1p-2")], (got, want)
    a, b = run(nsg, tmp_path / "module.onnx", bb), run(nsg, tmp_path / "twin.onnx", bb)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v)
    same_board_in_every_batch(a)


ROUNDED = [("mha", 24, 2, dict(need_weights=True)),  # d = 12 in rows of stride 32: pad channels in play
           ("enc", 64, 1, dict(ffn=96, norm_first=False, activation="gelu"))]  # d = 64, the limit; a whole post-norm layer


@pytest.mark.gpu
@pytest.mark.parametrize("kind,E,H,kw", ROUNDED, ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_a_module_against_itself_in_float64(nsg, boards, tmp_path, kind, E, H, kw):
    """Measured on an MI355X (max abs error over policy, value and draw, batches of 1 to 3; module, twin):
    see DESIGN.md section 13.3."""
    import torch
    bb, x = boards
    net = mm.make(kind, E, H, seed=E + H, **kw)
    mm.export(net, tmp_path / "module.onnx")
    mm.export(mm.twin(net), tmp_path / "twin.onnx")
    with torch.no_grad():
        ref = [t.numpy() for t in net.double()(x)]
        ref_twin = [t.numpy() for t in mm.twin(net).double()(x)]
    # the twin is the same function: float64 says so before the device is asked
    assert max_err(ref_twin, ref, 3) < 1e-12
    print(kind, E, H, "scales", scales(tmp_path / "module.onnx"), scales(tmp_path / "twin.onnx"))
    a, b = run(nsg, tmp_path / "module.onnx", bb), run(nsg, tmp_path / "twin.onnx", bb)
    err = max(max_err(o, ref, n) for o, n in zip(a, BATCHES))
    err_twin = max(max_err(o, ref, n) for o, n in zip(b, BATCHES))
    print(kind, E, H, "max abs err vs float64: module", err, "twin", err_twin)
    assert err < TOL, err
    assert err_twin < TOL, err_twin
    same_board_in_every_batch(a)
