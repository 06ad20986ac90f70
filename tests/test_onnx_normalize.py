"""The general graph path's host half on the L1 / L2 norms, the sum of squares, the log-sum-exp and F.normalize
(nsg_inspect_onnx, plan_dump): each reduction over the channels is one kLaunchChanReduce with its own mode, the exporter's
F.normalize chain is one kLaunchNormalize, a chain that deviates stays a reduction plus elementwise launches, and what
stays outside is refused with the node and the reason.  No device needed.  Before these modes every model here but the
ReduceProd one was refused with "op 'ReduceL2' is outside the supported op set" (or L1, SumSquare, LogSumExp)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import gate_models as gm
import normalize_models as nm
from test_plan_snapshot import PLAN_DUMP

F = nm.F


@pytest.fixture(scope="module")
def gen():
    import make_onnx_norm_golden
    return make_onnx_norm_golden


def export(gen, net, tmp_path, name="m.onnx", opset=17, fold=False):
    import torch
    torch.manual_seed(1)
    return gen.export_model(net.eval(), str(tmp_path / name), fold=fold, opset=opset)


def refused(nsg, data, *needles):
    with pytest.raises(nsg.NsgError) as e:
        nsg.inspect_onnx(data, 86)
    assert e.value.code == -4, e.value
    for n in needles:
        assert n in str(e.value), str(e.value)


def dump(data, tmp_path):
    """plan_dump's launch lines of the model, in order."""
    path = tmp_path / "d.onnx"
    path.write_bytes(data)
    out = subprocess.run([PLAN_DUMP, str(path)], check=True, capture_output=True, text=True).stdout
    assert "ERROR" not in out, out
    return [line for line in out.splitlines() if re.match(r"#\d+ kind=\d+ ", line)]


def of_kind(lines, kind):
    return [l for l in lines if f" kind={kind} " in l]


def front(f, mods=()):
    from test_onnx_linepool import front as fr
    return fr(f, mods=mods)


def tokens(x):
    return x.flatten(2).transpose(1, 2)


def untokens(t):
    return t.transpose(1, 2).reshape(-1, 86, 9, 9)


def eps_of(line):
    return np.float32(float.fromhex(re.search(r" eps=(\S+) ", line).group(1)))


# ---- plans: F.normalize ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opset", [13, 17])
def test_the_exported_normalize_is_one_launch(nsg, gen, tmp_path, opset):
    import torch
    import torch.nn.functional as Fn
    cases = [
        ("spatial", lambda x: Fn.normalize(x, dim=1), 2, 1e-12, "in=-1/96/0/86/s"),
        ("tokens", lambda x: untokens(Fn.normalize(tokens(x), dim=-1)), 2, 1e-12, "in=-1/96/0/86/s"),
        ("l1", lambda x: Fn.normalize(x, p=1.0, dim=1), 1, 1e-12, "in=-1/96/0/86/s"),
        ("eps", lambda x: Fn.normalize(x, dim=1, eps=1e-3), 2, 1e-3, "in=-1/96/0/86/s"),
        ("slice", lambda x: torch.cat([x[:, :4], Fn.normalize(x[:, 4:44], dim=1), x[:, 44:]], 1), 2, 1e-12, "in=-1/96/4/40/s"),
        ("flat", lambda x: x * Fn.normalize(x.amax(dim=(2, 3)), dim=-1).reshape(-1, 86, 1, 1), 2, 1e-12, "/96/0/86/f"),
    ]
    for name, f, p, eps, view in cases:
        data = export(gen, front(f), tmp_path, f"{name}.onnx", opset)
        assert (b"ReduceL1" if p == 1 else b"ReduceL2") in data and b"Clip" in data and b"Div" in data
        lines = dump(data, tmp_path)
        norm = of_kind(lines, 16)
        assert len(norm) == 1 and not of_kind(lines, 15), (name, lines)
        assert f" normP={p} " in norm[0] and eps_of(norm[0]) == np.float32(eps) and view in norm[0], (name, norm[0])
        assert re.search(r"name=\S*Reduce\S*\+\S*Clip\S*\+\S*Div ", norm[0]), norm[0]
        info = nsg.inspect_onnx(data, 86)
        assert info["path"] == "graph" and info["launches"] == len(lines) + 2


def test_normalize_adds_a_launch_and_no_flops(nsg, gen, tmp_path):
    import torch.nn.functional as Fn
    base = nsg.inspect_onnx(export(gen, front(lambda x: x), tmp_path, "b.onnx"), 86)
    info = nsg.inspect_onnx(export(gen, front(lambda x: Fn.normalize(x, dim=1)), tmp_path, "n.onnx"), 86)
    assert info["launches"] == base["launches"] + 1 and info["flops_per_position"] == base["flops_per_position"]


def test_hand_built_normalize_on_every_kind_of_row(nsg, tmp_path):
    for kind in ("spatial", "token", "flat"):
        for off, C, p, expand in ((0, 27, 2, True), (4, 40, 1, False), (3, 17, 2, True)):
            _, data, _ = nm.normalize_model(nsg, kind, off, C, p=p, eps=1e-6, expand=expand)
            norm = of_kind(dump(data, tmp_path), 16)
            assert len(norm) == 1 and f" normP={p} " in norm[0] and eps_of(norm[0]) == np.float32(1e-6), (kind, off, C)
            W = max(off + C, F)
            stride = (W + 15) // 16 * 16
            assert re.search(rf" out=\d+/{(C + 15) // 16 * 16}/0/{C}/{'f' if kind == 'flat' else 's'} in=\d+/{stride}/{off}/{C}/", norm[0]), norm[0]


# ---- plans: the reductions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opset", [13, 17])
def test_norms_and_logsumexp_are_one_reduction_each(nsg, gen, tmp_path, opset):
    import torch
    cases = [
        (lambda x: x * x.norm(dim=1, keepdim=True), 5, 1),
        (lambda x: x * torch.linalg.vector_norm(x, dim=1, keepdim=True), 5, 1),
        (lambda x: untokens(tokens(x) * torch.linalg.vector_norm(tokens(x), dim=-1, keepdim=True)), 5, 1),
        (lambda x: x * torch.logsumexp(x, 1, keepdim=True), 6, 1),
        (lambda x: x - torch.logsumexp(x, 1, keepdim=True), 6, 1),
        (lambda x: x * x.norm(p=1, dim=1, keepdim=True), 3, 1),
    ]
    for i, (f, mode, elt) in enumerate(cases):
        lines = dump(export(gen, front(f), tmp_path, f"r{i}.onnx", opset), tmp_path)
        red = of_kind(lines, 15)
        assert len(red) == 1 and f" redMode={mode} " in red[0] and " in=-1/96/0/86/s " in red[0] and " out=0/16/0/1/s " in red[0], (i, lines)
        assert len(of_kind(lines, 1)) == elt and not of_kind(lines, 16), (i, lines)


def test_every_new_mode_on_every_kind_both_forms_of_the_axes(nsg, tmp_path):
    for kind in ("spatial", "token", "flat"):
        items = [(op, off, C) for op in nm.REDUCE for off, C in ((0, 27), (3, 17))]
        _, data = nm.pack_model(nsg, kind, items, 40)
        red = of_kind(dump(data, tmp_path), 15)
        assert [int(re.search(r" redMode=(\d+) ", l).group(1)) for l in red] == [nm.MODE[op] for op, _, _ in items]
        for l, (op, off, C) in zip(red, items):
            assert re.search(rf" in=\d+/48/{off}/{C}/", l) and " scale=0x1p+0 " in l, l
    for op in nm.REDUCE:  # `axes` as an input (the opset-18 form)
        net = nm.NNet(nsg)
        net.stem(F)
        net.show(net.widen(net.reduce(op, "s", "r", 1, as_input=True), "spatial"), "spatial")
        net.heads_of("s", F)
        assert len(of_kind(dump(net.data(), tmp_path), 15)) == 1, op


# ---- chains that deviate stay a reduction plus elementwise launches ----------------------------------------------------
def test_fallbacks_load_as_two_launches_or_more(nsg, gen, tmp_path):
    import torch
    cases = {
        "second reader": nm.normalize_model(nsg, "spatial", 0, F, twin=True)[1],
        "eps 0": nm.normalize_model(nsg, "spatial", 0, F, eps=0.0)[1],
        "eps < 0": nm.normalize_model(nsg, "token", 0, F, eps=-1.0)[1],
        "max bound": nm.normalize_model(nsg, "spatial", 0, F, clip_max=5.0)[1],
        "exported clamp(min, max)": export(gen, front(lambda x: x / x.norm(dim=1, keepdim=True).clamp(min=1e-3, max=5.0)), tmp_path, "c.onnx"),
        "another numerator": export(gen, front(lambda x: x.abs() / x.norm(dim=1, keepdim=True).clamp(min=1e-3)), tmp_path, "a.onnx"),
        "reciprocal": export(gen, front(lambda x: x * (1.0 / x.norm(dim=1, keepdim=True).clamp(min=1e-3))), tmp_path, "m.onnx"),
    }
    for name, data in cases.items():
        lines = dump(data, tmp_path)
        assert len(of_kind(lines, 15)) == 1 and len(of_kind(lines, 1)) >= 1 and not of_kind(lines, 16), (name, lines)
        assert nsg.inspect_onnx(data, 86)["path"] == "graph"
    # an Expand to another shape than x's does not fuse: its nodes are lowered one by one, and the Div refuses the shape
    net = nm.NNet(nsg)
    net.stem(F)
    net.show(net.normalize("s", 1, "y", expand_to=[1, 2 * F, 9, 9]), "spatial")
    net.heads_of("s", F)
    refused(nsg, net.data(), "node 'y'", "[N,54,9,9]")


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_name_the_node(nsg, gen, tmp_path):
    import torch
    cases = [
        (lambda x: x * x.norm(dim=1).unsqueeze(1), "/ReduceL2", ("[N,86,9,9]", "keepdims = 0", "[N,9,9] is ambiguous")),
        (lambda x: x * torch.logsumexp(x, 1).unsqueeze(1), "/ReduceLogSumExp", ("keepdims = 0", "keeps the axis")),
        (lambda x: x * x.norm(dim=(2, 3), keepdim=True), "/ReduceL2", ("[N,86,9,9]", "over the channels only")),
        (lambda x: untokens(tokens(x) * tokens(x).norm(dim=1, keepdim=True)), "/ReduceL2", ("over the channels only",)),
        (lambda x: x * torch.logsumexp(x, (2, 3), keepdim=True), "/ReduceLogSumExp", ("over the channels only",)),
        (lambda x: x * x.prod(1, keepdim=True), "/ReduceProd", ("op 'ReduceProd'", "outside the supported op set")),
    ]
    for i, (f, node, needles) in enumerate(cases):
        refused(nsg, export(gen, front(f), tmp_path, f"x{i}.onnx"), node, *needles)


def test_cosine_similarity_keeps_its_refusal(nsg, gen, tmp_path):
    import torch.nn.functional as Fn
    refused(nsg, export(gen, front(lambda x: x * Fn.cosine_similarity(x, x.abs(), dim=1).unsqueeze(1)), tmp_path), "keepdims = 0")


@pytest.mark.parametrize("opset", [13, 17])
def test_the_cosine_policy_model_plans(nsg, gen, tmp_path, opset):
    """Two kLaunchNormalize on token rows at E = 32, their product one kLaunchBmm, the log-softmax one reduction."""
    lines = dump(export(gen, gm.randomize(nm.cosine_net(), 3), tmp_path, opset=opset, fold=True), tmp_path)
    norm = of_kind(lines, 16)
    assert len(norm) == 2 and all(" normP=2 " in l and "/32/0/32/s" in l for l in norm), lines
    assert len(of_kind(lines, 11)) == 1
    red = of_kind(lines, 15)
    assert len(red) == 1 and " redMode=6 " in red[0]


# ---- the float64 definitions the device tests use -----------------------------------------------------------------------
def test_the_reference_of_the_log_sum_exp_at_its_edges():
    a = np.array([[-np.inf] * 5, [1e4] * 5, [3.0, -np.inf, -np.inf, -np.inf, -np.inf], [1.0, np.inf, 0.0, 0.0, 0.0]])
    r = nm.reduce64("ReduceLogSumExp", a, (1,)).reshape(-1)
    assert np.isneginf(r[0]) and r[1] == 1e4 + np.log(5.0) and r[2] == 3.0 and np.isposinf(r[3])
    assert nm.reduce64("ReduceL2", np.array([[3.0, -4.0]]), (1,))[0, 0] == 5.0
    assert nm.reduce64("ReduceL1", np.array([[3.0, -4.0]]), (1,))[0, 0] == 7.0
    assert nm.reduce64("ReduceSumSquare", np.array([[3.0, -4.0]]), (1,))[0, 0] == 25.0
