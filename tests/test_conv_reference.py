"""The references, bounds, faults and models of tests/conv_models.py, checked on the host: no device needed.

  1. Every case's float64 reference equals torch's own float64 conv2d / avg_pool2d / max_pool2d / linear on the same
     operands (a dilated average, which torch's avg_pool2d does not know, against torch's unfold).
  2. Every exact case satisfies its below-2^24 assertion (`inputs`), has a reference that float32 holds, and shows
     something in every output channel; a plain float32 numpy evaluation gives the reference bit for bit there and
     stays inside the bound on every rounded case.
  3. Each fault of FAULTS moves at least one shown element of each device case built for it: any change on an exact
     case, more than the bound on a rounded one.  The geometry cases also tell the transposed kernel, the swapped
     dilations and the kernel without its outermost taps apart at square 0 and at square 40.
  4. Each model plans as exactly one launch of the intended kind -- tile, geo, depthwise, pool or dense layer -- with the
     geometry, the residual view and the fused ReLU of the case, read off plan_dump's line of the launch."""
import re
import subprocess

import numpy as np
import pytest

import conv_models as cm
from reduction_models import ratio
from test_plan_snapshot import PLAN_DUMP

ALL = list(cm.CONV) + list(cm.POOL) + list(cm.DENSE)


@pytest.fixture(scope="module")
def planes(nsg):
    """The seeded positions of the sibling files as float64 planes: 19, and the 163 of the dense cases."""
    bb = nsg.synth.random_batch(163, 86, seed=31)
    x = nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)
    return {False: nsg.synth.expand_reference(nsg.synth.random_batch(19, 86, seed=31), True).reshape(-1, 86, 9, 9).astype(np.float64), True: x}


def operands(nsg, planes, name):
    case = cm.case(nsg, name)
    return case, case.inputs(planes[name in cm.DENSE])


def torch_ref(case, inp):
    import torch
    import torch.nn.functional as F
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    x = t(inp["x"])
    if case.kind == "dense":
        if case.hidden:
            x = torch.relu(F.linear(x, t(case.w1), t(case.b1)))
        return F.linear(x, t(case.w), t(case.b)).numpy()
    (kh, kw), (dh, dw) = case.k, case.d
    pad = (cm.halo(kh, dh), cm.halo(kw, dw))
    if case.kind == "pool":
        if case.mode == "max":  # (max_pool2d takes pads up to half the kernel: the halo of -inf is put there first)
            halo = F.pad(x, (pad[1], pad[1], pad[0], pad[0]), value=float("-inf"))
            return F.max_pool2d(halo, (kh, kw), 1, 0, (dh, dw)).numpy()
        if (dh, dw) == (1, 1):
            return F.avg_pool2d(x, (kh, kw), 1, pad, count_include_pad=case.mode == "avg_include").numpy()
        N, C = x.shape[:2]
        total = F.unfold(x, (kh, kw), (dh, dw), pad).reshape(N, C, kh * kw, 81).sum(dim=2)
        count = F.unfold(torch.ones(1, 1, 9, 9, dtype=torch.float64), (kh, kw), (dh, dw), pad).sum(dim=1)
        return (total / (count if case.mode == "avg_exclude" else float(kh * kw))).reshape(N, C, 9, 9).numpy()
    y = F.conv2d(x, t(case.w), t(case.b), 1, pad, (dh, dw), case.cout if case.depthwise else 1)
    if case.res is not None:
        y = y + t(inp["r"][:, case.res:case.res + case.cout])
    return (torch.relu(y) if case.relu else y).numpy()


@pytest.mark.parametrize("name", ALL)
def test_the_reference_is_torchs_and_float32_fits_the_bound(nsg, planes, name):
    case, inp = operands(nsg, planes, name)  # (inputs holds the below-2^24 assertion of an exact case)
    ref, bound = case.ref(inp), case.bound(inp)
    want = torch_ref(case, inp)
    if case.kind == "pool" and case.mode != "max":
        np.testing.assert_allclose(case.quotient(inp), want, rtol=1e-15, atol=0)  # (torch may multiply by 1 / n)
    elif case.exact:
        np.testing.assert_array_equal(ref, want)
    else:
        np.testing.assert_allclose(ref, want, rtol=0, atol=1e-12)
    assert np.isfinite(ref).all()
    case.every_channel_shows(ref)
    got = case.emulate(inp)
    if case.exact:
        assert not bound.any() and np.array_equal(ref, cm.em.f32(ref))
        np.testing.assert_array_equal(got, ref.astype(np.float32))
    else:
        assert float(bound.min()) > 0.0
        r = ratio(got, ref, bound)
        print(name, "float32 error / bound", r, "largest bound", float(bound.max()))
        assert 0.0 < r <= 1.0, r


def moved(case, inp, fault):
    ref, bound = case.ref(inp), case.bound(inp)
    bad = case.ref(inp, fault)
    return any(ratio(case.select(bad, p), case.select(ref, p), case.select(bound, p)) > 1.0 for p in case.parts)


@pytest.mark.parametrize("fault", cm.FAULTS)
def test_each_fault_is_caught_by_the_device_cases_built_for_it(nsg, planes, fault):
    assert sorted(cm.FAULT_CASES) == sorted(cm.FAULTS) and cm.FAULT_CASES[fault]
    for name in cm.FAULT_CASES[fault]:
        case, inp = operands(nsg, planes, name)
        assert moved(case, inp, fault), (fault, name)


def outermost_zeroed(w):
    w = w.copy()
    for ax in (2, 3):
        if w.shape[ax] > 1:
            idx = [slice(None)] * 4
            for edge in (0, -1):
                idx[ax] = edge
                w[tuple(idx)] = 0
    return w


@pytest.mark.parametrize("name", list(cm.GEO) + [n for n in cm.ROUNDED if n.startswith("r_g")])
def test_geometry_cases_tell_the_axes_apart_at_a_corner_and_at_the_centre(nsg, planes, name):
    """The transposed kernel, the swapped dilations (where they differ) and the kernel without its outermost taps each
    change the policy at square 0 and at square 40."""
    case, inp = operands(nsg, planes, name)
    ref = case.ref(inp)
    cut = cm.ConvCase(nsg, **cm.CONV[name])
    cut.w = outermost_zeroed(case.w)
    others = {"outermost_zeroed": cut.ref(inp), "kernel_transposed": case.ref(inp, "kernel_transposed")}
    if case.d[0] != case.d[1]:
        others["dilations_swapped"] = case.ref(inp, "dilations_swapped")
    for what, other in others.items():
        for sq in (0, 40):
            assert (ref.reshape(*ref.shape[:2], 81)[:, :, sq] != other.reshape(*ref.shape[:2], 81)[:, :, sq]).any(), (what, sq)


def launch_lines(data, tmp_path):
    path = tmp_path / "d.onnx"
    path.write_bytes(data)
    out = subprocess.run([PLAN_DUMP, str(path)], check=True, capture_output=True, text=True).stdout
    assert "ERROR" not in out, out
    return [(m.group(1), line) for line in out.splitlines() if (m := re.match(r"#\d+ kind=\d+ name=(\S+)", line))]


@pytest.mark.parametrize("name", ALL)
def test_each_model_is_one_launch_of_the_kernel_it_names(nsg, tmp_path, name):
    case = cm.case(nsg, name)
    want, res = case.plan()
    for part in case.parts:
        lines = launch_lines(case.model(part), tmp_path)
        under = [(n, l) for n, l in lines if n.startswith("kut")]
        assert len(under) == case.launches, [n for n, _ in lines]
        assert {n for n, _ in lines if not n.startswith("kut")} <= case.others(), [n for n, _ in lines]
        n, line = under[-1]
        fused = "kut" + ("+kadd" if getattr(case, "res", None) is not None else "") + ("+kact" if getattr(case, "relu", False) else "")
        assert n == fused, n
        for w in want:
            assert w in line, (w, line)
        assert re.search(res, line), (res, line)
        if case.kind in ("tile", "geo", "depthwise"):  # which kernel runs it: ConvArgs::kernel()
            (kh, kw), (dh, dw) = case.k, case.d
            tile = kh == kw and kh in (1, 3) and dh == dw == 1
            assert case.kind == ("depthwise" if " depthwise=1 " in line else "tile" if tile else "geo")


def test_the_tap_groups_the_geometries_reach():
    """15 taps go as 8 + 7 (a boundary inside a kernel row), 63 as eight full groups; 21, 27, 35 and 45 in between."""
    taps = sorted({g[0] * g[1] for g in cm.GEOMETRIES})
    assert taps == [9, 15, 21, 25, 27, 35, 45, 63]
    assert [cm.tap_group(t) for t in taps] == [5, 8, 7, 7, 7, 7, 8, 8]
