"""The buffer assignment of the general graph planner against the rules R1-R5 of DESIGN.md section 13.7, on the CPU:
`plan_dump --lifetimes` through tests/plan_check.py.

Coverage: the 13 golden models, the topology models of tests/topology_models.py and one model from each sibling case
list.  Teeth: a plan mutated against one rule is rejected with that rule's name.  Fields: for every view field of
forEachView there is a topology in which a lifetime pass that forgets the field lets two live tensors collide, so the
device tests on those topologies (tests/test_gpu_graph_history.py) reach every field.  Also here, because the device
tests lean on them: the float64 interpreter against the outputs stored beside the golden models, and the swapped-operand
sensitivity of the topologies that cannot be exact."""
import copy
import glob
import os

import numpy as np
import pytest

import onnx_ref64
import plan_check as pc
import topology_models as tm
from test_plan_snapshot import PLANES

# every field of forEachView and the three outputs; one line mode stands for the three
FIELDS = ("in", "res", "attK", "attV", "rtBias", "bmmB", "seg", "srcSame", "srcBoard", "policy", "value", "draw")
LINE_FIELDS = ("srcRankLine", "srcFileLine", "srcLine")


@pytest.fixture(scope="module")
def golden_plans(golden_dir):
    plans = pc.dump(sorted(glob.glob(os.path.join(golden_dir, "*.onnx"))), PLANES)
    assert len(plans) == 13
    return plans


@pytest.fixture(scope="module")
def topo_plans(nsg, tmp_path_factory):
    d = tmp_path_factory.mktemp("topo")
    paths = []
    for name in tm.NAMES:
        paths.append(d / f"{name}.onnx")
        paths[-1].write_bytes(tm.build(nsg, name).data)
    return dict(zip(tm.NAMES, pc.dump(paths)))


def sibling_models(nsg, d):
    """One model from each case list of the sibling *_models files."""
    import attention_bias_models as abm
    import bmm_models as bm
    import elt_models as em
    import gather_models as gam
    import group_models as gm
    import line_models as lm
    import mix_models as mm
    import reduction_models as rm
    out = {"elt": em.family_model(nsg, "pooled_sum", 8)[1], "reduction": rm.AttCase(nsg, 32, 2).data,
           "bmm": bm.case(nsg, "ntnn").data, "mix": mm.case(nsg, next(iter(mm.EXACT))).data,
           "gather": gam.case(nsg, next(iter(gam.CASES))).data, "attention_bias": abm.RtAttCase(nsg, 64, 4).data}
    paths = []
    for k, data in out.items():
        paths.append(d / f"{k}.onnx")
        paths[-1].write_bytes(data)
    gm.export(gm.randomize(gm.ResNeXtNet(32, 8, blocks=3), 68).eval(), d / "group.onnx")
    gm.export(lm.randomize(lm.coord_att_net("reduce"), 11), d / "line.onnx")
    return paths + [d / "group.onnx", d / "line.onnx"]


def assert_clean(plans):
    for p in plans:
        assert pc.check(p) == [], p.name
        assert len(p.launches) >= 5 and any(len(ts) > 1 for ts in tenants(p).values()), p.name  # something is reused


def tenants(p):
    t = {}
    for v, (lo, hi) in p.intervals().items():
        t.setdefault(p.virts[v].phys, []).append((lo, hi, v))
    return t


# ---- coverage ----------------------------------------------------------------------------------------------------------
def test_the_golden_models_keep_the_rules(golden_plans):
    assert_clean(golden_plans)


def test_the_topology_models_keep_the_rules(topo_plans):
    assert_clean(topo_plans.values())


def test_one_model_of_each_sibling_case_list_keeps_the_rules(nsg, tmp_path):
    plans = pc.dump(sibling_models(nsg, tmp_path))
    assert len(plans) == 8
    assert_clean(plans)
    seen = {f for p in plans for f in pc.fields(p)}
    assert {"attK", "attV", "rtBias", "bmmB"} <= seen and seen & set(LINE_FIELDS), seen


# ---- teeth -------------------------------------------------------------------------------------------------------------
def every_plan(golden_plans, topo_plans):
    return list(golden_plans) + list(topo_plans.values())


def rename(p, virt, phys):
    p.virts[virt].phys = phys
    for _, r, _ in p.touches():
        if r.virt == virt:
            r.phys = phys


def test_merging_two_overlapping_tenants_breaks_r1(golden_plans, topo_plans):
    for p0 in every_plan(golden_plans, topo_plans):
        iv, done = p0.intervals(), 0
        for a, (alo, ahi) in iv.items():
            for b, (blo, bhi) in iv.items():
                if a < b and p0.virts[a].phys != p0.virts[b].phys and alo <= bhi and blo <= ahi and p0.virts[a].spatial == p0.virts[b].spatial and done < 6:
                    p = copy.deepcopy(p0)
                    rename(p, b, p.virts[a].phys)
                    assert "R1" in pc.rules(p), (p0.name, a, b)
                    done += 1
        assert done, p0.name


def test_the_output_of_a_launch_on_the_buffer_of_its_input_breaks_r1(topo_plans):
    """Intervals that meet in one launch collide."""
    for p0 in topo_plans.values():
        row = p0.launches[4]
        read = next(r for r in row[:-1] if r.used)
        p = copy.deepcopy(p0)
        rename(p, row[-1].virt, read.phys)
        assert "R1" in pc.rules(p), p0.name


def test_a_read_before_its_write_breaks_r2(golden_plans, topo_plans):
    for p0 in every_plan(golden_plans, topo_plans):
        # a launch that reads the output of the launch before it: swap the two
        i = next(i for i in range(1, len(p0.launches)) if any(r.used and r.virt == p0.launches[i - 1][-1].virt for r in p0.launches[i][:-1]))
        p = copy.deepcopy(p0)
        p.launches[i - 1], p.launches[i] = p.launches[i], p.launches[i - 1]
        assert "R2" in pc.rules(p), p0.name
        # and the first launch reading what the last one writes
        p = copy.deepcopy(p0)
        p.launches[0][0] = copy.copy(p.launches[-1][-1])
        p.launches[0][0].field = "in"
        assert "R2" in pc.rules(p), p0.name


def test_a_late_write_to_an_output_buffer_breaks_r3(golden_plans, topo_plans):
    for p0 in every_plan(golden_plans, topo_plans):
        done = 0
        for o in p0.outputs:
            producer = max(i for i, r, w in p0.touches() if w and r.virt == o.virt)
            if producer == len(p0.launches) - 1:
                continue
            p = copy.deepcopy(p0)
            rename(p, p.launches[-1][-1].virt, o.phys)
            assert "R3" in pc.rules(p), (p0.name, o.field)
            done += 1
        assert done, p0.name


def test_a_physical_stride_below_a_tenant_breaks_r4(golden_plans, topo_plans):
    for p0 in every_plan(golden_plans, topo_plans):
        for v, t in enumerate(p0.virts):
            if v not in p0.intervals():
                continue
            p = copy.deepcopy(p0)
            table = p.buf_spatial if t.spatial else p.buf_flat
            table[t.phys] = t.stride - 1
            found = pc.check(p)
            assert any(rule == "R4" and f"virtual {v} " in msg for rule, msg in found), (p0.name, v)
            assert "R5" in {rule for rule, _ in found} or max(81 * p.buf_spatial[t.phys], p.buf_flat[t.phys]) == max(81 * p0.buf_spatial[t.phys], p0.buf_flat[t.phys])
        also = [v for v, t in enumerate(p0.virts) if t.also_flat]
        for v in also:
            p = copy.deepcopy(p0)
            p.buf_flat[p.virts[v].phys] = p.virts[v].also_flat - 1
            assert "R4" in pc.rules(p), (p0.name, v)
    p = copy.deepcopy(topo_plans["fan_out"])  # a view past the end of its row
    seg = next(r for r in p.launches[9] if r.field == "seg")
    seg.offset = seg.stride - seg.C + 1
    assert pc.rules(p) == ["R4"]


def test_the_token_tensor_of_token_and_flat_has_an_also_flat_stride(topo_plans):
    p = topo_plans["token_and_flat"]
    also = [t for t in p.virts if t.also_flat]
    assert len(also) == 1 and also[0].spatial and also[0].also_flat == 81 * 16 and p.buf_flat[also[0].phys] >= 81 * 16


# ---- one topology per view field ----------------------------------------------------------------------------------------
def test_the_restated_allocation_keeps_the_rules(golden_plans, topo_plans):
    for p in every_plan(golden_plans, topo_plans):
        assert pc.check(pc.allocate(p)) == [], p.name


def test_every_view_field_has_a_topology_that_collides_without_it(nsg, topo_plans):
    covered = set()
    for name, p in topo_plans.items():
        topo = tm.build(nsg, name)
        for f in topo.fields:
            assert f in pc.fields(p), (name, f)
            assert "R1" in pc.rules(pc.allocate(p, ignore=f)), f"{name}: the allocation that ignores `{f}` does not collide"
            covered.add(f)
    assert set(FIELDS) <= covered, set(FIELDS) - covered
    assert covered & set(LINE_FIELDS)


def test_the_late_readers_come_more_than_three_launches_after_the_first_write(nsg, topo_plans):
    """Only the distance: that the launches in between are unrelated and that their outputs would take the tensor's
    buffer is what test_every_view_field_has_a_topology_that_collides_without_it shows."""
    for name, fields in (("long_skip", ["res"]), ("kv", ["attK", "attV"]), ("rtbias", ["rtBias"]), ("bmm", ["bmmB"]),
                         ("srcs", ["srcSame", "srcBoard", "srcRankLine"]), ("lines18", ["srcFileLine", "srcLine"])):
        p = topo_plans[name]
        for f in fields:
            gaps = [i - p.intervals()[r.virt][0] for i, r, w in p.touches() if r.field == f]
            assert gaps and max(gaps) > 3, (name, f, gaps)


def test_the_unrelated_launches_hold_a_gather_and_a_token_mix(topo_plans):
    """kLaunchTokenMix = 13 and kLaunchGather = 14 (onnx_graph.h), between the early operand and its late reader."""
    for name in ("early_heads", "token_and_flat", "kv", "rtbias", "bmm", "srcs", "lines18"):
        p = topo_plans[name]
        assert 13 in p.kinds[5:-1] and 14 in p.kinds[5:-1], (name, p.kinds)


# ---- what the device tests lean on ---------------------------------------------------------------------------------------
GOLDEN_REFS = {"net_att_pre": "net_att", "net_att_hybrid": "net_att", "net_graph_geom": "net_geom", "net_graph_math": "net_math",
               "net_graph_norm": "net_norm", "net_graph_pool": "net_pool", "net_graph_se": "net_graph", "net_graph_gpool93": "net_graph",
               "net_graph_softplus": "net_graph", "net_graph_views": "net_graph", "net_torch_2x64": "net_torch",
               "net_torch_bn_1x64": "net_torch", "net_torch_sigtanh_eps_1x64": "net_torch"}


def golden_case(nsg, golden_dir, name, n):
    """(model bytes, planes, bitboards [n], stored float64 outputs of those boards)."""
    planes = PLANES.get(name + ".onnx", 86)
    g = np.load(os.path.join(golden_dir, GOLDEN_REFS[name] + ".npz"))
    if GOLDEN_REFS[name] == "net_torch":
        bb, pol = g["bitboards"], g[name + "_policy"]
    else:
        bb = np.load(os.path.join(golden_dir, "net_graph.npz"))[f"bitboards{planes}"]
        pol = np.concatenate([np.load(os.path.join(golden_dir, f"{name}_policy_{h}.npz"))["policy"] for h in range(2)])
    with open(os.path.join(golden_dir, name + ".onnx"), "rb") as f:
        data = f.read()
    return data, planes, bb[:n], [pol[:n], g[name + "_value"][:n], g[name + "_draw"][:n]]


@pytest.mark.parametrize("name", sorted(GOLDEN_REFS))
def test_the_float64_interpreter_gives_the_stored_outputs(nsg, golden_dir, name):
    """The stored outputs are the torch modules' in float64; the file holds their float32 weights folded: 1e-6."""
    data, planes, bb, ref = golden_case(nsg, golden_dir, name, 4)
    x = nsg.synth.expand_reference(bb, True).reshape(-1, planes, 9, 9).astype(np.float64)
    for got, want in zip(onnx_ref64.outputs(nsg, data, x), ref):
        assert float(np.abs(got - want).max()) < 1e-6, name


def test_a_swapped_early_operand_moves_the_policy(nsg):
    bb = nsg.synth.random_batch(3, 86, seed=31)
    x = nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float64)
    seen = set()
    for name in tm.NAMES:
        topo = tm.build(nsg, name)
        ref = tm.reference(nsg, topo, x)
        assert float(ref[0].std()) > 1.0 and len(np.unique(ref[0])) >= 7, name
        if topo.exact:
            assert not topo.swaps
            continue
        for operand, models in topo.swaps.items():
            assert operand in topo.fields and models
            for data in models:
                moved = np.abs(tm.reference(nsg, topo, x, data)[0] - ref[0]).max(axis=1)
                assert float(moved.min()) > 1e-2, (name, operand, moved)  # on every board
            seen.add(operand)
    assert seen == {"attK", "attV", "rtBias"}
