"""The conv epilogue's instruction trims change no output bit: every launch plan that runs the staged
epilogue (cooperative K split, one- and two-board persistent tiles, per-layer kernels with a partial last
tile, the f16m8 partner that shares the staging code) and the team trunk (untouched) against arrays the
library of the commit BEFORE the trims produced for the same seeded inputs (tests/golden/epilogue_r05/).

Per case the fixtures hold win and draw of every board (float32), the policy of four boards (float32: first
board, second board of the first tile, a middle one, the last) and a 64-bit digest of the policy BITS of every
board, so that all three outputs are compared bit for bit on every board at a few hundred KB in total.
Written once, on the GPU, with the parent build:  NSG_LIB=<parent libnsg.so> python tests/test_epilogue_bits_r05.py <dir>
"""
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "epilogue_r05")
PER_LAYER = {"NSG_TRUNK_KERNEL": "0", "NSG_COOP_TRUNK": "0"}

# launch kinds: (Evaluator.last_launch_kind()[0], Evaluator.last_launch_form()["whole_trunk"])
TEAM, COOP, WHOLE_TRUNK, ONE_PER_LAYER = ("team", 0), ("coop", 0), ("per_layer", 1), ("per_layer", 0)

# (name, precision, blocks, channels, boards, environment of the golden run, the launch kind the case is about,
#  compare with the per-layer kernels too)
CASES = [
    ("m6_b1", "f16m6", 2, 256, 1, {}, TEAM, False),       # team trunk (its own arithmetic: no per-layer partner)
    ("m6_b17", "f16m6", 2, 256, 17, {}, COOP, True),      # cooperative K split, two row groups
    ("m6_b33", "f16m6", 2, 256, 33, {}, COOP, True),      # cooperative K split
    ("m6_b144", "f16m6", 2, 256, 144, {}, WHOLE_TRUNK, True),    # one-board persistent tiles, edge rows
    ("m6_b384", "f16m6", 2, 256, 384, {}, WHOLE_TRUNK, True),    # two-board persistent tiles
    ("m6_b385_per_layer", "f16m6", 2, 256, 385, dict(PER_LAYER, NSG_SPLIT_BATCH="0"), ONE_PER_LAYER, False),  # a partial last tile
    ("m6_192ch_b17", "f16m6", 2, 192, 17, {}, COOP, True),
    ("m8_b17", "f16m8", 2, 256, 17, {}, ONE_PER_LAYER, False),
    ("m8_b384", "f16m8", 2, 256, 384, {"NSG_TRUNK_KERNEL": "1"}, WHOLE_TRUNK, True),  # (persistent launch: opt-in for f16m8)
]
_ENV_KEYS = ("NSG_TRUNK_KERNEL", "NSG_COOP_TRUNK", "NSG_SPLIT_BATCH")


def sample_boards(n):
    return sorted({0, min(1, n - 1), n // 2, n - 1})


def policy_digest(p):
    """One uint64 per board over the policy's bit patterns (position-dependent odd multipliers, wrap-around sum)."""
    bits = np.ascontiguousarray(p, dtype=np.float32).view(np.uint32).astype(np.uint64)
    mult = (np.arange(bits.shape[1], dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1)
    with np.errstate(over="ignore"):
        return (bits * mult[None, :]).sum(axis=1, dtype=np.uint64)


def run_case(nsg, precision, blocks, channels, boards, env):
    """(policy, win, draw, plan, launch kind) of one seeded net on one seeded batch under `env` (set for the evaluator's lifetime)."""
    old = {k: os.environ.get(k) for k in _ENV_KEYS}
    try:
        for k in _ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        w = nsg.weights.make_random(blocks, channels, seed=500 + channels, bn="random")
        ev = nsg.Evaluator(0, boards, 86, precision=precision)
        ev.load_memory(nsg.weights.to_blob(w))
        bb = nsg.synth.random_batch(boards, 86, seed=1000 + boards)
        p, v, d = ev.compute_blocking(bb)
        plan = ev.last_plan()
        kind = (ev.last_launch_kind()[0], ev.last_launch_form()["whole_trunk"])
        ev.close()
    finally:
        for k, val in old.items():
            os.environ.pop(k, None)
            if val is not None:
                os.environ[k] = val
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float32)).reshape(boards, -1)
    return f32(p), f32(v), f32(d), plan, kind


@pytest.mark.parametrize("name,precision,blocks,channels,boards,env,want_kind,per_layer", CASES, ids=[c[0] for c in CASES])
def test_outputs_bit_identical_to_parent_build(nsg, name, precision, blocks, channels, boards, env, want_kind, per_layer):
    p, v, d, plan, kind = run_case(nsg, precision, blocks, channels, boards, env)
    assert kind == want_kind, (kind, plan)  # the launch this case is about
    g = lambda what: np.load(os.path.join(GOLDEN, f"{name}_{what}.npy"))
    assert plan["trunk_precision"] == str(g("plan")[0]), plan  # the plan the fixture was recorded under
    np.testing.assert_array_equal(v.view(np.uint32), g("win").view(np.uint32))
    np.testing.assert_array_equal(d.view(np.uint32), g("draw").view(np.uint32))
    np.testing.assert_array_equal(p[sample_boards(boards)].view(np.uint32), g("policy").view(np.uint32))
    np.testing.assert_array_equal(policy_digest(p), g("policy_digest"))
    if per_layer:  # the persistent / cooperative launch against one launch per layer, same process
        # (one plan for the whole batch: left to itself a per-layer 144-board batch runs as 128 K-split boards + the rest,
        # another summation order)
        p1, v1, d1, plan1, kind1 = run_case(nsg, precision, blocks, channels, boards, dict(env, NSG_SPLIT_BATCH="0", **PER_LAYER))
        assert kind1 == ONE_PER_LAYER, (kind1, plan1)
        same = ("fragments_per_wave", "k_split", "trunk_precision")
        assert [plan[k] for k in same] == [plan1[k] for k in same], (plan, plan1)  # the same split of K, hence the same sums
        np.testing.assert_array_equal(p.view(np.uint32), p1.view(np.uint32))
        np.testing.assert_array_equal(v.view(np.uint32), v1.view(np.uint32))
        np.testing.assert_array_equal(d.view(np.uint32), d1.view(np.uint32))


if __name__ == "__main__":  # writes the fixtures (run with the parent build's library)
    sys.path.insert(0, os.path.dirname(HERE))
    out = sys.argv[1]
    os.makedirs(out, exist_ok=True)
    nsg_ = importlib.import_module("nshogi-engine_amd")
    for name, precision, blocks, channels, boards, env, want_kind, _ in CASES:
        p, v, d, plan, kind = run_case(nsg_, precision, blocks, channels, boards, env)
        assert kind == want_kind, (name, kind, plan)
        np.save(os.path.join(out, f"{name}_win.npy"), v)
        np.save(os.path.join(out, f"{name}_draw.npy"), d)
        np.save(os.path.join(out, f"{name}_policy.npy"), p[sample_boards(boards)])
        np.save(os.path.join(out, f"{name}_policy_digest.npy"), policy_digest(p))
        np.save(os.path.join(out, f"{name}_plan.npy"), np.array([plan["trunk_precision"]]))
        print(name, plan, flush=True)
