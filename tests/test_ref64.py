"""The float64 reference of the plan sweep (tests/ref64.py), pinned on the CPU: against the committed golden fixture,
against the C oracle on feature planes of random (garbage-bit) bitboards and real positions, and a self-test of the
localisation check -- rounding noise passes it, a planted mutant that the absolute tolerance lets through does not.

Measured here: ref64 and the oracle (which stores float32 between layers) agree to 2-5e-7 on trunk and policy and
to 1e-8...6e-8 on value and draw."""
import numpy as np
import pytest
import torch

import ref64

ORACLE_TOL = 1e-5
# the absolute tolerances of the fp16 and bf16 rows (test_gpu_evaluator.py, test_gpu_plan_sweep.py)
ABS_TOL = {"fp16": 2e-2, "bf16": 1.5e-1}


def _inputs(nsg, n, seed):
    """n random bitboards with garbage bits, then n positions of real games."""
    return np.ascontiguousarray(np.concatenate([nsg.synth.random_batch(n, 86, seed=seed, garbage=True),
                                                nsg.positions.game_positions(n, seed=seed + 2)]))


def test_ref64_matches_golden(nsg, oracle, golden_dir):
    g = np.load(f"{golden_dir}/net_tiny.npz")
    w = nsg.weights.make_random(int(g["blocks"]), int(g["channels"]), seed=int(g["weights_seed"]), bn="random")
    r = ref64.forward(w, oracle.extract_bits(g["bitboards"]))
    np.testing.assert_allclose(r["policy"], g["policy"], rtol=0, atol=ORACLE_TOL)
    np.testing.assert_allclose(r["value"], g["value"], rtol=0, atol=ORACLE_TOL)
    np.testing.assert_allclose(r["draw"], g["draw"], rtol=0, atol=ORACLE_TOL)


@pytest.mark.parametrize("blocks,channels,bn", [(1, 64, "identity"), (2, 128, "random"), (2, 192, "identity"),
                                                (1, 384, "identity")])
def test_ref64_matches_oracle(nsg, oracle, blocks, channels, bn):
    w = nsg.weights.make_random(blocks, channels, seed=100 * blocks + channels, bn=bn)
    bb = _inputs(nsg, 3, seed=blocks + channels)
    planes = oracle.extract_bits(bb)
    p, v, d, t = oracle.net(nsg.weights.to_blob(w)).forward_planes(planes, want_trunk=True)
    r = ref64.forward(w, planes)
    err = {k: float(np.abs(a - r[k]).max()) for k, a in (("trunk", t), ("policy", p), ("value", v), ("draw", d))}
    print(f"{blocks}x{channels} bn={bn}: ref64 vs oracle {err}")
    assert max(err.values()) <= ORACLE_TOL, err
    # boards are independent: a slice of the batch's reference is the reference of the slice (to float64 rounding:
    # the matrix products block differently by batch size)
    s = ref64.forward(w, planes[2:4])
    for k in r:
        np.testing.assert_allclose(ref64.take(r, slice(2, 4))[k], s[k], rtol=0, atol=1e-12)


# Planted mutants: the contribution of ONE tap of ONE corner square is dropped from the 16 output channels of ONE
# fragment of ONE board (board 1: a real position) in one trunk layer -- a kernel that mis-indexes a corner's halo
# would do that.  Each is small enough for the absolute tolerance of its precision's row.
# (precision, layer, (row, column), (ky, kx), fragment)
MUTANTS = [
    ("fp16", 3, (8, 0), (0, 2), 7),
    ("bf16", 4, (0, 8), (2, 0), 7),
]


@pytest.fixture(scope="module")
def mutant_net(nsg, oracle):
    w = nsg.weights.make_random(2, 256, seed=11, bn="random")
    bb = np.ascontiguousarray(np.concatenate([nsg.synth.random_batch(1, 86, seed=5, garbage=True),
                                              nsg.positions.game_positions(1, seed=7)]))
    planes = oracle.extract_bits(bb)
    return w, planes, ref64.forward(w, planes)


def _abs_errors(r, ref):
    tmax = max(1.0, float(np.abs(ref["trunk"]).max()))
    out = max(float(np.abs(r[k] - ref[k]).max()) for k in ("policy", "value", "draw"))
    return out, float(np.abs(r["trunk"] - ref["trunk"]).max()) / tmax


@pytest.mark.parametrize("precision,layer,square,tap,frag", MUTANTS)
def test_localisation_accepts_rounding_and_rejects_a_dropped_tap(mutant_net, precision, layer, square, tap, frag):
    w, planes, ref = mutant_net
    dtype = {"fp16": torch.float16, "bf16": torch.bfloat16}[precision]
    tol = ABS_TOL[precision]

    # rounding every layer's activations to the row's type: within the tolerance, and evenly spread
    noisy = ref64.forward(w, planes, round_to=dtype)
    loc = ref64.localisation(noisy["trunk"], ref["trunk"])
    assert max(_abs_errors(noisy, ref)) < tol
    assert not ref64.localisation_failures(loc, precision), ref64.localisation_ratios(loc)

    def drop_tap(lay, xp, taps, acc):
        if lay == layer:
            (y, x), (ky, kx), c = square, tap, slice(16 * frag, 16 * frag + 16)
            acc[1, y, x, c] -= xp[1, y + ky, x + kx, :] @ taps[ky, kx][:, c]

    bad = ref64.forward(w, planes, round_to=dtype, hook=drop_tap)
    out_err, trunk_err = _abs_errors(bad, ref)
    ratios = ref64.localisation_ratios(ref64.localisation(bad["trunk"], ref["trunk"]))
    print(f"{precision}: mutant max|err| outputs {out_err:.3e}, trunk {trunk_err:.3e} x max|t|; ratios {ratios}")
    # the old check lets it through ...
    assert out_err < tol and trunk_err < tol
    # ... the localisation check does not
    assert ref64.localisation_failures(ref64.localisation(bad["trunk"], ref["trunk"]), precision), ratios
