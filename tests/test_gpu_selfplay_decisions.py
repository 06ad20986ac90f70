"""`selfplay --decision-log` with the HIP evaluator: the search decisions recompute (tests/selfplay_ref.py)
also when the logits and values they read come from the network on the GPU, not from a stand-in executor."""
import json
import os
import subprocess

import pytest

import selfplay_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFPLAY = os.path.join(ROOT, "nshogi-engine_amd", "csrc", "selfplay", "selfplay")

# Every 8th selection of a game is recorded (the other record types always are): the AlphaZero-mode log of this
# run is 62 MB with every 4th -- the network's games are long -- against the 64 MB a log may have here.
EVERY = 8


@pytest.mark.gpu
@pytest.mark.parametrize("gumbel", [0, 1])
def test_hip_selfplay_decisions_recompute(nsg, tmp_path, gumbel):
    """The 2-block 64-channel random net of the HIP self-play tests (test_shogi_core.py)."""
    weights, log = tmp_path / "net.nsgw", tmp_path / "decisions"
    nsg.weights.save(str(weights), nsg.weights.make_random(2, 64, seed=3, bn="random"))
    r = subprocess.run([SELFPLAY, "--executor", "hip", "--weights", str(weights), "--playouts", "24", "--max-games", "4",
                        "--seed", "9", "--threads", "1", "--games-per-group", "6", "--gumbel", str(gumbel),
                        "--decision-log", str(log), "--decision-log-every", str(EVERY)],
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout)
    assert out["games_finished"] >= 4
    size = os.path.getsize(log)
    rep = ref.check_log(log)
    print("gumbel", gumbel, "K", EVERY, "bytes", size, rep.counts, "noisy", rep.noisy_evaluations, "ties", rep.ties,
          "softmax worst", rep.softmax_worst, "of the bound; non-uniform", rep.nonuniform_evaluations)
    assert rep.disagreements == 0, rep.examples
    assert size < 64 * 2 ** 20
    assert rep.nonuniform_evaluations > 0  # the network really fed the search
    assert rep.counts["transition"] == out["moves"] - out["dfpn_mates"] > 0
    if gumbel:  # (24 playouts over 16 sampled moves never reach below the root's children: no select records)
        assert rep.counts["halve"] > 0 and rep.counts["sample"] > 0 and rep.counts["gumbel-select"] > 0
    else:
        assert rep.counts["select"] > 0 and rep.noisy_evaluations > 0
