"""`selfplay --decision-log`: every search decision of the self-play engine (csrc/selfplay), recomputed from
the numbers it read by tests/selfplay_ref.py, which restates the reference's formulas and knows nothing of
selfplay.cc.  CPU executors here; the HIP evaluator in test_gpu_selfplay_decisions.py."""
import dataclasses
import json
import os
import subprocess

import pytest

import selfplay_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SP = os.path.join(ROOT, "nshogi-engine_amd", "csrc", "selfplay")


def _tool(name):
    path = os.path.join(SP, name)
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def selfplay(*args, timeout=120):
    r = subprocess.run([_tool("selfplay")] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


COMMON = ["--threads", "1", "--dfpn-nodes", "2000"]
ALPHAZERO = ["--playouts", "48", "--full-search-ratio", "0.75", "--games-per-group", "2", "--max-games", "4",
             "--decision-log-every", "16"]
GUMBEL = ["--gumbel", "1", "--playouts", "32", "--full-search-ratio", "0.5", "--games-per-group", "2", "--max-games", "3"]
# name -> options.  The AlphaZero-mode runs are sized by the 10**3 noisy roots asked of them, which is some
# 3 * 10**5 selections: they record every 16th; the Gumbel runs and `small` record every one.
RUNS = {
    "alphazero-hash": ["--executor", "hash", "--seed", "3"] + ALPHAZERO,
    "alphazero-random": ["--executor", "random", "--seed", "4"] + ALPHAZERO,
    "gumbel16-hash": ["--executor", "hash", "--seed", "3", "--num-sampling-moves", "16"] + GUMBEL,
    "gumbel16-random": ["--executor", "random", "--seed", "4", "--num-sampling-moves", "16"] + GUMBEL,
    "gumbel4-hash": ["--executor", "hash", "--seed", "5", "--num-sampling-moves", "4"] + GUMBEL,
    "gumbel4-random": ["--executor", "random", "--seed", "6", "--num-sampling-moves", "4"] + GUMBEL,
    "small": ["--executor", "hash", "--seed", "3", "--playouts", "48", "--full-search-ratio", "0.5",
              "--games-per-group", "1", "--max-games", "1"],
}
CHECKED = [r for r in RUNS if r != "small"]


class Runs:
    """Each run is made once, and checked against the reference's rules once."""

    def __init__(self, tmp):
        self.tmp, self.done, self.reports = tmp, {}, {}

    def run(self, name):
        if name not in self.done:
            log = self.tmp / f"{name}.decisions"
            self.done[name] = (selfplay(*COMMON, *RUNS[name], "--decision-log", log), log)
        return self.done[name]

    def report(self, name):
        if name not in self.reports:
            self.reports[name] = ref.check_log(self.run(name)[1])
        return self.reports[name]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("decisions"))


@pytest.mark.parametrize("name", CHECKED + ["small"])
def test_every_record_recomputes(runs, name):
    out, _ = runs.run(name)
    rep = runs.report(name)
    print(name, rep.counts, "noisy", rep.noisy_evaluations, "ties", rep.ties, "softmax", rep.softmax_worst)
    assert rep.disagreements == 0, rep.examples
    assert rep.softmax_worst > 0  # the softmax was really compared
    # every transition: one per move played, but for the mating moves the df-pn solver plays itself
    assert rep.counts["transition"] == out["moves"] - out["dfpn_mates"] > 0


def test_the_runs_cover_what_they_should(runs):
    reps = [runs.report(n) for n in CHECKED]
    total = lambda kind: sum(r.counts.get(kind, 0) for r in reps)
    noisy, ties = sum(r.noisy_evaluations for r in reps), sum(r.ties for r in reps)
    print({k: total(k) for k in ("select", "gumbel-select", "evaluation", "sample", "halve", "transition")},
          "noisy", noisy, "ties", ties)
    assert total("select") >= 2 * 10 ** 4
    assert noisy >= 10 ** 3
    assert total("halve") >= 200
    # both kinds of root in AlphaZero mode: evaluations of a root with the mix and without it
    assert all(0 < runs.report(n).noisy_evaluations < runs.report(n).counts["transition"] for n in CHECKED[:2])
    # exact ties at a partial_sort cut: either survivor set passes, so they must be rare
    assert ties * 1000 < total("halve") + total("sample")


# fault -> (the rule changed, the log it must show on, the record types it can show in)
FAULTS = {
    "1.2 for 1.25": (dict(c_puct=1.2), "small", ("select",)),
    # C * P / (1 + n) alone is C * P at n = 0, bit for bit, and cannot show (0 disagreements of 39 012 selections):
    # the fault is the whole visited-child expression for the unvisited too, whose win rate is 0 / 0 (6 019)
    "C*P/(1+n) for unvisited children too": (dict(unvisited_as_visited=True), "small", ("select",)),
    "blend with draw and win swapped": (dict(swap_blend=True), "small", ("select",)),
    "noise weight 0.3": (dict(noise_weight=0.3), "small", ("evaluation",)),
    "mix on Gumbel roots": (dict(mix_on_gumbel_root=True), "gumbel16-hash", ("evaluation",)),
    "NumSort >> HalvingCount without the + 1": (dict(keep_plus_one=False), "gumbel16-hash", ("halve",)),
    "no minimum of 2 survivors": (dict(keep_at_least_two=False), "gumbel4-hash", ("halve",)),
    "Q transform without the 50": (dict(c_visit=0.0), "gumbel16-hash", ("halve", "transition")),
    "final pick by prior alone": (dict(final_by_prior=True), "small", ("transition",)),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_the_checker_sees_a_wrong_formula(runs, fault):
    """The checker is worth what it can catch: with one of the reference's rules changed it must disagree with
    the same log that checks clean under the reference's."""
    change, name, kinds = FAULTS[fault]
    assert runs.report(name).disagreements == 0
    rep = ref.check_log(runs.run(name)[1], dataclasses.replace(ref.REFERENCE, **change), kinds=kinds)
    print(fault, rep.disagreements, "of", rep.counts)
    assert rep.disagreements > 0


UNCHANGED = ("digest", "moves", "games_finished", "black", "white", "draw", "teacher_records", "mates_found", "dfpn_mates")


@pytest.mark.parametrize("mode", [["--gumbel", "0"], ["--gumbel", "1", "--num-sampling-moves", "4"]])
def test_logging_changes_no_result(tmp_path, mode):
    base = COMMON + ["--executor", "hash", "--seed", "8", "--playouts", "32", "--full-search-ratio", "0.5",
                     "--games-per-group", "2", "--max-games", "2"] + mode
    outs, games = [], []
    for i, extra in enumerate(([], ["--decision-log", tmp_path / "d1"],
                               ["--decision-log", tmp_path / "d7", "--decision-log-every", "7"])):
        outs.append(selfplay(*base, *extra, "--game-log", tmp_path / f"g{i}", "--teacher", tmp_path / f"t{i}"))
        games.append(open(tmp_path / f"g{i}").read())
    assert games[0] == games[1] == games[2] and games[0]
    for key in UNCHANGED:
        assert outs[0][key] == outs[1][key] == outs[2][key], key
    assert open(tmp_path / "t0", "rb").read() == open(tmp_path / "t1", "rb").read()
    assert ref.check_log(tmp_path / "d7").disagreements == 0
    # every 7th selection of each game, counted per game; every record of the other types
    every, seventh = ref.records_by_game(tmp_path / "d1"), ref.records_by_game(tmp_path / "d7")
    assert set(every) == set(seventh)
    is_selection = lambda line: line.startswith(("select ", "gumbel-select "))
    for game in every:
        assert [x for x in every[game] if is_selection(x)][::7] == [x for x in seventh[game] if is_selection(x)]
        assert [x for x in every[game] if not is_selection(x)] == [x for x in seventh[game] if not is_selection(x)]


def test_several_workers_write_the_same_records(tmp_path):
    """Three host workers advancing 14 game slots: each slot buffers its own records, so every game's records
    are the ones, in the order, of the one-worker run.  (No evaluation cache: it is keyed by the position alone,
    and which game stores a position first depends on the threads.)"""
    base = COMMON + ["--executor", "hash", "--seed", "6", "--playouts", "16", "--games-per-group", "7", "--max-games", "3",
                     "--evaluation-cache-memory-size", "0", "--decision-log-every", "4"]
    logs, finished = [], []
    for workers in (1, 3):
        selfplay(*base, "--workers", workers, "--decision-log", tmp_path / f"d{workers}", "--game-log", tmp_path / f"g{workers}")
        assert ref.check_log(tmp_path / f"d{workers}").disagreements == 0
        logs.append(ref.records_by_game(tmp_path / f"d{workers}"))
        finished.append({int(line.split()[0]) for line in open(tmp_path / f"g{workers}")})
    both = finished[0] & finished[1]
    assert len(both) >= 3
    for game in both:
        assert logs[0][game] == logs[1][game], game
    # the games still going when a run stops: one run's records are the other's, as far as they go
    for game in set(logs[0]) & set(logs[1]):
        a, b = logs[0][game], logs[1][game]
        n = min(len(a), len(b))
        assert n and a[:n] == b[:n], game
