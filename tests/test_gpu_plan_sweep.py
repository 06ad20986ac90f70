"""Every board of every launch plan against the float64 reference (tests/ref64.py).

On one device the evaluator picks among some fifteen launch forms by batch size, channel count, precision and CU
count: chooseLaunchForm in csrc/launch_form.cc (with planForBatch and chooseConvPlan), whose decisions
tests/golden/launch_forms.txt tabulates on the CPU.  Each row of the matrix below is ONE evaluator run through batch sizes
derived from info()["compute_units"] -- n - 1, n, n + 1 of every threshold of those functions -- ascending, then
descending, as the engine's varying batches would.  Before every forward of the ascending pass the test reads what
chooseLaunchForm says of the batch (Evaluator.launch_form), and what the forward then reports must be exactly that: the
table is what the device runs.  Every forward of that pass is checked board by board against ref64 (policy, value, draw, and the trunk), with the
localisation check on top of the absolute tolerance; the descending pass and a forward with the boards in reversed
slots must be bit-identical to it (two-part batches, whose parts run different plans: within the tolerance).  Each
row then asserts that every launch form FORMS says it can reach was reached, and that no persistent launch gave up.
The input is random bitboards with garbage bits in the even slots and positions of real games in the odd ones."""
import hashlib
import math

import numpy as np
import pytest

import ref64

pytestmark = pytest.mark.gpu

TOL = {"fp32": 2e-4, "f16x3": 2e-4, "f16m8": 1e-3, "f16m6": 1e-3, "fp16": 2e-2, "bf16": 1.5e-1}
TEAM_MAX = 16  # nsg::kTeamMaxBoards


def _thresholds(cus, F, kind):
    """The batch sizes at which some launch decision changes, for a device of `cus` compute units."""
    t = set()
    if kind in ("full", "team"):
        nj = F // 16
        t |= {TEAM_MAX} | {cus // (nj * rg) for rg in (6, 3, 2, 1)}            # team trunk, its row groups
    if kind == "full":
        t |= {cus // 24, cus // 12, cus // 8, cus // 4}                           # K4 row splits, K4
        t |= {cus // 2}                                                            # K2 window, four-wave heads
        if F == 192:
            t |= {cus // 3, cus // 6, cus // 9, cus // 18}                        # the 192-channel K3 plans
        t |= {cus // 2 + 3 * cus // 16}                                            # first two-part range
        t |= {math.ceil(9 * cus / 16), cus}                                        # one-board whole trunk
        t |= {cus + cus // 2, 2 * cus}                                             # two-part, two-board whole trunk
        t |= {2 * cus + cus // 4}                                                  # two-part above 2 CUs boards
        if F == 256:
            t |= {4 * cus}                                                         # BASELINE configs[4]: chains
    if kind in ("full", "conv"):
        for nf in (4, 2, 1):                                                       # chooseConvPlan: waves cover 3/4
            per = F // (16 * nf)                                                   # of the SIMDs, 2 / 1 boards
            for nb in (2, 1):
                t.add(nb * math.ceil(3 * cus / per))
        t |= {cus // 2, cus}                                                       # the one-round rule
    return t


def _sizes(cus, F, kind, top):
    if kind == "short":
        s = {1, cus // 16, cus // 16 + 1, cus // 4, cus // 4 + 1, cus // 2, cus // 2 + 1, cus, cus + 1, 2 * cus}
    elif kind == "few":
        s = {1, 7, cus // 4 + 1, cus + 3}
    elif kind == "handful":
        s = {1, TEAM_MAX, cus // 4 + 1, cus // 2 + 1, cus, 2 * cus + 1}
    else:
        s = {m for n in _thresholds(cus, F, kind) for m in (n - 1, n, n + 1)} | {1}
    return sorted(b for b in s if 1 <= b <= top)


# ---- launch forms: name -> (the condition of chooseLaunchForm / planForBatch in launch_form.cc that selects it, reachable(row, cus))
def _mx(r):
    return r["prec"] in ("f16m8", "f16m6")


FORMS = {
    "team trunk": ("chooseLaunchForm: Team, teamAvailable and teamMembers > 0 -- MX or f16x3, 192/256 channels, B <= kTeamMaxBoards "
                   "and B x F/16 x row groups <= CUs",
                   lambda r, cus: (_mx(r) or r["prec"] == "f16x3") and r["F"] in (192, 256) and not _off(r, "TEAM")),
    "coop K2": ("chooseLaunchForm: Coop, coopAvailable && canRunCoopTrunk (f16m6, 256 ch.) && coopFits, on planForBatch's K2 "
                "window (CUs/4 < B <= CUs/2)",
                lambda r, cus: r["prec"] == "f16m6" and r["F"] == 256 and r["kind"] == "full"),
    "coop K4 x1": ("... planForBatch's four-way K split (B x 4 <= CUs), one row group",
                   lambda r, cus: r["prec"] == "f16m6" and r["F"] == 256 and not _off(r, "COOP")),
    "coop K4 x2": ("... two row groups (B x 8 <= CUs); with the cooperative trunk three row groups give way to two",
                   lambda r, cus: r["prec"] == "f16m6" and r["F"] == 256 and not _off(r, "COOP") and cus // 8 > 1),
    "coop K4 x3": ("NOT CHOSEN BY DEFAULT: 256 channels take the cooperative trunk up to 8 members per board only "
                   "(coopMembers <= 8 in chooseLaunchForm); NSG_COOP_TRUNK=1 forces it", lambda r, cus: False),
    "coop K4 x6": ("NOT CHOSEN BY DEFAULT: 24 members per board, as coop K4 x3", lambda r, cus: False),
    "coop K3 x1": ("chooseLaunchForm: Coop, 192 channels, planForBatch's three-way K split (B x 3 <= CUs), one row group, "
                   "coopFits (ceil(B / 8) x 3 members <= CUs / 8)",
                   lambda r, cus: r["prec"] == "f16m6" and r["F"] == 192 and r["kind"] == "full"),
    "coop K3 x2": ("... two row groups (B x 6 <= CUs), 6 members",
                   lambda r, cus: r["prec"] == "f16m6" and r["F"] == 192 and r["kind"] == "full"),
    "coop K3 x3": ("... three row groups (B x 9 <= CUs), 9 members",
                   lambda r, cus: r["prec"] == "f16m6" and r["F"] == 192 and r["kind"] == "full" and
                   cus // 9 > TEAM_MAX),
    "coop K3 x6": ("... six row groups (B x 18 <= CUs), 18 members: below the team trunk's sizes unless it is off",
                   lambda r, cus: r["prec"] == "f16m6" and r["F"] == 192 and _off(r, "TEAM") and cus >= 18),
    "per-layer K3 x1": ("planForBatch: the 192-channel K3 plans where coopFits fails (per-layer launches)",
                        lambda r, cus: r["prec"] == "f16m6" and r["F"] == 192 and r["kind"] == "full"),
    "per-layer K3 x2": ("... two row groups", lambda r, cus: r["prec"] == "f16m6" and r["F"] == 192 and
                        r["kind"] == "full"),
    "per-layer K3 x3": ("... three row groups", lambda r, cus: r["prec"] == "f16m6" and r["F"] == 192 and
                        r["kind"] == "full" and cus // 9 > TEAM_MAX),
    "per-layer K4 x1": ("planForBatch: the four-way K split on per-layer launches (f16m8, or NSG_COOP_TRUNK=0)",
                        lambda r, cus: _mx(r) and r["F"] == 256 and (r["prec"] == "f16m8" or _off(r, "COOP"))),
    "per-layer K4 x2": ("... two row groups", lambda r, cus: _mx(r) and r["F"] == 256 and
                        (r["prec"] == "f16m8" or _off(r, "COOP"))),
    "per-layer K4 x3": ("... three row groups (B x 12 <= CUs)",
                        lambda r, cus: _mx(r) and r["F"] == 256 and (r["prec"] == "f16m8" or _off(r, "COOP")) and
                        (_off(r, "TEAM") or cus // 12 > TEAM_MAX)),
    "per-layer K4 x6": ("... six row groups (B x 24 <= CUs): below the team trunk's sizes unless it is off",
                        lambda r, cus: _mx(r) and r["F"] == 256 and _off(r, "TEAM") and cus >= 24),
    "per-layer K2": ("planForBatch: the K2 window on per-layer launches (f16m8; 128 channels)",
                     lambda r, cus: (r["prec"] == "f16m8" and r["F"] == 256 and r["kind"] == "full") or
                     (_mx(r) and r["F"] == 128 and r["kind"] == "short")),
    "whole trunk nb1": ("chooseLaunchForm: WholeTrunk -- f16m6, canRunTrunk, one-board tiles, 9/16 CUs <= B <= CUs",
                        lambda r, cus: r["prec"] == "f16m6" and r["F"] in (192, 256) and r["kind"] == "full"),
    "whole trunk nb2": ("... two-board tiles, 3/4 CUs <= tiles <= CUs",
                        lambda r, cus: r["prec"] == "f16m6" and r["F"] in (192, 256) and r["kind"] == "full"),
    "two-part batch": ("chooseLaunchForm: Parts -- MX, 256 ch., not trunkKernel, CUs/2 < B <= CUs/2 + 3 CUs/16, "
                       "CUs < B < 3/2 CUs, or 2 CUs < B <= 9/4 CUs",
                       lambda r, cus: _mx(r) and r["F"] == 256 and r["kind"] == "full"),
    "half-batch chains": ("chooseLaunchForm: Chains -- two-board plan with more tiles than CUs, no two-part split",
                          lambda r, cus: (r["F"] in (192, 256) and r["kind"] == "full") or r["kind"] == "handful" or
                          (r["F"] == 384 and r["kind"] == "conv")),
    "tiles nfrag 1": ("chooseConvPlan: one fragment per wave, two-board tiles",
                      lambda r, cus: r["kind"] == "conv"),
    "tiles nfrag 2": ("chooseConvPlan: two fragments per wave (or one-board, one-fragment tiles as two row groups)",
                      lambda r, cus: not _mx(r) and r["kind"] in ("conv", "few", "handful")),
    "tiles nfrag 4": ("chooseConvPlan: full tiles (waves cover 3/4 of the SIMDs)",
                      lambda r, cus: r["kind"] in ("conv", "short", "handful") or
                      (r["kind"] == "full" and not (r["prec"] == "f16m6" and r["F"] == 256))),
    "f16x3 fallback of MX": ("chooseLaunchForm: trunkPrec -- an f16m8 / f16m6 evaluator whose plan has no MX form "
                             "(plan.nfrag != 4) runs the f16x3 copy of its trunk",
                             lambda r, cus: _mx(r) and r["kind"] in ("full", "short")),
}


def _off(r, what):
    return r["env"].get(f"NSG_{what}_TRUNK") == "0"


def form_of(prec, kind, form, plan):
    k, rows = plan["k_split"], plan["row_split"]
    if kind == "team":
        return "team trunk"
    if kind == "coop":
        return f"coop K{k}" + (f" x{rows}" if k in (3, 4) else "")
    if form["whole_trunk"]:
        return f"whole trunk nb{plan['boards_per_group']}"
    if form["parts"]:
        return "two-part batch"
    if plan["chains"] > 1:
        return "half-batch chains"
    if prec in ("f16m8", "f16m6") and plan["trunk_precision"] == "f16x3":
        return "f16x3 fallback of MX"
    if k > 1:
        return f"per-layer K{k}" + (f" x{rows}" if k in (3, 4) else "")
    return f"tiles nfrag {plan['fragments_per_wave']}"


# precision, channels, sizes, NSG_* environment (only where a form cannot be reached by default)
ROWS = [
    ("f16m6", 256, "full", {}),
    ("f16m6", 192, "full", {}),
    ("f16m6", 256, "team", {"NSG_TEAM_TRUNK": "0"}),
    ("f16m6", 256, "team", {"NSG_TEAM_TRUNK": "0", "NSG_COOP_TRUNK": "0"}),
    ("f16m6", 192, "team", {"NSG_TEAM_TRUNK": "0"}),
    ("f16m6", 384, "short", {}),
    ("f16m6", 128, "short", {}),
    ("f16m8", 256, "full", {}),
    ("f16m8", 256, "team", {"NSG_TEAM_TRUNK": "0"}),
    ("f16m8", 384, "short", {}),
    ("f16x3", 256, "conv", {}),
    ("f16x3", 192, "conv", {}),
    ("f16x3", 384, "conv", {}),
    ("fp32", 256, "conv", {}),
    ("fp32", 64, "few", {}),
    ("fp16", 256, "handful", {}),
    ("bf16", 256, "handful", {}),
]

_REPORT = []


def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def pool(nsg):
    """Inputs: slot 2i a random bitboard with garbage bits, slot 2i + 1 a position of a real game."""
    cache = {}

    def get(n):
        if n not in cache:
            half = (n + 1) // 2
            bb = np.empty((2 * half, 86, 2), dtype=np.uint64)
            bb[0::2] = nsg.synth.random_batch(half, 86, seed=4242, garbage=True)
            bb[1::2] = nsg.positions.game_positions(half, seed=4343)
            cache[n] = np.ascontiguousarray(bb[:n])
        return cache[n]
    return get


def _reference(nsg, oracle, blocks, F, pool, top):
    w = nsg.weights.make_random(blocks, F, seed=blocks * 1000 + F, bn="random")
    ref = ref64.cached(("sweep", blocks, F, top), w, oracle.extract_bits(pool(top)))
    return w, ref


def _check(ev, prec, n, bb, ref, stats):
    """One forward of boards bb[:n] checked against ref64; returns (digest, outputs)."""
    p, v, d = ev.compute_blocking(bb[:n])
    t = ev.download_trunk(n)
    r = ref64.take(ref, slice(0, n))
    tol = TOL[prec]
    err = max(float(np.abs(p - r["policy"]).max()), float(np.abs(v - r["value"]).max()),
              float(np.abs(d - r["draw"]).max()))
    terr = float(np.abs(t - r["trunk"]).max())
    tbound = tol * max(1.0, float(np.abs(r["trunk"]).max()))
    assert np.isfinite(p).all() and np.isfinite(t).all(), f"B={n}: non-finite output"
    assert err <= tol, f"B={n}: max|err| {err:.3e} > {tol} ({ev.last_plan()})"
    assert terr <= tbound, f"B={n}: trunk max|err| {terr:.3e} > {tbound:.3e} ({ev.last_plan()})"
    loc = ref64.localisation(t, r["trunk"])
    bad = ref64.localisation_failures(loc, prec)
    for a, ratio in ref64.localisation_ratios(loc).items():
        stats[a] = max(stats.get(a, 0.0), ratio)
    assert not bad, f"B={n}: localised error {bad} ({loc}; {ev.last_plan()})"
    return _digest(p, v, d, t), (p, v, d, t), err


@pytest.mark.parametrize("prec,F,kind,env", ROWS,
                         ids=[f"{p}-{F}-{k}" + "".join(f"-{e[4:].lower()}{v}" for e, v in env.items())
                              for p, F, k, env in ROWS])
def test_plan_sweep(nsg, oracle, pool, monkeypatch, prec, F, kind, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    probe = nsg.Evaluator(0, 1, 86, precision=prec)
    cus = probe.info()["compute_units"]
    probe.close()
    top = {"full": 4 * cus if F == 256 else 2 * cus + cus // 4 + 1, "team": max(2 * TEAM_MAX, cus // 8 + 1), "conv": 2 * cus,
           "short": 2 * cus, "few": cus + 3, "handful": 2 * cus + 1}[kind]
    sizes = _sizes(cus, F, kind, top)
    if kind == "team":
        sizes = sorted(set(sizes) | {1, 2, 3, cus // 24, cus // 24 + 1, cus // 18, cus // 18 + 1, cus // 12,
                                     cus // 12 + 1, cus // 8, cus // 8 + 1})
        sizes = [b for b in sizes if 1 <= b <= top]
    top = max(sizes)
    w, ref = _reference(nsg, oracle, 2, F, pool, top)
    bb = pool(top)
    ev = nsg.Evaluator(0, top, 86, precision=prec)
    ev.load_memory(nsg.weights.to_blob(w))
    row = dict(prec=prec, F=F, kind=kind, env=env)
    seen, per_size, stats, errs = {}, {}, {}, {}
    try:
        for n in sizes:  # ascending: every board against ref64, and the same boards in reversed slots
            foretold = ev.launch_form(n)
            dig, out, err = _check(ev, prec, n, bb, ref, stats)
            kind_, _ = ev.last_launch_kind()
            form, plan = ev.last_launch_form(), ev.last_plan()
            assert (kind_, form, plan) == foretold, f"B={n}: ran {(kind_, form, plan)}, chooseLaunchForm said {foretold}"
            name = form_of(prec, kind_, form, plan)
            per_size[n] = (dig, name, kind_, form["whole_trunk"], form["parts"], plan["chains"], plan)
            seen.setdefault(name, []).append(n)
            errs[name] = max(errs.get(name, 0.0), err)
            rev = bb[:n][::-1].copy()
            pr, vr, dr = ev.compute_blocking(rev)
            tr = ev.download_trunk(n)
            same_plan = form_of(prec, *ev.last_launch_kind()[:1], ev.last_launch_form(), ev.last_plan()) == name
            assert same_plan, f"B={n}: reversed slots ran another form"
            back = (pr[::-1], vr[::-1], dr[::-1], tr[::-1])
            if form["parts"]:
                for a, b in zip(out, back):
                    assert float(np.abs(a - b).max()) <= TOL[prec] * max(1.0, float(np.abs(a).max())), \
                        f"B={n}: two-part batch, reversed slots disagree"
            else:
                assert _digest(*back) == dig, f"B={n} ({name}): reversed slots are not bit-identical"
        for n in reversed(sizes):  # descending: other histories (stale pad slots, flags, hand-off images), same bits
            p, v, d = ev.compute_blocking(bb[:n])
            t = ev.download_trunk(n)
            assert _digest(p, v, d, t) == per_size[n][0], \
                f"B={n} ({per_size[n][1]}): descending pass differs from the ascending one"
        assert ev.team_stats()["fallbacks"] == 0, f"a persistent launch gave up: {ev.team_stats()}"
    finally:
        ev.close()
    want = {f for f, (_, reach) in FORMS.items() if reach(row, cus)}
    lines = [f"{prec} {F}x2 ({kind}{', ' + str(env) if env else ''}) on {cus} CUs; localisation max ratios " +
             ", ".join(f"{a} {stats.get(a, 0):.2f}" for a in ref64.AXES)]
    for name in sorted(seen):
        lines.append(f"  {name:26s} max|err| {errs[name]:.2e}  sizes {seen[name]}")
    report = "\n".join(lines)
    print(report)
    _REPORT.append(report)
    missing = want - set(seen)
    assert not missing, f"launch forms not reached: {sorted(missing)}\n{report}"


def test_headline_20x256_every_board(nsg, oracle, pool):
    """bench.py's line: 20x256, f16m6, 512 boards of real positions and random bitboards, every board checked."""
    blocks, F, n, prec = 20, 256, 512, "f16m6"
    w = nsg.weights.make_random(blocks, F, seed=0, bn="random")
    bb = pool(n)
    ref = ref64.cached(("headline", blocks, F, n), w, oracle.extract_bits(bb))
    ev = nsg.Evaluator(0, n, 86, precision=prec)
    ev.load_memory(nsg.weights.to_blob(w))
    stats = {}
    try:
        _, _, err = _check(ev, prec, n, bb, ref, stats)
        name = form_of(prec, ev.last_launch_kind()[0], ev.last_launch_form(), ev.last_plan())
        assert ev.team_stats()["fallbacks"] == 0
    finally:
        ev.close()
    print(f"headline 20x256 {prec} B={n}: {name}, max|err| {err:.2e}, localisation max ratios {stats}")


def test_print_coverage():
    """The coverage tables of the rows above, together (run with -s)."""
    print("\n" + "\n".join(_REPORT))
