"""Device half of DESIGN 4.6: the exact nets of split_nets.py in every launch form, bit for bit.

Per row of the plan sweep's matrix the smallest batch that takes each launch form is found with Evaluator.launch_form
over the sweep's thresholds; that batch and the next size that leaves a partial last tile are run.  Tier A (integer
nets) must equal float64 in every precision; Tier B (nonzero x_lo and w_lo) must equal split_models.forward in the
arithmetic the form runs (the team trunk and the fallback of an MX evaluator run f16x3).  Boards come from a pool of 32
at an offset; every board is compared with its pool entry."""
import numpy as np
import pytest

import split_models as sm
import split_nets as sn
from test_gpu_plan_sweep import FORMS, ROWS, TOL, TEAM_MAX, _sizes, form_of

pytestmark = pytest.mark.gpu

SPLIT = ("f16x3", "f16m8", "f16m6")
# (blocks, cases run in every form) per width; tests/test_split_reference.py asserts exactness for exactly these nets.
# "res" (two blocks) brings a nonzero residual lo into the MX epilogues of 192 / 256 channels; "edge" holds the two
# encoder edges of f16m6 and runs wherever the form's arithmetic is f16m6.
TIER_B = {64: [(2, ("tap4", "blk0", "blk1"))],
          192: [(1, ("tap4", "blk0", "blk5", "edge")), (2, ("res",))],
          256: [(1, ("tap4", "blk0", "blk7", "edge")), (2, ("res",))]}
# Tier A value and draw: the two logits are exact (integers in units of 2^-8, asserted on the host), so the device's
# outputs are tanhf and expf of float64's arguments.  HIP documents tanhf to 2 ulp and expf to 1 ulp.
# value = 0.5 (tanhf(o) + 1): 2 ulp of a tanh below 1 (2^-23) plus the half ulp of a sum below 2 (2^-24), halved.
# draw = 1 / (1 + expf(-o)): e (1 + d1) with |d1| <= 2^-23 moves the quotient by at most 2^-23 e / (1 + e) relative,
# the sum and the division add 2^-24 each: below 2^-22 of a draw below 1.  Both leave room for the float32 rounding of
# the reference's own value (2^-25).
VALUE_BOUND, DRAW_BOUND = 2.0 ** -23, 2.0 ** -22
# the sweep's rows, and 64 channels (one chunk pair, two blocks: the residual's lo half) in the three split precisions
ALL_ROWS = ROWS + [(p, 64, "few", {}) for p in SPLIT]


def _forms(ev, prec, sizes):
    """{form name: smallest batch that takes it}."""
    first = {}
    for n in sizes:
        kind, form, plan = ev.launch_form(n)
        first.setdefault(form_of(prec, kind, form, plan), n)
    return first


def _run(ev, nsg, prec, F, blocks, name, n, offset, cus):
    slots = sn.batch_slots(n, offset)
    foretold = ev.launch_form(n)
    p, v, d = ev.compute_blocking(np.ascontiguousarray(sn.pool_boards()[slots]))
    t = ev.download_trunk(n)
    ran = (ev.last_launch_kind()[0], ev.last_launch_form(), ev.last_plan())
    assert ran == foretold, f"B={n}: ran {ran}, launch_form said {foretold}"
    ref = sn.reference(F, blocks, name)
    if name == "int":
        want_t, want_p = ref["trunk"][slots], ref["policy"][slots]
    else:
        mod = sn.model(F, blocks, name, foretold[2]["trunk_precision"])  # the arithmetic the form reports for the batch
        want_t, want_p = mod["trunk"][slots], mod["policy"][slots]
    bad_t = np.nonzero((sn.bits(t) != sn.bits(want_t)).any(axis=(1, 2)))[0]
    bad_p = np.nonzero((sn.bits(p) != sn.bits(want_p)).any(axis=1))[0]
    what = f"{prec} {F} {name} B={n} offset {offset} {form_of(prec, *ran)}"
    assert bad_t.size == 0, f"{what}: trunk bits differ on boards {bad_t[:8]} (max |d| {np.abs(t - want_t).max():.3e})"
    assert bad_p.size == 0, f"{what}: policy bits differ on boards {bad_p[:8]} (max |d| {np.abs(p - want_p).max():.3e})"
    dv = np.abs(v.astype(np.float64) - ref["value"][slots]).max()
    dd = np.abs(d.astype(np.float64) - ref["draw"][slots]).max()
    tv, td = (VALUE_BOUND, DRAW_BOUND) if name == "int" else (TOL[prec], TOL[prec])  # Tier B: the model has no value head
    assert dv <= tv and dd <= td, f"{what}: value off by {dv:.3e} (bound {tv:.3e}), draw by {dd:.3e} (bound {td:.3e})"


@pytest.mark.parametrize("prec,F,kind,env", ALL_ROWS,
                         ids=[f"{p}-{F}-{k}" + "".join(f"-{e[4:].lower()}{v}" for e, v in env.items())
                              for p, F, k, env in ALL_ROWS])
def test_exact_nets_in_every_form(nsg, monkeypatch, prec, F, kind, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if prec == "f16m8":
        # the load-time guard estimates the activation range from weight norms and would send these integer-weight
        # nets to f16x3 altogether; the model clamps the e4m3 copies as the format does, so nothing needs the window
        monkeypatch.setenv("NSG_M8_GUARD", "0")
    probe = nsg.Evaluator(0, 1, 86, precision=prec)
    cus = probe.info()["compute_units"]
    probe.close()
    top = {"full": 4 * cus if F == 256 else 2 * cus + cus // 4 + 1, "team": max(2 * TEAM_MAX, cus // 8 + 1),
           "conv": 2 * cus, "short": 2 * cus, "few": cus + 3, "handful": 2 * cus + 1}[kind]
    sizes = _sizes(cus, F, kind, top)
    if kind == "team":
        sizes = sorted(set(sizes) | {1, 2, 3, cus // 24, cus // 24 + 1, cus // 18, cus // 18 + 1, cus // 12,
                                     cus // 12 + 1, cus // 8, cus // 8 + 1})
        sizes = [b for b in sizes if 1 <= b <= top]
    row = dict(prec=prec, F=F, kind=kind, env=env)
    ev = nsg.Evaluator(0, max(sizes) + 1, 86, precision=prec)
    tier_b = prec in SPLIT and F in TIER_B
    seen = {}
    try:
        ev.load_memory(nsg.weights.to_blob(sn.net(F, 2, "int")))
        first = _forms(ev, prec, sizes)
        want = {f for f, (_, reach) in FORMS.items() if reach(row, cus)}
        assert not want - set(first), f"launch forms not reachable over the sweep's sizes: {sorted(want - set(first))}"
        runs = []  # (form, batch): the smallest batch of the form, and the next one of it with a partial last tile
        for name, n in first.items():
            runs.append((name, n))
            odd = next((m for m in range(n + 1, n + 4) if m <= max(sizes) + 1 and m % 2 == 1 and
                        form_of(prec, *ev.launch_form(m)) == name), None)
            if odd is not None:
                runs.append((name, odd))
        for i, (name, n) in enumerate(runs):
            _run(ev, nsg, prec, F, 2, "int", n, 3 * i + 1, cus)
            seen.setdefault(name, []).append(n)
        if tier_b:
            whole = {next((f for f in first if f.startswith("per-layer") or f.startswith("tiles")), None),
                     next((f for f in first if f.startswith("whole trunk") or f.startswith("coop") or f == "team trunk"), None)}
            ci = 0
            tier_b_runs = {}
            for blocks, everywhere in TIER_B[F]:
                for case in sn.cases(F, blocks):
                    ev.load_memory(nsg.weights.to_blob(sn.net(F, blocks, case)))
                    ci += 1
                    for i, (name, n) in enumerate(runs):
                        if ev.launch_form(n)[2]["trunk_precision"] not in sn.ariths(case):
                            continue
                        if name in whole or case in everywhere:
                            assert form_of(prec, *ev.launch_form(n)) == name
                            _run(ev, nsg, prec, F, blocks, case, n, 5 * i + ci, cus)
                            tier_b_runs[case] = tier_b_runs.get(case, 0) + 1
            assert all(tier_b_runs.get(c, 0) >= 2 for _, cs in TIER_B[F] for c in cs if prec in sn.ariths(c) or F == 64), tier_b_runs
            print(f"{prec} {F} Tier B forwards per case: {tier_b_runs}")
        assert ev.team_stats()["fallbacks"] == 0, f"a persistent launch gave up: {ev.team_stats()}"
    finally:
        ev.close()
    line = f"{prec} {F} ({kind}{', ' + str(env) if env else ''}) on {cus} CUs: " + \
        "; ".join(f"{k} {v}" for k, v in sorted(seen.items()))
    print(line)
    assert not want - set(seen), f"launch forms not run: {sorted(want - set(seen))}"


@pytest.mark.parametrize("prec", SPLIT)
def test_rounded_net_device_and_model(nsg, prec):
    """A seeded random net: device and model each within TOL of float64; |device - model| is printed, not bounded (a
    last-bit difference of a float32 sum may flip an f16 or fp6 code downstream)."""
    import ref64
    F, n = 256, 20  # above the team trunk's sixteen boards: an MX evaluator runs its own arithmetic
    w = nsg.weights.make_random(2, F, seed=2000 + F, bn="random")
    planes = sn.pool_planes()[:n]
    ref = ref64.cached(("trunk_bits_rounded", F), w, planes)
    ev = nsg.Evaluator(0, n, 86, precision=prec)
    try:
        ev.load_memory(nsg.weights.to_blob(w))
        arith = ev.launch_form(n)[2]["trunk_precision"]
        assert arith == prec, (arith, ev.launch_form(n))
        p, _, _ = ev.compute_blocking(np.ascontiguousarray(sn.pool_boards()[:n]))
        t = ev.download_trunk(n)
    finally:
        ev.close()
    mod = sm.forward(w, planes, arith)
    tb = TOL[prec] * max(1.0, float(np.abs(ref["trunk"]).max()))
    for who, (tt, pp) in {"device": (t, p), "model": (mod["trunk"], mod["policy"])}.items():
        assert np.abs(tt - ref["trunk"]).max() <= tb and np.abs(pp - ref["policy"]).max() <= TOL[prec], who
    print(f"rounded 2x{F} {prec} (trunk arithmetic {arith}, B={n}): |device - model| trunk "
          f"{np.abs(t - mod['trunk']).max():.3e} policy {np.abs(p - mod['policy']).max():.3e}; |device - ref64| trunk "
          f"{np.abs(t - ref['trunk']).max():.3e} policy {np.abs(p - ref['policy']).max():.3e}; "
          f"trunk words equal {(sn.bits(t) == sn.bits(mod['trunk'])).mean():.4f}")
