"""The self-play search arithmetic, restated from the reference's own definitions, and a checker that
recomputes every record of a `selfplay --decision-log` file with it.

Nothing here is derived from csrc/selfplay/selfplay.cc: each function below is the formula at the cited
lines of the reference (paths below its src/), written in plain Python and numpy.  Doubles are evaluated in
the reference's operation order, one IEEE operation at a time (numpy does not contract a*b+c), so a choice
recomputed from the logged bit patterns must equal the logged choice exactly; the first maximum wins, by
strict `>`, as in the reference's loops.

What is NOT taken from the reference, and why:
  * the Dirichlet mix normalises the gamma draws by their sum over the root's N moves.  The reference
    (selfplay/worker.cc:167-177) draws 600 per root and normalises over all 600; the engine draws N, which
    its own notes list as deliberate.  The checker takes the sum over the draws the record holds.
  * std::partial_sort leaves the order among exactly equal scores unspecified: where the score at the cut
    equals the next one, either survivor set is accepted and the case is counted (Report.ties).
  * the f32 softmax is libnshogi's ml::math::softmax_ (called at selfplay/frame.cc:117), which is not in the
    reference tree: it is taken to be exp(x - max) / sum, and the logged f32 output is compared with the
    float64 softmax of the logged logits within (N + 4) * 2**-24 relative per entry (one expf ulp, an N-term
    f32 sum, one divide).

Rules holds the reference's constants.  The honesty checks of tests/test_selfplay_decisions.py change one
of them at a time and require the checker to object."""
import math
from dataclasses import dataclass, field

import numpy as np

HEADER = "nsg-decision-log 1"


@dataclass(frozen=True)
class Rules:
    c_puct: float = 1.25             # selfplay/worker.cc:694
    unvisited_as_visited: bool = False  # worker.cc:701-702: a child without a node scores C * P and nothing else
    swap_blend: bool = False         # worker.cc:761
    noise_weight: float = 0.25       # selfplay/frame.cc:126
    mix_on_gumbel_root: bool = False  # frame.cc:121: `!isGumbel() &&`
    keep_plus_one: bool = True       # worker.cc:853: (NumSort + 1) >> count
    keep_at_least_two: bool = True   # worker.cc:853: max(2, ...)
    c_visit: float = 50.0            # worker.cc:657
    final_by_prior: bool = False     # worker.cc:563-590, 607-632


REFERENCE = Rules()


# ---------------------------------------------------------------- the formulas

def blend(visits, win_sum, draw_sum, draw_value, rules=REFERENCE):
    """computeWinRateOfChild, selfplay/worker.cc:745-762: the child's accumulated win rate is the
    opponent's, so the parent's is (visits - sum) / visits; a draw counts as the side to move's draw value."""
    v = np.asarray(visits, dtype=np.float64)
    win = (v - win_sum) / v
    draw = draw_sum / v
    dv = float(draw_value)
    if rules.swap_blend:
        return win * dv + (1.0 - win) * draw
    return draw * dv + (1.0 - draw) * win


def puct_scores(parent_visits, priors, visits, q, rules=REFERENCE):
    """pickUpEdgeToExplore<false>, selfplay/worker.cc:688-715.  `q`: blend() of the visited children, in
    child order."""
    c = rules.c_puct * math.sqrt(float(parent_visits))       # :694
    score = c * priors.astype(np.float64)                    # :702
    seen = visits > 0
    if rules.unvisited_as_visited:
        # the fault: no special case, :703-705 for every child.  C * P / (1 + 0) alone IS C * P, bit for bit;
        # what differs is the win rate of no visits, 0 / 0, which no strict `>` ever prefers
        q_all = np.full(len(priors), np.nan)
        q_all[seen] = q
        score = score / (1 + visits).astype(np.float64) + q_all
    else:
        score[seen] = score[seen] / (1 + visits[seen]).astype(np.float64) + q   # :703-705
    return score


def first_max(score):
    """`if (Score > ScoreMax)` from lowest(): the first of the largest (worker.cc:707-710, 628-631)."""
    score = np.where(np.isnan(score), -np.inf, score)        # a NaN is never `>`
    return int(np.argmax(score))


def softmax64(logits):
    x = logits.astype(np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def gamma_sum(gamma):
    """std::accumulate(..., 0.0), selfplay/worker.cc:172-173: left to right."""
    s = 0.0
    for g in gamma.tolist():
        s += g
    return s


def dirichlet_mix(softmax, gamma, total, rules=REFERENCE):
    """selfplay/frame.cc:126-131 on noise normalised as in worker.cc:174-176: the draw is divided by the sum
    first, then (1 - EPS) * (double)p + EPS * noise, rounded to f32."""
    eps = rules.noise_weight
    return ((1 - eps) * softmax.astype(np.float64) + eps * (gamma / total)).astype(np.float32)


def initial_halving_playouts(budget, m):
    """selfplay/worker.cc:205-210."""
    return max(1, int(math.floor(float(budget) / (math.log2(float(m)) * float(m)))))


def sampling_scores(noise, priors):
    """sampleTopMMoves, selfplay/worker.cc:802: noise + logit (a Gumbel root keeps the raw logits, frame.cc:116)."""
    return noise + priors.astype(np.float64)


def transform_q(q, visits, rules=REFERENCE):
    """selfplay/worker.cc:656-661: (C_VISIT + N) * C_SCALE * Q with C_SCALE = 1."""
    return (rules.c_visit + visits.astype(np.float64)) * 1.0 * q


def gumbel_scores(noise, priors, q, visits, rules=REFERENCE):
    """selfplay/worker.cc:620-624 and :838-842: noise + logit + transformQ(win rate, visits)."""
    return noise + priors.astype(np.float64) + transform_q(q, visits, rules)


def halving_keep(m, n, count, rules=REFERENCE):
    """executeSequentialHalving, selfplay/worker.cc:848-853."""
    num = min(m, n)
    kept = (num + 1) >> count if rules.keep_plus_one else num >> count
    return max(2, kept) if rules.keep_at_least_two else kept


def halving_schedule(m, count, budget, root_visits, playouts, kept):
    """updateSequentialHalvingSchedule, selfplay/worker.cc:870-905.  Returns (playouts after, goes on)."""
    md = max(1, m >> count)                                  # :874-876
    d = math.log2(float(m)) * float(md)                      # :877
    extra = int(math.floor(float(budget) / d))               # :878-879
    if extra == 0:
        return playouts, False                               # :881-883
    if kept <= 2:
        left = budget + 1 - root_visits                      # :892-894
        return playouts + (left + 1) // 2, True              # :895-896
    return playouts + extra, True                            # :899-900


def gumbel_next_target(targets, visits, playouts):
    """pickUpEdgeToExplore<true>, selfplay/worker.cc:663-685: the first target below the round's quota.
    None where there is none (the reference asserts that this cannot happen)."""
    below = np.flatnonzero(targets & (visits < playouts))
    return int(below[0]) if below.size else None


def most_visited(priors, visits, rules=REFERENCE):
    """transition, AlphaZero style, selfplay/worker.cc:563-590: most visited, ties by the larger prior."""
    if rules.final_by_prior:
        return first_max(priors)
    best, max_visits = None, 0
    for i in range(len(priors)):
        if visits[i] == 0:                                   # :571-579: no child node
            if best is None or (visits[best] == 0 and priors[i] > priors[best]):
                best = i
            continue
        if visits[i] > max_visits:                           # :582-584
            max_visits, best = int(visits[i]), i
        elif visits[i] == max_visits and priors[i] > priors[best]:   # :585-588
            best = i
    return best


def gumbel_final(noise, priors, visits, win_sum, draw_sum, draw_value, targets, rules=REFERENCE):
    """transition, Gumbel, selfplay/worker.cc:600-637: the only move, else the best score over the targets
    (all of them visited there; the unvisited are skipped here)."""
    if len(priors) == 1:
        return 0
    seen = visits > 0
    cand = np.flatnonzero(targets & seen)
    if cand.size == 0:
        return 0
    if rules.final_by_prior:
        return int(cand[first_max(priors[cand])])
    q_all = np.zeros(len(priors))
    q_all[seen] = blend(visits[seen], win_sum, draw_sum, draw_value, rules)
    score = gumbel_scores(noise[cand], priors[cand], q_all[cand], visits[cand], rules)
    return int(cand[first_max(score)])


def top_k_agrees(score, k, logged):
    """Is `logged` (flags) a top-k set of `score` by descending order?  Returns (agrees, tie): tie where the
    k-th and (k+1)-th scores are equal, so that partial_sort may keep either."""
    order = np.sort(score)[::-1]
    cut = order[k - 1]
    must, may = score > cut, score == cut
    agrees = int(logged.sum()) == k and bool(np.all(logged[must])) and bool(np.all((must | may)[logged]))
    return agrees, bool(k < len(order) and order[k] == cut)


# ---------------------------------------------------------------- the log

def _f32(tok):
    if tok == "-":
        return np.zeros(0, dtype=np.float32)
    return np.frombuffer(bytes.fromhex(tok), dtype=">u4").astype(np.uint32).view(np.float32)


def _f64(tok):
    if tok == "-":
        return np.zeros(0, dtype=np.float64)
    return np.frombuffer(bytes.fromhex(tok), dtype=">u8").astype(np.uint64).view(np.float64)


def _u32(tok):
    if tok == "-":
        return np.zeros(0, dtype=np.int64)
    return np.frombuffer(bytes.fromhex(tok), dtype=">u4").astype(np.int64)


def _flags(tok):
    if tok == "-":
        return np.zeros(0, dtype=bool)
    return np.frombuffer(tok.encode(), dtype=np.uint8) == ord("1")


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def records_by_game(path):
    """game id -> its record lines, in file order."""
    games = {}
    with open(path) as f:
        assert f.readline().rstrip("\n") == HEADER
        for line in f:
            games.setdefault(int(line.split(" ", 2)[1]), []).append(line)
    return games


@dataclass
class Report:
    counts: dict = field(default_factory=dict)       # record type -> records checked
    disagreements: int = 0
    examples: list = field(default_factory=list)     # the first few, as text
    ties: int = 0                                    # sample / halve records with equal scores at the cut
    noisy_evaluations: int = 0                       # evaluation records with a Dirichlet mix
    nonuniform_evaluations: int = 0                  # evaluation records whose priors are not all equal
    softmax_worst: float = 0.0                       # largest deviation seen, in units of (N + 4) * 2**-24
    games: set = field(default_factory=set)


def check_log(path, rules=REFERENCE, kinds=None):
    """Recomputes every record of the log at `path` under `rules` (`kinds`: of these record types only)."""
    rep = Report()
    last = {}  # game -> (ply, playouts) of its previous record

    def bad(line_no, what):
        rep.disagreements += 1
        if len(rep.examples) < 10:
            rep.examples.append(f"line {line_no}: {what}")

    with open(path) as f:
        head = f.readline().rstrip("\n")
        if head != HEADER:
            raise ValueError(f"not a version 1 decision log: {head!r}")
        for line_no, line in enumerate(f, start=2):
            if kinds is not None and line[:line.index(" ")] not in kinds:
                continue
            t = line.rstrip("\n").split(" ")
            kind, game, ply, playouts = t[0], int(t[1]), int(t[2]), int(t[3])
            rep.counts[kind] = rep.counts.get(kind, 0) + 1
            rep.games.add(game)
            if (ply, playouts) < last.get(game, (0, 0)):
                bad(line_no, f"game {game}: records out of order")
            last[game] = (ply, playouts)
            a = t[4:]
            if kind == "evaluation":
                _check_evaluation(a, rules, rep, lambda w: bad(line_no, "evaluation: " + w))
            elif kind == "select":
                parent_visits, dv, n = int(a[1]), _f32(a[2])[0], int(a[3])
                priors, visits, wins, draws, chosen = _f32(a[4]), _u32(a[5]), _f64(a[6]), _f64(a[7]), int(a[8])
                assert len(priors) == len(visits) == n
                seen = visits > 0
                q = blend(visits[seen], wins, draws, dv, rules)
                want = first_max(puct_scores(parent_visits, priors, visits, q, rules))
                if want != chosen:
                    bad(line_no, f"select: child {chosen} logged, {want} recomputed")
            elif kind == "gumbel-select":
                quota, n, targets, visits, chosen = int(a[0]), int(a[1]), _flags(a[2]), _u32(a[3]), int(a[4])
                assert len(targets) == len(visits) == n
                want = gumbel_next_target(targets, visits, quota)
                if want != chosen:
                    bad(line_no, f"gumbel-select: child {chosen} logged, {want} recomputed")
            elif kind == "search-start":
                budget, m, quota = int(a[0]), int(a[1]), int(a[2])
                want = initial_halving_playouts(budget, m)
                if want != quota:
                    bad(line_no, f"search-start: quota {quota} logged, {want} recomputed")
            elif kind == "sample":
                m, n, noise, priors, targets = int(a[0]), int(a[1]), _f64(a[2]), _f32(a[3]), _flags(a[4])
                assert len(noise) == len(priors) == len(targets) == n
                if m >= n:                                   # worker.cc:793-796
                    if not targets.all():
                        bad(line_no, "sample: fewer moves than samples, yet not all are targets")
                else:
                    ok, tie = top_k_agrees(sampling_scores(noise, priors), m, targets)
                    rep.ties += tie
                    if not ok:
                        bad(line_no, "sample: the targets are not the top m by noise + logit")
            elif kind == "halve":
                _check_halve(a, rules, rep, lambda w: bad(line_no, "halve: " + w))
            elif kind == "transition":
                mode, dv, n = int(a[0]), _f32(a[1])[0], int(a[2])
                visits, wins, draws, priors = _u32(a[3]), _f64(a[4]), _f64(a[5]), _f32(a[6])
                targets, noise, chosen = _flags(a[7]), _f64(a[8]), int(a[9])
                assert len(visits) == len(priors) == n
                if mode == 0:
                    want = most_visited(priors, visits, rules)
                else:
                    want = gumbel_final(noise, priors, visits, wins, draws, dv, targets, rules)
                if want != chosen:
                    bad(line_no, f"transition: child {chosen} logged, {want} recomputed")
            else:
                bad(line_no, f"unknown record type {kind}")
    return rep


def _check_evaluation(a, rules, rep, bad):
    n, gumbel, full, is_root = int(a[0]), a[1] == "1", a[2] == "1", a[3] == "1"
    logits, soft, gamma = _f32(a[6]), _f32(a[7]), _f64(a[8])
    priors = soft if a[10] == "=" else _f32(a[10])           # "=": the writer found them equal bit for bit
    assert len(logits) == len(priors) == n
    if not np.all(priors == priors[0]):
        rep.nonuniform_evaluations += 1
    if gumbel and is_root and not rules.mix_on_gumbel_root:  # frame.cc:116: the raw logits
        if len(soft) or len(gamma) or not _same_bits(priors, logits):
            bad("a Gumbel root does not keep the raw logits")
        return
    if len(soft) != n:
        return bad("no softmax where the reference takes one")
    want = softmax64(logits)
    bound = (n + 4) * 2.0 ** -24
    worst = float(np.max(np.abs(soft.astype(np.float64) - want) / want)) / bound
    rep.softmax_worst = max(rep.softmax_worst, worst)
    if worst > 1.0:
        bad(f"softmax off by {worst:.3f} of the bound")
    noisy = is_root and full and (not gumbel or rules.mix_on_gumbel_root)  # frame.cc:121-125
    if noisy != (len(gamma) == n):
        return bad("noise drawn" if len(gamma) else "no noise drawn where the reference mixes it in")
    if not noisy:
        if not _same_bits(priors, soft):
            bad("priors differ from the softmax output")
        return
    rep.noisy_evaluations += 1
    total = gamma_sum(gamma)
    if total <= 0.0:
        total = 1.0
    if _bits(np.float64(total).reshape(1))[0] != int(a[9], 16):
        bad("sum of the gamma draws")
    if not _same_bits(priors, dirichlet_mix(soft, gamma, total, rules)):
        bad("priors are not the mix of the logged softmax and noise")


def _check_halve(a, rules, rep, bad):
    dv, count, m, n, before = _f32(a[0])[0], int(a[1]), int(a[2]), int(a[3]), _flags(a[4])
    visits, wins, draws, priors, noise = _u32(a[5]), _f64(a[6]), _f64(a[7]), _f32(a[8]), _f64(a[9])
    budget, root_visits, quota = int(a[10]), int(a[11]), int(a[12])
    kept, after, quota_after, goes_on = int(a[13]), _flags(a[14]), int(a[15]), a[16] == "1"
    assert len(before) == len(after) == n and len(visits) == int(before.sum())
    want_kept = halving_keep(m, n, count, rules)
    if want_kept != kept:
        return bad(f"{kept} kept, {want_kept} recomputed")
    score = np.full(n, np.finfo(np.float64).min)             # worker.cc:829-831: not a target
    score[before] = gumbel_scores(noise, priors, blend(visits, wins, draws, dv, rules), visits, rules)
    ok, tie = top_k_agrees(score, kept, after)
    rep.ties += tie
    if not ok:
        bad("the survivors are not the top scores")
    want_quota, want_on = halving_schedule(m, count, budget, root_visits, quota, kept)
    if (want_quota, want_on) != (quota_after, goes_on):
        bad(f"schedule: quota {quota_after}, goes on {goes_on} logged; {want_quota}, {want_on} recomputed")
