"""The exact nets of DESIGN 4.6, their pool of boards, and the cached models the host and device tests share.

Tier A ("int"): integer weights, integer negative biases, every lo zero: float64 itself is the reference, in all six
precisions.  Tier B ("tap<t>", "blk<c>"): weights m (1 + j 2^-13) and biases -c + i 2^-12, nonzero only in tap t of
every input-channel block, or in every tap of input block c; compared with split_models.forward.  BatchNorm is
gamma = 1, mean = 0, var = 1 with bn_eps = 0, so the fold returns the weights themselves; the stem is zero on the planes
that are not 0 / 1 over the pool."""
import importlib

import numpy as np

import split_models as sm

POOL = 32
_CACHE = {}


def pool_boards():
    """32 distinct boards: even slots random bitboards with garbage bits, odd slots positions of real games."""
    if "bb" not in _CACHE:
        nsg = importlib.import_module("nshogi-engine_amd")
        bb = np.empty((POOL, 86, 2), dtype=np.uint64)
        bb[0::2] = nsg.synth.random_batch(POOL // 2, 86, seed=515, garbage=True)
        bb[1::2] = nsg.positions.game_positions(POOL // 2, seed=616)
        assert len({b.tobytes() for b in bb}) == POOL
        _CACHE["bb"] = np.ascontiguousarray(bb)
    return _CACHE["bb"]


def pool_planes():
    if "planes" not in _CACHE:
        import oracle_lib
        _CACHE["planes"] = oracle_lib.load().extract_bits(pool_boards())
    return _CACHE["planes"]


def batch_slots(n, offset):
    """Pool entries of the n slots of a batch."""
    return (offset + np.arange(n)) % POOL


def _identity_bn(n):
    return np.stack([np.ones(n), np.zeros(n), np.zeros(n), np.ones(n)]).astype(np.float32)


def _conv_weights(rng, F, cin, live_in, kind, tap, block, per_block, lo):
    """[F, cin, 3, 3]: per output channel and 32-channel input block `per_block` nonzero weights (kind "tap": all in
    tap `tap`; "blk": only input block `block`, one per tap and `per_block` more; "int": anywhere)."""
    w = np.zeros((F, cin, 9), dtype=np.float64)
    mags = np.array([1, 1, 1, 2, 2, 3], dtype=np.float64)
    nblk = (cin + 31) // 32
    for n in range(F):
        for c in range(nblk):
            if kind == "blk" and c != block:
                continue
            chans = np.array([k for k in range(32 * c, min(cin, 32 * c + 32)) if live_in[k]])
            if chans.size == 0:
                continue
            if kind == "tap":
                taps = np.full(per_block, tap)
            elif kind == "blk":
                taps = np.concatenate([np.arange(9), rng.integers(0, 9, per_block)])
            else:
                taps = rng.integers(0, 9, per_block)
            ks = rng.choice(chans, size=len(taps), replace=len(taps) > chans.size)
            for k, t in zip(ks, taps):
                m = rng.choice(mags[:4] if kind == "blk" else mags) * rng.choice([-1.0, -1.0, 1.0])
                j = int(rng.integers(0, 4)) if lo else 0
                w[n, k, t] = m * (1 + j * 2.0 ** -13)
    return w.reshape(F, cin, 3, 3).astype(np.float32)


def _stem_output(w):
    """The stem's activations over the pool in float64, [POOL, 81, F] (integers on the exact nets)."""
    x = pool_planes().astype(np.float64).transpose(0, 2, 1).reshape(POOL, 9, 9, -1)
    v = sm._conv([x], [w["stem_w"].astype(np.float64)]) + w["stem_bn"][1].astype(np.float64)
    return np.maximum(v, 0.0)


def _edge_layer(rng, w, F):
    """b0_w1 / b0_bn1 of the "edge" net: the two encoder edges of f16m6 that need a scale of their own.

    Every output is bias + at most one stem activation in 0..3, so the whole layer stays below 8 and a bias may use all
    24 bits (q = 2^-21).  Channels 32..63 have no weight and the bias 2^-3 + a 2^-13 + b 2^-16 (a < 8, b = 1..3): hi is
    the f16 below, lo = b 2^-16 is an f16 subnormal in every row, so the whole block has exponent field 0 (byte 110,
    under which b 2^-16 is the code 8 b exactly; under byte 127 it would be 0).  Of the other channels every fourth has
    the bias 4 + s 2^-10 (1 + m / 8 + 1 / 16 + d 2^-11): hi = 4 + x, lo = the fraction, twelve significant bits whose
    last is half an f16 step, so the f16 rounding (a tie, to even) lands exactly on the e2m3 midpoint between the codes
    m and m + 1 of the top binade (block byte 115), which then goes to the even code -- while the fraction itself lies
    on the other side of the midpoint (d = +1 for even m, -1 for odd m).  The rest have bias -1."""
    small = _stem_output(w).reshape(-1, F)
    ok = np.nonzero((small.max(axis=0) <= 3) & (small.std(axis=0) > 0))[0]
    assert ok.size >= 8, "too few stem channels with activations in 0..3"
    wt = np.zeros((F, F, 9))
    b = np.full(F, -1.0)
    for n in range(F):
        if n // 32 == 1:
            b[n] = 2.0 ** -3 + int(rng.integers(0, 8)) * 2.0 ** -13 + int(rng.integers(1, 4)) * 2.0 ** -16
            continue
        wt[n, rng.choice(ok), n % 9] = 1.0
        if n % 4 == 1:
            m = (n // 4) % 7
            d = 1.0 if m % 2 == 0 else -1.0
            b[n] = 4.0 + rng.choice([-1.0, 1.0]) * 2.0 ** -10 * (1 + m / 8 + 1 / 16 + d * 2.0 ** -11)
    assert (b.astype(np.float32) == b).all()
    p = _identity_bn(F)
    p[1] = b.astype(np.float32)
    return wt.reshape(F, F, 3, 3).astype(np.float32), p


def make_net(F, blocks, kind, tap=None, block=None, seed=0):
    """kind: "int" (Tier A); "tap", "blk", "res" or "edge" (Tier B).

    "res" (two blocks at every width): weights as "int", one per input block, no w_lo anywhere, and fractions i 2^-12
    in the biases from the second layer of block 0 on -- every product stays on the 2^-12 grid, so two blocks fit the
    window at 192 and 256 channels too, and the second block's residual has a nonzero lo half.
    "edge" (one block, f16m6 only): see _edge_layer; the other layers are those of "tap4" with integer biases."""
    special = kind
    if kind == "res":
        kind, lo_w = "int", False
    elif kind == "edge":
        kind, tap, lo_w = "tap", 4, False
    else:
        lo_w = kind != "int"
    rng = np.random.default_rng([seed, F, blocks, {"int": 0, "tap": 1, "blk": 2, "res": 3, "edge": 4}[special],
                                 tap or 0, block or 0])
    lo = special in ("tap", "blk")
    planes = pool_planes()
    binary = np.array([bool(np.isin(planes[:, c], (0, 1)).all()) for c in range(planes.shape[1])])
    per = {"int": 2 if F == 64 and special == "int" else 1, "tap": 2 if F == 64 else 1, "blk": 0}[kind]
    w = {}

    def bias(n, stem, frac):
        c = rng.integers(0, 3, n).astype(np.float64) if stem else rng.integers(2, 6 + F // 16, n).astype(np.float64)
        i = rng.integers(0, 4, n) if frac and not stem else np.zeros(n)
        return (-c + i * 2.0 ** -12).astype(np.float32)

    def bn(n, stem=False, frac=lo):
        p = _identity_bn(n)
        p[1] = bias(n, stem, frac)
        return p

    w["stem_w"] = _conv_weights(rng, F, 86, binary, kind, tap, None if block is None else block % 3, per + 2, False)
    if lo:  # every eighth stem channel eight times as large: hi blocks whose e2m3 copy has to round (max >= 64: step 2 below 32)
        w["stem_w"][0::8] *= 8
    w["stem_bn"] = bn(F, True)
    for k in range(blocks):
        for i in (1, 2):
            # w_lo only where the input is still integer: the first layer behind the stem
            w[f"b{k}_w{i}"] = _conv_weights(rng, F, F, np.ones(F, bool), kind, tap, block, per, lo_w and (k, i) == (0, 1))
            w[f"b{k}_bn{i}"] = bn(F, frac=lo or (special == "res" and (k, i) >= (0, 2)))
    if special == "edge":
        w["b0_w1"], w["b0_bn1"] = _edge_layer(rng, w, F)
    vc, vh = 32, 256
    pw = np.zeros((27, F))
    for c in range(27):  # every trunk channel shows in some policy channel
        ks = np.arange(c, F, 27)
        pw[c, ks] = rng.choice([1.0, -1.0, 2.0], ks.size)
    w["policy_w"] = pw.astype(np.float32)
    w["policy_b"] = rng.integers(-2, 3, 27).astype(np.float32)
    vw = np.zeros((vc, F))
    for c in range(vc):
        vw[c, rng.choice(F, 2, replace=False)] = rng.choice([1.0, -1.0], 2)
    w["value_w"] = vw.astype(np.float32)
    w["value_bn"] = _identity_bn(vc)
    f1 = np.zeros((vh, vc * 81))
    for n in range(vh):
        f1[n, rng.choice(vc * 81, 4, replace=False)] = rng.choice([1.0, -1.0], 4)
    w["fc1_w"] = f1.astype(np.float32)
    w["fc1_b"] = rng.integers(-1, 2, vh).astype(np.float32)
    w["fc2_w"] = (rng.integers(-2, 3, (2, vh)) * 2.0 ** -8).astype(np.float32)
    w["fc2_b"] = np.array([0.25, -0.5], dtype=np.float32)
    w["_meta"] = dict(blocks=blocks, channels=F, in_channels=86, policy_channels=27, value_channels=vc,
                      value_hidden=vh, bn_eps=0.0)
    return w


TIER_B = [(64, 2), (192, 1), (256, 1), (192, 2), (256, 2)]  # (channels, blocks) of the Tier B families


def cases(F, blocks):
    """{name: (kind, tap, block)} of the Tier B family of a shape.  Two blocks at 192 / 256 channels: "res" alone."""
    if (F, blocks) in ((192, 2), (256, 2)):
        return {"res": ("res", None, None)}
    d = {f"tap{t}": ("tap", t, None) for t in range(9)}
    d.update({f"blk{c}": ("blk", None, c) for c in range(F // 32)})
    if F > 64:
        d["edge"] = ("edge", None, None)
    return d


def ariths(name):
    """The arithmetics in which a case is exact: "edge" needs lo cut to four bits (f16 would keep eleven)."""
    return ("f16m6",) if name == "edge" else sm.PRECS


def net(F, blocks, name):
    key = ("net", F, blocks, name)
    if key not in _CACHE:
        if name == "int":
            _CACHE[key] = make_net(F, blocks, "int")
        else:
            kind, tap, block = cases(F, blocks)[name]
            _CACHE[key] = make_net(F, blocks, kind, tap, block)
    return _CACHE[key]


def model(F, blocks, name, arith, fault=None, report=None, keep=None, fault_layers=None, boards=POOL):
    """split_models.forward of a named net on the pool (its first `boards` entries), once per session for the
    unfaulted model of the whole pool."""
    key = ("model", F, blocks, name, arith)
    if fault is None and report is None and keep is None and key in _CACHE:
        return {k: v[:boards] for k, v in _CACHE[key].items()} if boards < POOL else _CACHE[key]
    out = sm.forward(net(F, blocks, name), pool_planes()[:boards], arith, fault=fault, fault_layers=fault_layers,
                     report=report, keep=keep)
    if fault is None and boards == POOL:
        _CACHE[key] = out
    return out


def reference(F, blocks, name):
    """ref64.forward of a named net on the pool (Tier A's reference; value and draw of every case)."""
    import ref64
    return ref64.cached(("split_nets", F, blocks, name), net(F, blocks, name), pool_planes())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
