"""Bit-level host models of the split formats f16x3, f16m8 and f16m6 (kernels.h).

Written from the format definitions, not from the kernels: numpy / torch float64 on the CPU, and of the package only
`weights.to_blob` (the exact nets serialise themselves with it).  Every value a model handles is a float64 holding a
number of the modelled format exactly; a rounding happens only where a function named after a format is called.

Quantisers
    f16        round to nearest even.
    e4m3       OCP fp8, bias 7, subnormal step 2^-9, largest 448: nearest, ties to the even code, saturating.
    e2m3       fp6, bias 1, subnormal step 1/8, largest 7.5: nearest, ties to the even code, saturating.
    E8M0       one byte per 32 input channels, value 2^(byte - 127).
               weights      floor(log2 max|v|) - 2 + 127 clamped to 1..254; an all-zero block: byte 0, codes 0.
               activations  biased f16 exponent (0..30) of the block's largest |f16 value| plus 110: a zero block or a
                            block of f16 subnormals has exponent field 0, hence byte 110.

Weights (the loader)
    BatchNorm folded in double, s = gamma / sqrt(var + eps), w' = float(w s), b' = float(beta - mean s); one power of
    two per layer that puts max|w'| into [2^8, 2^9), undone by accScale = 1 / scale; w_hi = f16(w), w_lo = w - w_hi in
    float32 (exact).  f16x3: f16(w_lo).  f16m8: e4m3(w_lo 2^10) 2^-10 and e4m3(w_hi 2^-2) 2^2.  f16m6: e2m3 of w_lo and of
    w_hi under one E8M0 byte per (output channel, tap, 32 input channels).

Activations (every epilogue, and the expansion of the input planes with floor = -65000)
    x = clamp(v, floor, 65000), floor = 0 with ReLU; hi = f16(x); lo = x - hi in float32 (exact).
    f16x3: f16(lo).  f16m8: e4m3(clamp(hi, +-448)) and e4m3(clamp(lo 2^12, +-448)) 2^-12, lo taken from float32.
    f16m6: lo rounded to f16 first, then e2m3 under the byte of ITS block; an e2m3 copy of hi under the byte of the hi
    block.  The last trunk layer of an MX evaluator stores the f16x3 pair, which the heads read.

One 3x3 layer, in the order of the epilogue
    acc = sum w_hi x_hi + sum q(w_lo) q(x_hi) + sum q(w_hi) x_lo      float32 accumulators, any order and any K split
    v   = fma(acc, accScale, bias)                                      ONE float32 rounding
    r   = hi_res + lo_res                                               one float32 rounding (lo_res as stored: decoded)
    v   = v + r                                                         one float32 rounding
    then the activation split above, whose clamp is the ReLU.
The model sums acc in float64 and rounds it to float32 once: on the exact nets (split_nets.py) no float32 operation of
this list rounds, so the device must give the model's bits in every launch form; on other nets the model is one
admissible evaluation among several.  The f16x3 products are w_hi x_hi + f16(w_lo) x_hi + w_hi f16(x_lo).

Heads of a split evaluator: one f16x3 1x1 product over [value rows (BN folded) | policy rows] with ONE scale for all of
them; policy = fma(acc, accScale, policy_b), index c * 81 + square.

`forward(..., fault=NAME)` evaluates a deliberately wrong model (FAULTS): what tests/test_split_reference.py uses to show
that each such mistake changes bits the device test compares.
"""
import numpy as np
import torch

PRECS = ("f16x3", "f16m8", "f16m6")
M8_LO_SHIFT, M8_WLO_SHIFT, M8_WHI_SHIFT = 12, 10, -2

FAULTS = {
    "drop_wlo_xhi": "the correction term w_lo * x_hi is left out",
    "drop_whi_xlo": "the correction term w_hi * x_lo is left out",
    "wexp_fragment_xor1": "f16m6: the weight blocks of fragment j of a group of four decode under the byte of j ^ 1",
    "xlo_under_hi_exponent": "f16m6: the activation lo block decodes under the hi block's byte",
    "residual_lo_dropped": "the residual is hi alone",
    "lo_direct_to_e2m3": "f16m6: lo goes from float32 to e2m3 without the f16 rounding in between",
    "subnormal_block_exponent_127": "f16m6: an activation block whose f16 exponent field is 0 gets byte 127, not 110",
    "xhi_copy_is_xhi": "MX: w_lo meets x_hi itself, not its e2m3 / e4m3 copy (f16x3 arithmetic on an MX plan)",
    "tap_transposed": "the weights of tap (ky, kx) are taken from tap (kx, ky)",
}


# ---------------------------------------------------------------------------------------------------- quantisers
def f16(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def _table(ebits, mbits, bias, codes):
    t = np.zeros(codes, dtype=np.float64)
    for c in range(codes):
        e, m = c >> mbits, c & ((1 << mbits) - 1)
        t[c] = m / (1 << mbits) * 2.0 ** (1 - bias) if e == 0 else (1 + m / (1 << mbits)) * 2.0 ** (e - bias)
    return t


E2M3 = _table(2, 3, 1, 32)    # magnitudes of codes 0..31; bit 5 is the sign
E4M3 = _table(4, 3, 7, 128)   # magnitudes of codes 0..127; code 127 is NaN; bit 7 is the sign
E4M3[127] = np.nan


def _encode(v, emin, emax, top, sign_bit, nan_code):
    """Nearest code of a format with 3 mantissa bits whose normal binades are 2^emin .. 2^emax, ties to even."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.clip(np.floor(np.log2(np.where(a > 0, a, 1.0))), emin, emax)
    step = np.exp2(e - 3)
    r = np.minimum(np.rint(np.minimum(a, 2 * top) / step) * step, top)  # rint: ties to even; the integer's parity is the code's
    e2 = np.clip(np.floor(np.log2(np.where(r > 0, r, 1.0))), emin, emax)
    sub = r < 2.0 ** emin
    mant = np.where(sub, r / 2.0 ** (emin - 3), r / np.exp2(e2 - 3) - 8)
    code = np.nan_to_num(np.where(sub, mant, (e2 - emin + 1) * 8 + mant)).astype(np.int64)
    code = np.where(np.isnan(v), nan_code, code)
    return (code | np.where(np.signbit(v), sign_bit, 0)).astype(np.uint8)


def e2m3_encode(v):
    return _encode(v, 0, 2, 7.5, 0x20, 0x1f)


def e2m3_decode(code):
    code = np.asarray(code, dtype=np.uint8)
    return np.where(code & 0x20, -1.0, 1.0) * E2M3[code & 0x1f]


def e4m3_encode(v):
    return _encode(v, -6, 8, 448.0, 0x80, 0x7f)


def e4m3_decode(code):
    code = np.asarray(code, dtype=np.uint8)
    return np.where(code & 0x80, -1.0, 1.0) * E4M3[code & 0x7f]


def q_e2m3(v):
    return e2m3_decode(e2m3_encode(v))


def q_e4m3(v):
    return e4m3_decode(e4m3_encode(v))


def _blocks(v):
    """[..., C] -> [..., C / 32, 32] (C a multiple of 32)."""
    return v.reshape(*v.shape[:-1], v.shape[-1] // 32, 32)


def e8m0_weights(v):
    """Byte per block of `v` [..., C]: [..., C / 32]."""
    m = np.abs(_blocks(v)).max(axis=-1)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(m > 0, m, 1.0))) - 2 + 127
    return np.where(m > 0, np.clip(e, 1, 254), 0).astype(np.int64)


def e8m0_activations(v16, subnormal_byte=110):
    """Byte per block of f16 values `v16` [..., C]."""
    m = np.abs(_blocks(v16)).max(axis=-1)
    e5 = (m.astype(np.float16).view(np.uint16).astype(np.int64) >> 10) & 31
    return np.where(e5 == 0, subnormal_byte, e5 + 110)


def mx6(v, byte, decode_byte=None):
    """e2m3 of `v` [..., C] under the block bytes `byte` [..., C / 32]; decoded under decode_byte (default: the same).
    Byte 0 (an all-zero weight block): codes 0."""
    s = np.exp2(byte.astype(np.float64) - 127)[..., None]
    d = s if decode_byte is None else np.exp2(decode_byte.astype(np.float64) - 127)[..., None]
    q = np.where(byte[..., None] == 0, 0.0, q_e2m3(_blocks(v) / s) * d)
    return q.reshape(v.shape)


# ---------------------------------------------------------------------------------------------------- weights
def fold(w, bn, eps):
    """-> (w' float32 values as float64 [F, C, ...], bias float32 values as float64 [F])."""
    g, b, mu, var = (np.asarray(bn[i], dtype=np.float64) for i in range(4))
    s = g / np.sqrt(var + float(np.float32(eps)))
    wf = f32(np.asarray(w, dtype=np.float64) * s.reshape(-1, *([1] * (np.ndim(w) - 1))))
    return wf, f32(b - mu * s)


def layer_scale(wf):
    m = float(np.abs(wf).max())
    if not (m > 0 and np.isfinite(m)):
        return 1.0
    return 2.0 ** (9 - np.frexp(m)[1])


def weight_operands(wf, arith, fault=None):
    """wf [F, C, 3, 3] or [F, C, 1, 1] folded weights -> (w_hi, q(w_lo), q(w_hi)) [F, C, kh, kw], accScale; C padded to 32."""
    F_, C = wf.shape[:2]
    pad = (-C) % 32
    if pad:
        wf = np.concatenate([wf, np.zeros((F_, pad) + wf.shape[2:])], axis=1)
    if fault == "tap_transposed":
        wf = wf.transpose(0, 1, 3, 2)
    scale = layer_scale(wf)
    ws = f32(wf * scale)
    hi = f16(ws)
    lo = f32(ws - hi)
    if arith == "f16x3":
        return (hi, f16(lo), hi), 1.0 / scale
    if arith == "f16m8":
        return (hi, q_e4m3(lo * 2.0 ** M8_WLO_SHIFT) / 2.0 ** M8_WLO_SHIFT,
                q_e4m3(hi * 2.0 ** M8_WHI_SHIFT) / 2.0 ** M8_WHI_SHIFT), 1.0 / scale
    assert arith == "f16m6", arith
    out = [hi]
    for v in (lo, hi):
        t = np.ascontiguousarray(np.moveaxis(v, 1, -1))  # [F, kh, kw, C]: blocks of 32 input channels
        byte = e8m0_weights(t)
        dec = None
        if fault == "wexp_fragment_xor1":  # fragment j = bits 2..3 of the output channel: its neighbour j ^ 1 is n ^ 4
            dec = byte[np.arange(F_) ^ 4]
        out.append(np.moveaxis(mx6(t, byte, dec), -1, 1))
    return tuple(out), 1.0 / scale


# ---------------------------------------------------------------------------------------------------- activations
def activation_operands(v, arith, relu=True, fault=None):
    """v [..., C] float32 values -> dict(hi, xq = the copy of hi that meets w_lo, lo = what meets w_hi and what a
    residual reads, value = hi + lo as stored).  C a multiple of 32."""
    x = np.clip(v, 0.0 if relu else -65000.0, 65000.0)
    hi = f16(x)
    lo32 = f32(x - hi)
    if arith == "f16x3":
        lo, xq = f16(lo32), hi
    elif arith == "f16m8":
        lo = q_e4m3(np.clip(lo32 * 2.0 ** M8_LO_SHIFT, -448, 448)) / 2.0 ** M8_LO_SHIFT
        xq = q_e4m3(np.clip(hi, -448, 448))
    else:
        assert arith == "f16m6", arith
        sub = 127 if fault == "subnormal_block_exponent_127" else 110
        lo16 = f16(lo32)
        bh, bl = e8m0_activations(hi, sub), e8m0_activations(lo16, sub)
        xq = mx6(hi, bh)
        lo = mx6(lo32 if fault == "lo_direct_to_e2m3" else lo16, bl, bh if fault == "xlo_under_hi_exponent" else None)
    if fault == "xhi_copy_is_xhi":
        xq = hi
    return {"hi": hi, "xq": xq, "lo": lo}


# ---------------------------------------------------------------------------------------------------- layers
def lowbit_exponent(a):
    """Exponent of the largest power of two that divides every nonzero entry of `a` (None: all zero)."""
    a = np.asarray(a, dtype=np.float64)
    a = a[a != 0]
    if a.size == 0:
        return None
    m, e = np.frexp(np.abs(a))
    mant = (m * 2.0 ** 53).astype(np.int64)
    low = np.log2((mant & -mant).astype(np.float64))
    return int((e - 53 + low).min())


def _conv(xs, ws):
    """sum over families of the "same" convolution: xs [B, 9, 9, C] each, ws [F, C, kh, kw] each -> [B, 81, F] float64.
    Taps and input channels whose weights are all zero are skipped (the one-tap and one-block nets)."""
    x = torch.from_numpy(np.concatenate(xs, axis=-1))
    w = torch.from_numpy(np.concatenate(ws, axis=1))
    B, k = x.shape[0], w.shape[2]
    h = k // 2
    xp = torch.zeros((B, 9 + 2 * h, 9 + 2 * h, x.shape[-1]), dtype=torch.float64)
    xp[:, h:h + 9, h:h + 9, :] = x
    acc = torch.zeros((B * 81, w.shape[0]), dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            wt = w[:, :, ky, kx]
            live = torch.nonzero((wt != 0).any(dim=0)).flatten()
            if live.numel() == 0:
                continue
            acc += xp[:, ky:ky + 9, kx:kx + 9, :][..., live].reshape(B * 81, -1) @ wt[:, live].T
    return acc.view(B, 81, -1).numpy()


def layer(act, wops, acc_scale, bias, res, arith, fault=None, report=None, name=""):
    """One layer up to the value the epilogue splits: float32 values [B, 81, F] as float64."""
    B = act["hi"].shape[0]
    fam_x = [act["hi"], act["xq"], act["lo"]]
    fam_w = list(wops)
    if fault == "drop_wlo_xhi":
        del fam_x[1], fam_w[1]
    elif fault == "drop_whi_xlo":
        del fam_x[2], fam_w[2]
    xs = [a.reshape(B, 9, 9, -1) for a in fam_x]
    acc = _conv(xs, fam_w)
    v = f32(f32(acc) * acc_scale + bias)
    r = None
    if res is not None:
        r = f32(res["hi"] + (0.0 if fault == "residual_lo_dropped" else res["lo"]))
        v = f32(v + r)
    if report is not None:
        # exactness: q divides every product of the layer (in the output's units), the bias and the residual; then
        # sum|products| + |bias| + |residual| < 2^24 q makes every partial sum in every order a float32
        exps = []
        for a, w in zip(fam_x, fam_w):
            live = (w != 0).any(axis=(0, 2, 3))  # input channels with no weight (the non-binary planes) give no product
            ea, ew = lowbit_exponent(a[..., live]), lowbit_exponent(w)
            if ea is not None and ew is not None:
                exps.append(ea + ew + int(np.log2(acc_scale)))
        for extra in (bias, None if res is None else res["hi"], None if res is None else res["lo"]):
            e = None if extra is None else lowbit_exponent(extra)
            if e is not None:
                exps.append(e)
        q = 2.0 ** min(exps) if exps else 1.0
        mag = _conv([np.abs(a) for a in xs], [np.abs(w) for w in fam_w]) * acc_scale + np.abs(bias)
        if r is not None:
            mag = mag + np.abs(res["hi"]) + np.abs(res["lo"])
        report.append({"layer": name, "q": q, "span": float(mag.max() / q), "exact": bool(mag.max() < 2.0 ** 24 * q)})
    return v


def forward(w, planes, arith, fault=None, fault_layers=None, report=None, keep=None):
    """The network `w` (a weight dict as weights.make_random's) on planes [B, C, 81] with the trunk in `arith`.

    -> {"trunk": [B, F, 81] float32, "policy": [B, 2187] float32}.  report: a list that receives one exactness record
    per 3x3 layer; keep: a list that receives every layer's operands (the coverage assertions); fault_layers: the 3x3
    layers (0 = stem) a fault applies to, default all."""
    assert arith in PRECS, arith
    m = w["_meta"]
    eps, F_, nb = m["bn_eps"], m["channels"], m["blocks"]
    planes = np.asarray(planes, dtype=np.float64)
    B, C = planes.shape[:2]
    x = planes.transpose(0, 2, 1)
    pad = (-C) % 32
    if pad:
        x = np.concatenate([x, np.zeros((B, 81, pad))], axis=-1)
    names = [("stem_w", "stem_bn")] + [(f"b{k}_w{i}", f"b{k}_bn{i}") for k in range(nb) for i in (1, 2)]

    def flt(i):
        return fault if fault_layers is None or i in fault_layers else None

    act = activation_operands(x, arith, relu=False, fault=flt(0))
    block_in = None
    for i, (wn, bn) in enumerate(names):
        wf, bias = fold(w[wn], w[bn], eps)
        wops, s = weight_operands(wf, arith, flt(i))
        res = block_in if (i > 0 and i % 2 == 0) else None
        if i % 2 == 1:
            block_in = act
        v = layer(act, wops, s, bias, res, arith, flt(i), report, wn)
        if keep is not None:
            keep.append({"name": wn, "x": act, "w": wops, "v": v})
        last = i == len(names) - 1
        # the encoder of layer i feeds layer i + 1: its faults belong to the consumer's index
        act = activation_operands(v, "f16x3" if last else arith, relu=True, fault=None if last else flt(i + 1))
    trunk = f32(act["hi"] + act["lo"])
    # heads: f16x3, one scale over the value rows (BN folded) and the policy rows
    vw, _ = fold(w["value_w"], w["value_bn"], eps)
    pw = f32(w["policy_w"])
    rows = np.concatenate([vw, pw], axis=0)[:, :, None, None]
    hops, hs = weight_operands(rows, "f16x3")
    nv = vw.shape[0]
    pol_ops = tuple(o[nv:] for o in hops)
    acc = _conv([a.reshape(B, 9, 9, -1) for a in (act["hi"], act["hi"], act["lo"])], list(pol_ops))
    pol = f32(f32(acc) * hs + f32(w["policy_b"]))
    return {"trunk": trunk.transpose(0, 2, 1).astype(np.float32),
            "policy": pol.transpose(0, 2, 1).reshape(B, -1).astype(np.float32)}
