"""Models around the general graph path's Linear over the 81 squares (kLaunchTokenMix, DESIGN.md sections 13.3 and
13.4: MLP-Mixer's token MLP, ResMLP's cross-patch layer, gMLP's spatial gating projection), their float64 references,
per-element bounds and a float32 emulation with injectable faults: the shared half of tests/test_onnx_tokenmix.py
(host) and tests/test_gpu_onnx_tokenmix.py (device).

The hand-built half.  Every model is the exact stem of elt_models.Net (weights and bias small integers times 2^exp: its
float32 output is exact in any order of summation), C of its channels as [N,C,81] -- the Transpose of a Slice of the
token rows, or the Reshape of a Slice of the spatial tensor --, ONE pattern

    MatMul(x [N,C,81], W1 [81,D]) + b1 -> act1 [-> MatMul(., W2 [D,81]) + b2 -> act2]

and a policy that shows 27 channels of the result through nothing that rounds: the Reshape to [N,2187] where C = 27,
otherwise the Reshape to [N,C,9,9] and a 1x1 conv whose weight is a 0/1 selection (back = "conv"), or the Transpose to
tokens and a selection MatMul (back = "tokens").  Either selection reads the whole rows, pad channels included: a
non-finite value in a pad channel times the zero weight is NaN in every output.  Value and draw read the stem's mean.

Exact cases: stem values are multiples of 2^exp, the constants integers times 2^wexp, the activations none or ReLU.
`inputs` asserts in float64 that sum|w x| + |b| is below 2^24 quanta for every element of either stage: every partial
sum, in any order, is then an integer below 2^24 times the quantum and float32 holds it.  The bound is 0.

Rounded cases: the stem on the fine grid 2^-11 (its values must be known exactly for the bound to be one), the
constants float32 normals.  u = 2^-24, gamma(n) = n u / (1 - n u) as in reduction_models:

  stage 1   e = gamma(84) sum|w x|,  t = sum + b:  d = e + u (|t64| + e)                 the chain, then the bias add
  act       None, ReLU: d.  Sigmoid: d max s' + 2 x 1.28 ulps.  GELU (|t| <= 8 asserted): 1.13 d + 2 x 35.93 ulps
            (1.13 bounds |GELU'|; the ulp figures are DESIGN.md 13.3's, asserted at twice the measurement as there).
            Reciprocal and Sqrt are correctly rounded (half an ulp) behind their slopes, Exp is held to 2 ulps.
  stage 2   sum|W2| dH + gamma(D padded) sum|W2 H|, then the bias add and the activation as above.

The torch half: a Mixer block (token MLP with exact GELU, then channel MLP), a ResMLP block (Affine, one [81,81] stage,
LayerScale, residual) and a gMLP spatial gating unit (split, LayerNorm, [81,81] stage, u * v), each behind a conv stem
with the contract's heads.  They are exported at test time; nothing is added to tests/golden."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import elt_models as em  # noqa: E402
import reduction_models as rm  # noqa: E402
from bmm_models import ulp32  # noqa: E402
from reduction_models import U, gamma  # noqa: E402

WIN = rm.WIN
SIGMOID_ULPS = 2 * 1.28  # measured 1.28 and 35.93, asserted at twice that
GELU_ULPS = 2 * 35.93
GELU_SLOPE = 1.13        # max |GELU'| = 1.1289 (at x = 1.41)
ACT_ONNX = {"relu": "Relu", "sigmoid": "Sigmoid", "exp": "Exp", "recip": "Reciprocal", "sqrt": "Sqrt"}
ACT64 = {None: lambda a: a, "relu": em.ACT64["relu"], "sigmoid": em.ACT64["sigmoid"], "gelu": em.ACT64["gelu"], "exp": np.exp,
         "recip": lambda a: 1.0 / a, "sqrt": np.sqrt}


def pad16(n):
    return (n + 15) // 16 * 16


def act_bound(act, t, d, y):
    """|act32(t') - act64(t)| for |t' - t| <= d, y = act64(t): the slope on d plus the activation's own figure."""
    if act in (None, "relu"):
        return d
    if act == "sigmoid":
        sg = em.ACT64["sigmoid"](np.maximum(np.abs(t) - d, 0.0))  # s' is largest at the point of the interval nearest 0
        return d * sg * (1.0 - sg) * (1.0 + 2.0 * d) + SIGMOID_ULPS * ulp32(y)
    if act == "gelu":
        assert float(np.abs(t).max()) <= 8.0, float(np.abs(t).max())  # the range the ulp figure was measured on
        return GELU_SLOPE * d + GELU_ULPS * ulp32(np.abs(y) + GELU_SLOPE * d)
    if act == "recip":
        assert float((np.abs(t) - d).min()) > 0.0
        s = d / (np.abs(t) * (np.abs(t) - d))
        return s + 0.5 * ulp32(np.abs(y) + s)
    if act == "sqrt":
        assert float((t - d).min()) > 0.0
        s = d / (2.0 * np.sqrt(t - d))
        return s + 0.5 * ulp32(y + s)
    assert act == "exp"
    s = np.abs(y) * np.expm1(d)
    return s + 2.0 * ulp32(np.abs(y) + s)


def act32(act, a):
    f = np.float32
    with np.errstate(all="ignore"):
        if act is None:
            return a
        if act == "relu":
            return np.maximum(a, f(0))
        if act == "sigmoid":
            return (f(1) / (f(1) + np.exp(-a))).astype(f)
        if act == "gelu":
            return em.ACT64["gelu"](a.astype(np.float64)).astype(f)
        if act == "recip":
            return (f(1) / a).astype(f)
        if act == "sqrt":
            return np.sqrt(a).astype(f)
        return np.exp(a).astype(f)


class MixCase(rm.Case):
    """C channels at channel `off` of a stem of `width`; D: None for one stage [81,81], else the hidden width of two.
    src: "tokens" (Transpose of the token rows, sliced along axis 2) or "spatial" (Reshape of the spatial tensor, sliced
    along axis 1).  bias: (first, second) stage has one; act1, act2: one activation behind each.  pattern = False: the
    same model without the pattern (the baseline of the launch counts).  wexp: the constants' grid (exact cases);
    bias_sign: -1 makes every bias negative (with `positive`: every sum stays above zero, the biases do not)."""
    kind = "tokenmix"

    def __init__(self, nsg, C, D=None, off=0, width=None, src="tokens", bias=(True, True), act1=None, act2=None, exact=True,
                 exp=-3, span=1, wexp=0, wspan=3, seed=0, part=0, back="conv", positive=False, pattern=True, bias_sign=0, wscale=0.05):
        self.C, self.D, self.off, self.act1, self.act2, self.exact, self.exp, self.wexp, self.part = C, D, off, act1, act2, exact, exp, wexp, part
        self.two = D is not None
        self.D1 = D if self.two else 81
        W = self.W = width or off + C
        rng = np.random.default_rng(1000 + seed)
        net = self.net = rm.RNet(nsg)
        net.stem(W, seed, exp, span)
        if positive:  # every stem value is above zero
            net.consts["s_w"], net.consts["s_b"] = np.abs(net.consts["s_w"]), np.abs(net.consts["s_b"]) + np.float32(2.0 ** exp)
        self.src = src
        if src == "tokens":
            net.tokens("s", W, "tok")
        net.mark = False
        if src == "tokens":
            x = "tok"
            if (off, C) != (0, W):
                for nm, val in (("st", [off]), ("en", [off + C]), ("ax", [2])):
                    net.const("x_" + nm, val, np.int64)
                x = net.node("Slice", ["tok", "x_st", "x_en", "x_ax"], "xtok", name="x_slice")
            x = net.node("Transpose", [x], "x3", name="x_t", perm=[0, 2, 1])
        else:
            x = "s"
            if (off, C) != (0, W):
                for nm, val in (("st", [off]), ("en", [off + C]), ("ax", [1])):
                    net.const("x_" + nm, val, np.int64)
                x = net.node("Slice", ["s", "x_st", "x_en", "x_ax"], "xs", name="x_slice")
            x = net.node("Reshape", [x, net.const("x_to3", [-1, C, 81], np.int64)], "x3", name="x_c3")

        def weights(k, d, positive_w):
            if exact:
                w = rng.integers(1 if positive_w else -wspan, wspan + 1, size=(k, d)) * 2.0 ** wexp
            else:
                w = rng.normal(size=(k, d)) * wscale
                w = np.abs(w) + 0.01 if positive_w else w
            return em.f32(w)

        def biases(d, quantum):
            b = rng.integers(-8, 9, size=d) * quantum if exact else rng.normal(size=d) * 0.2
            b = -np.abs(b) - quantum if bias_sign < 0 else np.abs(b) + quantum if positive else b
            return em.f32(b)

        y = x
        self.W1 = self.b1 = self.W2 = self.b2 = None
        if pattern:
            q1 = 2.0 ** (exp + wexp)
            self.W1 = weights(81, self.D1, positive)
            y = net.node("MatMul", [y, net.const("w1", self.W1)], "mm1", name="mm1")
            self.b1 = biases(self.D1, q1) if bias[0] else np.zeros(self.D1)
            if bias[0]:
                y = net.node("Add", [net.const("b1", self.b1.reshape(1, 1, -1)), y], "biased1", name="bias1")
            if act1 is not None:
                y = self.act_node(y, act1, "act1")
            if self.two:
                self.W2 = weights(D, 81, positive)
                y = net.node("MatMul", [y, net.const("w2", self.W2)], "mm2", name="mm2")
                self.b2 = biases(81, q1 * 2.0 ** wexp) if bias[1] else np.zeros(81)
                if bias[1]:
                    y = net.node("Add", [y, net.const("b2", self.b2)], "biased2", name="bias2")
                if act2 is not None:
                    y = self.act_node(y, act2, "act2")
        self.result = y
        if C == WIN:
            self.ch = np.arange(WIN)
            self.sel = None
            net.node("Reshape", [y, net.const("to2", [-1, WIN * 81], np.int64)], "policy", name="pflat")
        else:
            self.ch = rm.window(C, part)
            sel = self.sel = np.zeros((WIN, C))
            sel[np.arange(WIN), self.ch] = 1.0
            if back == "conv":
                net.node("Reshape", [y, net.const("to4", [-1, C, 9, 9], np.int64)], "r4", name="rows_4d")
                net.node("Conv", ["r4", net.const("sel", sel.reshape(WIN, C, 1, 1))], "picked", name="select", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
                net.node("Flatten", ["picked"], "policy", name="pflat", axis=1)
            else:
                net.node("Transpose", [y], "ytok", name="y_t", perm=[0, 2, 1])
                net.node("MatMul", ["ytok", net.const("sel", sel.T)], "picked", name="select")
                net.node("Transpose", ["picked"], "pt", perm=[0, 2, 1])
                net.node("Reshape", ["pt", net.const("to2", [-1, WIN * 81], np.int64)], "policy", name="pflat")
        net.mark = True
        net.heads_of("s", W)
        self.data = net.data()

    def act_node(self, y, act, name):
        net = self.net
        if act == "gelu":  # the exporter's exact GELU
            e = net.node("Erf", [net.node("Div", [y, net.const(name + "_sqrt2", [np.sqrt(2.0)])], name + "_xd")], name + "_xe")
            m = net.node("Mul", [y, net.node("Add", [e, net.const(name + "_one", [1.0])], name + "_e1")], name + "_xm")
            return net.node("Mul", [m, net.const(name + "_half", [0.5])], name, name=name)
        return net.node(ACT_ONNX[act], [y], name, name=name)

    # ---- the pattern's exact input and float64 sides ------------------------------------------------------------------
    def inputs(self, x):
        env = self.net.known(x)
        s = env["s"]
        assert rm.on_grid(s, self.exp)
        rows = s.reshape(s.shape[0], s.shape[1], 81).transpose(0, 2, 1)[:, :, self.off:self.off + self.C]  # [N,81,C]
        inp = dict(x=rows, env=env, all=s.reshape(s.shape[0], s.shape[1], 81).transpose(0, 2, 1))
        if self.exact:  # every partial sum of every element, in any order, is an integer below 2^24 times the quantum
            q1 = 2.0 ** (self.exp + self.wexp)
            mass = (np.einsum("sd,nsc->ndc", np.abs(self.W1), np.abs(rows)) + np.abs(self.b1)[None, :, None]) / q1
            assert float(mass.max()) < 2 ** 24, float(mass.max())
            if self.two and self.act1 in (None, "relu"):
                h = np.abs(self.hidden(rows))
                mass = (np.einsum("dj,ndc->njc", np.abs(self.W2), h) + np.abs(self.b2)[None, :, None]) / (q1 * 2.0 ** self.wexp)
                assert float(mass.max()) < 2 ** 24, float(mass.max())
        return inp

    def hidden(self, rows, act="own"):
        """[N,D,C] in float64"""
        t = np.einsum("sd,nsc->ndc", self.W1, rows) + self.b1[None, :, None]
        with np.errstate(all="ignore"):
            return ACT64[self.act1 if act == "own" else act](t)

    def ref(self, inp):
        """[N,81,C]: out[n,j,c]"""
        h = self.hidden(inp["x"])
        if not self.two:
            return h
        with np.errstate(all="ignore"):
            return ACT64[self.act2](np.einsum("dj,ndc->njc", self.W2, h) + self.b2[None, :, None])

    def zero_bound(self):
        return self.exact and self.act1 in (None, "relu") and self.act2 in (None, "relu")

    def bound(self, inp):
        rows = inp["x"]
        if self.zero_bound():
            return np.zeros_like(self.ref(inp))
        t1 = self.hidden(rows, act=None)
        if self.exact:
            d1 = np.zeros_like(t1)
        else:
            e1 = gamma(84) * np.einsum("sd,nsc->ndc", np.abs(self.W1), np.abs(rows))
            d1 = e1 + (U * (np.abs(t1) + e1) if self.b1.any() else 0.0)
        h = self.hidden(rows)
        dh = act_bound(self.act1, t1, d1, h)
        if not self.two:
            return dh
        exact2 = self.exact and self.act1 in (None, "relu")
        t2 = np.einsum("dj,ndc->njc", self.W2, h) + self.b2[None, :, None]
        e2 = np.einsum("dj,ndc->njc", np.abs(self.W2), dh)
        if not exact2:
            e2 = e2 + gamma(pad16(self.D)) * np.einsum("dj,ndc->njc", np.abs(self.W2), np.abs(h))
            if self.b2.any():
                e2 = e2 + U * (np.abs(t2) + e2)
        return act_bound(self.act2, t2, e2, ACT64[self.act2](t2))

    def emulate(self, inp, fault=None):
        """float32 numpy, numpy's own order in the products; one fault by name (FAULTS).  Returns whole rows
        [N,81,stride]: the pad channels are part of what the selection reads."""
        f = np.float32
        x = inp["x"].astype(f)
        stride = pad16(self.C)
        W1, b1 = self.W1.astype(f), self.b1.astype(f)
        if fault == "untransposed":
            assert self.D1 == 81
            W1 = W1.T
        if fault == "neighbour_row":  # the last square read from the first row of the next board
            x = x.copy()
            x[:, 80] = np.roll(x, -1, axis=0)[:, 0]
        xp = np.concatenate([x, np.zeros(x.shape[:2] + (stride - self.C,), f)], axis=2)  # pad channels: zeros
        real = np.arange(stride) < self.C
        with np.errstate(all="ignore"):
            t = np.einsum("sd,nsc->ndc", W1, xp)
            if fault != "dropped_bias":
                t = t + b1[None, :, None]
            h = act32(self.act1, t)
            if not self.two:
                return h if fault == "bias_on_pads" else np.where(real, h, f(0))
            W2, b2 = self.W2.astype(f), self.b2.astype(f)
            Dp = pad16(self.D)
            if fault == "hidden_pads":  # the units D..Dp-1: act1 of a zero sum, against W2's zero pad rows
                h = np.concatenate([h, act32(self.act1, np.zeros((h.shape[0], Dp - self.D, stride), f))], axis=1)
                W2 = np.concatenate([W2, np.zeros((Dp - self.D, 81), f)], axis=0)
            if fault != "bias_on_pads":
                h = np.where(real, h, f(0))
            if fault == "bias2_early":  # bias and activation behind the first hidden fragment, the rest added after
                o = act32(self.act2, np.einsum("dj,ndc->njc", W2[:16], h[:, :16]) + b2[None, :, None]) + np.einsum("dj,ndc->njc", W2[16:], h[:, 16:])
            else:
                o = act32(self.act2, np.einsum("dj,ndc->njc", W2, h) + b2[None, :, None])
            return o if fault == "bias_on_pads" else np.where(real, o, f(0))

    def select(self, out):
        """[N,81,C or stride] -> policy[n, j * 81 + sq]: the view where C = 27, else the selection's sum over the whole row
        (0 * inf = NaN, as on the device)."""
        out = np.asarray(out)
        if self.sel is None:
            return out[:, :, :WIN].transpose(0, 2, 1).reshape(out.shape[0], -1)
        sel = np.concatenate([self.sel, np.zeros((WIN, out.shape[2] - self.C))], axis=1).astype(out.dtype)
        with np.errstate(all="ignore"):
            return np.einsum("jc,nsc->njs", sel, out).reshape(out.shape[0], -1)


# ---- the cases, by id ------------------------------------------------------------------------------------------------
EXACT = {
    "one_c27": dict(C=27),
    "one_c24_relu": dict(C=24, act1="relu"),
    "one_c65_at4": dict(C=65, off=4, back="tokens"),
    "one_c27_at2": dict(C=27, off=2, act1="relu"),
    "one_c80_spatial": dict(C=80, src="spatial", bias=(False, False)),
    "one_c64_spatial_at4": dict(C=64, off=4, width=72, src="spatial", act1="relu"),
    "two_c27_d1": dict(C=27, D=1),
    "two_c24_d16": dict(C=24, D=16, act1="relu"),
    "two_c64_d20_at4": dict(C=64, D=20, off=4, act1="relu", back="tokens"),
    "two_c65_d81": dict(C=65, D=81, act1="relu", bias=(True, False)),
    "two_c80_d100": dict(C=80, D=100, act1="relu", act2="relu"),
    "two_c27_d336": dict(C=27, D=336, act1="relu", wexp=-2),
    "two_c27_d20_at2": dict(C=27, D=20, off=2, src="spatial"),
}
FINE = dict(exp=-11, span=2047, exact=False)  # the stem: 2^-11 times integers up to 2047
ROUNDED = {
    "one_c27": dict(C=27, **FINE),
    "one_c64_sigmoid": dict(C=64, act1="sigmoid", **FINE),
    "two_c27_d100_gelu": dict(C=27, D=100, act1="gelu", wscale=0.02, **FINE),
    "two_c65_d336_relu": dict(C=65, D=336, act1="relu", **FINE),
    "two_c24_d20_sigmoid2": dict(C=24, D=20, act1="relu", act2="sigmoid", **FINE),
}
ROUNDED = {"r_" + k: v for k, v in ROUNDED.items()}
# Pad channels (C = 24 in rows of 32) and hidden pad units (D = 20 of 32) behind Exp, Reciprocal and Sqrt, the whole rows
# read by the selecting conv.  Reciprocal of a zero pad is inf; Sqrt of a pad that received a negative bias is NaN; Exp
# of a pad is 1, hidden by the zero weight, and stands for the activations that are finite at zero.
PADS = {
    "pad_one_exp": dict(C=24, act1="exp", wexp=-6),
    "pad_one_recip": dict(C=24, act1="recip", positive=True),
    "pad_one_sqrt_negative_bias": dict(C=24, act1="sqrt", positive=True, bias_sign=-1, wexp=2),
    "pad_two_recip_d20": dict(C=24, D=20, act1="recip", positive=True),
    "pad_two_exp_recip_d20": dict(C=24, D=20, act1="exp", act2="recip", positive=True, wexp=-7),
}
CASES = dict(EXACT, **ROUNDED, **PADS)
# fault -> the cases built for it
FAULTS = {
    "dropped_bias": ["one_c27", "two_c24_d16", "r_one_c64_sigmoid"],
    "untransposed": ["one_c27", "two_c65_d81", "r_one_c27"],
    "hidden_pads": ["pad_two_recip_d20"],
    "bias_on_pads": ["pad_one_sqrt_negative_bias"],
    "neighbour_row": ["one_c24_relu", "r_two_c27_d100_gelu"],
    "bias2_early": ["two_c80_d100", "r_two_c24_d20_sigmoid2"],
}


def case(nsg, name, part=0, **more):
    return MixCase(nsg, part=part, **dict(CASES[name], **more))


def parts_of(name):
    C = CASES[name]["C"]
    return [0] if C == WIN else rm.starts(C)


def all_parts(names):
    return [(n, p) for n in names for p in parts_of(n)]


# ---- the torch modules -----------------------------------------------------------------------------------------------
def torch_net(kind, F=32, seed=0):
    """kind: "mixer" | "resmlp" | "gmlp".  A conv stem of F channels, the block on the 81 token rows, a 27-channel policy
    conv and the value / draw heads on the mean."""
    import torch
    import torch.nn as nn
    import make_onnx_attention_golden as gen

    class Mixer(nn.Module):
        def __init__(self):
            super().__init__()
            self.n1, self.n2 = nn.LayerNorm(F), nn.LayerNorm(F)
            self.t1, self.t2 = nn.Linear(81, 100), nn.Linear(100, 81)
            self.c1, self.c2 = nn.Linear(F, 2 * F), nn.Linear(2 * F, F)

        def forward(self, x):  # [N,81,F]
            y = self.n1(x).transpose(1, 2)
            x = x + self.t2(nn.functional.gelu(self.t1(y))).transpose(1, 2)
            return x + self.c2(nn.functional.gelu(self.c1(self.n2(x))))

    class ResMLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.mix = nn.Linear(81, 81)
            self.alpha, self.beta = nn.Parameter(torch.linspace(0.5, 1.5, F)), nn.Parameter(torch.linspace(-0.2, 0.2, F))  # Affine
            self.scale = nn.Parameter(torch.full((F,), 0.5))
            self.c1, self.c2 = nn.Linear(F, 2 * F), nn.Linear(2 * F, F)

        def forward(self, x):
            x = x + self.scale * self.mix((self.alpha * x + self.beta).transpose(1, 2)).transpose(1, 2)
            return x + self.c2(nn.functional.gelu(self.c1(x)))

    class GMLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.inp, self.norm, self.mix, self.out = nn.Linear(F, 2 * F), nn.LayerNorm(F), nn.Linear(81, 81), nn.Linear(F, F)

        def forward(self, x):
            u, v = nn.functional.gelu(self.inp(x)).chunk(2, dim=-1)
            v = self.mix(self.norm(v).transpose(1, 2)).transpose(1, 2)
            return x + self.out(u * v)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Conv2d(86, F, 3, padding=1)
            self.block = {"mixer": Mixer, "resmlp": ResMLP, "gmlp": GMLP}[kind]()
            self.policy = nn.Conv2d(F, WIN, 1)
            self.fc_v, self.fc_d = nn.Linear(F, 1), nn.Linear(F, 1)

        def forward(self, x):
            N = x.size(0)
            t = self.block(torch.tanh(self.stem(x)).flatten(2).transpose(1, 2))
            policy = self.policy(t.transpose(1, 2).reshape(N, F, 9, 9)).flatten(1)
            h = t.mean(dim=1)
            return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))

    torch.manual_seed(seed)
    return gen.randomize(Net(), seed + 1).eval()


def export(net, path, opset):
    import make_onnx_norm_golden as ng
    return ng.export_model(net, str(path), opset=opset)
