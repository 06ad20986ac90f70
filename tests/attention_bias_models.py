"""Models whose attention scores take an additive bias computed at run time, shared by
tests/test_onnx_attention_bias.py (host) and tests/test_gpu_onnx_attention_bias.py (device).

The torch half: `Generator` is the bias generator current board-game transformers use (Lc0's "smolgen"): a token
Linear(F, comp), the tokens flattened to [N, 81 comp] in their own order, Linear + swish, and then one of three forms

  A  Linear(hidden, 6561) -> [N,1,81,81]                          one bias for all heads, a flat tensor viewed 4-D
  B  Linear(hidden, H 6561) -> [N,H,81,81]                        a flat tensor, head stride 6561
  C  Linear(hidden, H K) -> LayerNorm -> [N,H,K] -> one shared Linear(K, 6561, bias=False) -> [N,H,81,81]
                                                                  the Lc0 form: head rows, head stride 6576

`BiasAttention` adds that bias to the scores of make_onnx_attention_golden.Attention, before or after the constant
bias, in either operand order, optionally with a scalar Mul behind it; `BiasNet` is AttNet around it.  The models are
exported at test time with the shared recipe: no file is added to tests/golden.

The hand-built half: `RtAttCase` is reduction_models.AttCase with a run-time bias whose every bit is known: the global
max of the exact stem over the squares (a flat [N,64] tensor on the grid) goes through one dense layer whose weights
are small integers (times a power of two), so the bias is a sum of exactly representable products, exact in float32 in
any order; it differs per board (the stem), per head, per query and per key (the weights).  `ref`, `bound` and
`emulate` are AttCase's with the bias added; the bound gains the terms of the two added roundings (below)."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_onnx_attention_golden as gen  # noqa: E402
import reduction_models as rm  # noqa: E402
from reduction_models import U, gamma  # noqa: E402


# ---- torch models ----------------------------------------------------------------------------------------------------
class Generator(nn.Module):
    def __init__(self, F, H, form, comp=16, hidden=32, K=16, heads=None):
        super().__init__()
        self.form, self.H, self.K = form, H, K
        self.comp = nn.Linear(F, comp)
        self.fc1 = nn.Linear(81 * comp, hidden)
        if form == "A":
            self.out = nn.Linear(hidden, 6561)
        elif form == "B":
            self.out = nn.Linear(hidden, H * 6561)
        else:
            self.fc2 = nn.Linear(hidden, H * K)
            self.ln = nn.LayerNorm(H * K)
            self.out = nn.Linear(K, 6561, bias=False)  # shared by the heads

    def forward(self, x):
        N = x.size(0)
        h = Fn.silu(self.fc1(self.comp(x).flatten(1)))
        if self.form == "A":
            return self.out(h).view(N, 1, 81, 81)
        if self.form == "B":
            return self.out(h).view(N, self.H, 81, 81)
        h = self.ln(self.fc2(h)).view(N, self.H, self.K)
        return self.out(h).view(N, self.H, 81, 81)

    def flops(self, F):
        comp, hidden = self.comp.out_features, self.fc1.out_features
        f = 2 * 81 * F * comp + 2 * 81 * comp * hidden
        if self.form == "A":
            return f + 2 * hidden * 6561
        if self.form == "B":
            return f + 2 * hidden * self.H * 6561
        return f + 2 * hidden * self.H * self.K + 2 * self.H * self.K * 6561

    launches = property(lambda self: 3 if self.form in "AB" else 5)  # the views cost none; swish rides on fc1


class BiasAttention(gen.Attention):
    """rt_first: the run-time Add stands before the constant one; swap: the bias is the Add's first operand;
    mul_behind: a scalar Mul behind both Adds (it scales the scores and both biases).  tweak: "second_rt" (two
    run-time Adds), "relu_bias" (a Relu on the 4-D bias), "bias_twice" (the bias view feeds the Add and a second
    consumer) are outside the pattern, for the refusal tests."""

    def __init__(self, F, H, form="A", rt_first=False, swap=False, mul_behind=None, gen_kw=None, **kw):
        super().__init__(F, H, **kw)
        self.gen = Generator(F, H, form, **(gen_kw or {}))
        self.gen2 = Generator(F, H, form) if self.tweak == "second_rt" else None
        self.rt_first, self.swap, self.mul_behind = rt_first, swap, mul_behind
        self.rt = None  # checks only: the last run-time bias as the softmax sees it

    def scale_bias(self, s):
        with torch.no_grad():
            self.gen.out.weight *= s
            if self.gen.out.bias is not None:
                self.gen.out.bias *= s

    def forward(self, x):
        N = x.size(0)
        q, k, v = self.qkv(x).chunk(3, dim=-1) if self.fused else (self.q(x), self.k(x), self.v(x))
        scale = self.d ** -0.5
        if self.scale_on == "q":
            q = q * scale
        if self.scale_on == "k":
            k = k * scale
        q = q.view(N, 81, self.H, self.d).transpose(1, 2)
        v = v.view(N, 81, self.H, self.d).transpose(1, 2)
        k = k.view(N, 81, self.H, self.d).permute(0, 2, 3, 1)
        a = q @ k
        if self.scale_on == "scores":
            a = a * scale
        rt = self.gen(x)
        if self.tweak == "relu_bias":
            rt = torch.relu(rt)
        if self.rt_first:
            a = rt + a if self.swap else a + rt
        if self.rel is not None:
            a = a + self.rel
        if not self.rt_first:
            a = rt + a if self.swap else a + rt
        if self.gen2 is not None:
            a = a + self.gen2(x)
        if self.mul_behind is not None:
            a = a * self.mul_behind
        self.scores = a
        self.rt = rt * (self.mul_behind if self.mul_behind is not None else 1.0)
        a = torch.softmax(a, dim=-1)
        o = (a @ v).transpose(1, 2).reshape(N, 81, self.F)
        if self.tweak == "bias_twice":
            o = o + rt.reshape(N, -1, 81)[:, :81, :1]
        return self.proj(o) if self.proj is not None else o


class BiasNet(gen.AttNet):
    def __init__(self, F, H, C=86, **kw):
        super().__init__(F, H, C=C)
        self.att = BiasAttention(F, H, **kw)

    def flops(self):
        a = self.att
        F, H, d = a.F, a.H, a.d
        f = 2 * 81 * 9 * 86 * F + 2 * 81 * (F * 3 * F + F * F) + 2 * (2 * 81 * 81 * d) * H
        return f + 2 * 81 * F * 27 + 2 * 2 * F + a.gen.flops(F)

    def launches(self):
        # stem, QKV (fused: 1), attention, projection (+ residual), policy, mean, value, draw, planes and outputs: AttNet's
        return 1 + (1 if self.att.fused else 3) + 1 + 1 + 1 + 1 + 2 + 2 + self.att.gen.launches


class SmolgenPreNet(gen.PreNet):
    """make_onnx_attention_golden.PreNet (the attention bench net of scripts/graph_bench.py) with generator C in every
    block: each block's attention takes a run-time bias [N,H,81,81] from that block's own tokens."""

    def __init__(self, C=86, F=256, H=8, ffn=1024, VH=256, blocks=8, comp=32, hidden=256, K=64):
        super().__init__(C=C, F=F, H=H, ffn=ffn, VH=VH, blocks=blocks)
        for i, b in enumerate(self.blocks):
            b.att = BiasAttention(F, H, form="C", bias=(i == 0), gen_kw=dict(comp=comp, hidden=hidden, K=K))


def sharpen_bias(net, x, target=2.0):
    """Scales the generator's last layer until the run-time bias has a standard deviation near `target` across the keys
    (a near-zero bias would hide a dropped or mis-indexed one); returns that standard deviation."""
    a = net.att
    for _ in range(4):
        with torch.no_grad():
            net(x)
        sd = float(a.rt.std(dim=-1).mean())
        a.scale_bias(min(max(target / max(sd, 1e-9), 1e-3), 1e3))
    with torch.no_grad():
        net(x)
    sd = float(a.rt.std(dim=-1).mean())
    a.rt = a.scores = None
    return sd


def build(F, H, seed, **kw):
    """A BiasNet with randomised biases and LayerNorm parameters (make_onnx_attention_golden.randomize)."""
    torch.manual_seed(seed)
    return gen.randomize(BiasNet(F, H, **kw), seed).eval()


# ---- the near-direct case --------------------------------------------------------------------------------------------
RT_KINDS = {"broadcast": 0, "flat": 6561, "rows": 6576}  # the kernel's head stride per kind
RT_FAULTS = ("rt_transposed", "rt_previous_head", "rt_board0", "rt_scale_dropped")


class RtAttCase(rm.AttCase):
    """reduction_models.AttCase (exact stem, q / k / v views, one attention launch, a 0/1 policy) plus a run-time bias
    whose every bit is known.  g = the stem's max over the squares, a flat [N,64] tensor on the grid of 2^exp.
      "broadcast"  MatMul(g, W [64,6561]) + c -> Reshape [N,1,81,81]                          head stride 0
      "flat"       MatMul(g, W [64,H 6561]) + c -> Reshape [N,H,81,81]                        head stride 6561
      "rows"       Reshape g to [N,H,64/H] -> MatMul W [64/H,6561] -> Reshape [N,H,81,81]     head stride 6576
    W holds integers in -3..3 times 2^wexp, so the bias is a sum of exactly representable products, exact in float32 in
    any order (asserted); it differs per board (g), per head, per query and per key (W).  mask: c is -inf except at
    one key per (head, query) -- `closed` -- on every board, so each output row equals one V row bit for bit (kind
    "rows": the constant Add rides in the head-row dense launch).  mask_board = the planes x of the batch (kinds
    "flat" and "broadcast"): the mask holds on ONE board only, made from run-time data: with g0 the first channel of
    g whose largest value one board holds alone, and thr the second largest g0 of the batch, z = 1 - 16 (g0 - thr) closed is a second dense layer of g, exact;
    it is >= 1 on every board but the one with the largest g0, and <= -1 there where a key is closed; t = Clip(z, 0, 1)
    is exactly 0 or 1 and Log(t) exactly -inf or 0, added to the bias elementwise.  -inf must stay with its board.
    rt_scale: a scalar Mul behind the run-time Add; it scales the scores and the constant bias too, and is a power of
    two, which rounds nothing.

    The bound is section 13.6's attention bound with the terms of the two added roundings, fl(rtScale rt) and
    fl(t + that): each adds u times the magnitude of its result to the score's error delta.  The cases here keep d in
    {16, 64} (exact = True) have every operand on a grid on which acc scale, + bias, rtScale rt and the last sum are all
    exactly representable (asserted on the final scores in `inputs`): both added terms, like delta itself, are then
    zero.  The cases at d = 32 and 48 (exact = False: the scale is no power of two) carry the full delta: `bound`
    below is AttCase.bound with delta = e_t + u (|t2| + e_t) [the constant Add] + u |rtScale rt| + u (|s| + delta so
    far) [the two added roundings], s in units of the final factor rt_scale, which is a power of two."""

    def __init__(self, nsg, F, H, kind="rows", rt_scale=None, wexp=-2, mask=False, heads=None, second=False, exp=-3,
                 seed=0, bias="grid", start=0, stem=64, exact=True, mask_board=None, other=False):
        self.kind, self.rt_scale, self.wexp, self.mask = kind, rt_scale, wexp, mask
        self.F, self.H, self.d, self.exp, self.exact, self.start = F, H, F // H, exp, exact, start
        self.thr = None
        self.offs = (0, (stem - F) // 2 // 4 * 4, stem - F)
        self.scale = float(np.float32(self.d ** -0.5))
        self.bias = None if bias is None else rm.att_bias(bias, H, seed).astype(np.float32).astype(np.float64)
        self.bias_kind = bias
        Hb = self.Hb = heads or (1 if kind == "broadcast" else H)
        net = self.net = rm.RNet(nsg)
        net.stem(stem, seed, exp, 1)
        net.tokens("s", stem, "tok")
        views = {}
        for nm, off in zip("qkv", self.offs):
            if off in views:
                continue
            sizes = [z for z in (off, F, stem - off - F) if z > 0]
            outs = [f"{nm}_{i}" for i in range(len(sizes))]
            if len(sizes) > 1:
                net.const(nm + "_sizes", sizes, np.int64)
                net.node("Split", ["tok", nm + "_sizes"], outs, name=nm + "_split", axis=2)
                views[off] = outs[1 if off > 0 else 0]
            else:
                views[off] = "tok"
        net.mark = False
        # the generator: exact by construction
        rng = np.random.default_rng(500 + 10 * Hb + seed)
        net.node("GlobalMaxPool", ["s"], "gm4", name="gmax")
        net.node("Flatten", ["gm4"], "gm", name="gmflat", axis=1)
        if kind == "rows":
            K = stem // Hb
            self.W = rng.integers(-3, 4, size=(K, 6561)) * 2.0 ** wexp
            self.c = np.zeros(Hb * 6561)
            net.node("Reshape", ["gm", net.const("to_rows", [-1, Hb, K], np.int64)], "gm_rows", name="rows")
            if mask:  # the same row for every head: the constant Add is per channel of the head rows
                self.c = np.tile(np.where(self.closed(1).reshape(-1), -np.inf, 0.0), Hb)
                net.node("MatMul", ["gm_rows", net.const("rt_w", self.W)], "rt_mm", name="rt_dense")
                net.node("Add", ["rt_mm", net.const("rt_c", self.c[:6561])], "rt_flat", name="rt_add")
            else:
                net.node("MatMul", ["gm_rows", net.const("rt_w", self.W)], "rt_flat", name="rt_dense")
        else:
            self.W = rng.integers(-3, 4, size=(stem, Hb * 6561)) * 2.0 ** wexp
            self.c = np.where(self.closed(Hb).reshape(-1), -np.inf, 0.0) if mask else np.zeros(Hb * 6561)
            net.node("MatMul", ["gm", net.const("rt_w", self.W)], "rt_mm", name="rt_dense")
            net.node("Add", ["rt_mm", net.const("rt_c", self.c)], "rt_plain" if mask_board is not None else "rt_flat", name="rt_add")
            if mask_board is not None:
                gs = np.sort(self.stem_max(net.known(mask_board)), axis=0)
                self.gch = int(np.argmax(gs[-1] > gs[-2]))  # the first channel of g whose largest value one board holds alone
                assert gs[-1, self.gch] > gs[-2, self.gch]
                self.thr = float(gs[-2, self.gch])
                shut = self.closed(Hb).reshape(-1).astype(np.float64)
                wz = np.zeros((stem, Hb * 6561))
                wz[self.gch] = -16.0 * shut
                net.node("MatMul", ["gm", net.const("mask_w", wz)], "mask_mm", name="mask_dense")
                net.node("Add", ["mask_mm", net.const("mask_c", 1.0 + 16.0 * self.thr * shut)], "mask_z", name="mask_add")
                net.node("Clip", ["mask_z", net.const("mask_lo", np.zeros(())), net.const("mask_hi", np.ones(()))], "mask_t", name="mask_clip")
                net.node("Log", ["mask_t"], "mask_m", name="mask_log")
                net.node("Add", ["rt_plain", "mask_m"], "rt_flat", name="mask_into_bias")
        net.node("Reshape", ["rt_flat", net.const("to_bias", [-1, Hb, 81, 81], np.int64)], "rt4", name="rt_view")
        net.const("to4", [-1, 81, H, self.d], np.int64)
        q4, k4, v4 = (net.node("Reshape", [views[off], "to4"], nm + "4") for nm, off in zip("qkv", self.offs))
        qh = net.node("Transpose", [q4], "qh", perm=[0, 2, 1, 3])
        kt = net.node("Transpose", [k4], "kt", perm=[0, 2, 3, 1])
        vh = net.node("Transpose", [v4], "vh", perm=[0, 2, 1, 3])
        a = net.node("MatMul", [qh, kt], "qk")
        a = net.node("Mul", [a, net.const("scale", [self.scale])], "scaled")
        if self.bias is not None:
            a = net.node("Add", [a, net.const("rel", self.bias)], "biased")
        if other:  # a run-time tensor that is no score-bias view: the flat generator output itself
            a = net.node("Add", [a, "rt_flat"], "with_rt", name="rt_into_scores")
        else:
            a = net.node("Add", [a, "rt4"], "with_rt", name="rt_into_scores")
        if second:
            a = net.node("Add", [a, "rt4"], "with_rt2", name="rt_again")
        if rt_scale is not None:
            a = net.node("Mul", [a, net.const("rt_scale", [rt_scale])], "rt_scaled", name="rt_mul")
        p = net.node("Softmax", [a], "probs", axis=-1)
        o = net.node("MatMul", [p, vh], "oh")
        o = net.node("Transpose", [o], "ot", perm=[0, 2, 1, 3])
        o = net.node("Reshape", [o, net.const("to3", [-1, 81, F], np.int64)], "att")
        self.ch = rm.window(F, start)
        sel = np.zeros((F, rm.WIN))
        sel[self.ch, np.arange(rm.WIN)] = 1.0
        net.node("MatMul", [o, net.const("sel", sel)], "picked", name="select")
        net.node("Transpose", ["picked"], "pt", perm=[0, 2, 1])
        net.node("Reshape", ["pt", net.const("to2", [-1, rm.WIN * 81], np.int64)], "policy", name="pflat")
        net.mark = True
        net.heads_of("s", stem)
        self.data = net.data()

    @staticmethod
    def closed(Hb):
        """[Hb,81,81]: every (head, query) keeps the one key (7 query + 5 head + 2) % 81."""
        h, i, j = np.arange(Hb)[:, None, None], np.arange(81)[None, :, None], np.arange(81)[None, None, :]
        return np.broadcast_to(j != (7 * i + 5 * h + 2) % 81, (Hb, 81, 81))

    @staticmethod
    def stem_max(env):
        return env["s"].reshape(env["s"].shape[0], env["s"].shape[1], 81).max(axis=-1)

    def masked_board(self, env):
        return int(np.argmax(self.stem_max(env)[:, self.gch]))

    def rt_of(self, env):
        """The run-time bias [N,Hb,81,81] in float64 from the exact stem; asserted exact in float32."""
        g = self.stem_max(env)
        assert rm.on_grid(g, self.exp)
        if self.kind == "rows":
            b = np.einsum("nhk,kj->nhj", g.reshape(g.shape[0], self.Hb, -1), self.W).reshape(g.shape[0], -1)
        else:
            b = g @ self.W
        assert rm.on_grid(b, self.exp + self.wexp) and np.array_equal(b, b.astype(np.float32))
        b = b + self.c[None]
        if self.thr is not None:
            z = 1.0 - 16.0 * (g[:, self.gch:self.gch + 1] - self.thr) * self.closed(self.Hb).reshape(1, -1)
            assert ((z >= 1.0) | (z <= -1.0)).all()  # so Clip gives exactly 0 or 1
            b = b + np.where(z <= 0.0, -np.inf, 0.0)
        return b.reshape(g.shape[0], self.Hb, 81, 81)

    def inputs(self, x):
        env = self.net.known(x)
        self._rt = self.rt_of(env)
        inp = super().inputs(x)  # exact: asserts that the final scores (self.scores below) are exact in float32
        inp["rt"] = self._rt
        return inp

    def bound(self, inp):
        """AttCase.bound, with the score's error delta carrying the constant Add's and the two added roundings."""
        if self.exact:
            return super().bound(inp)
        q, k, v, d = inp["q"], inp["k"], inp["v"], self.d
        rs = 1.0 if self.rt_scale is None else self.rt_scale  # a power of two: it rounds nothing
        assert rs > 0 and np.log2(rs) == np.round(np.log2(rs))
        qk = np.einsum("nqhd,nkhd->nhqk", q, k)
        aqk = np.einsum("nqhd,nkhd->nhqk", np.abs(q), np.abs(k))
        s = self.scores(q, k)
        closed = np.isneginf(s)
        sf = np.where(closed, 0.0, s)
        rt = np.where(np.isfinite(inp["rt"]), inp["rt"], 0.0)
        t1 = self.scale * qk
        e_t = self.scale * (gamma(d) * aqk + U * (np.abs(qk) + gamma(d) * aqk))
        delta = e_t
        if self.bias is not None:
            delta = delta + U * (np.abs(t1 + self.bias[None]) + delta)       # fl(t1 + bias)
        delta = delta + U * np.abs(rt)                                        # fl(rtScale rt) (0 for a power of two)
        delta = rs * (delta + U * (np.abs(sf) / rs + delta))                  # fl(t2 + that), then the units of s
        m = s.max(axis=-1, keepdims=True)
        assert np.isfinite(m).all()
        a = np.where(closed, -np.inf, sf - m)
        top = np.take_along_axis(delta, s.argmax(axis=-1)[..., None], axis=-1)
        near = ~closed & (sf + delta >= m - top)
        Dm = np.where(near, delta, 0.0).max(axis=-1, keepdims=True)
        assert float(Dm.max()) < 0.1
        with np.errstate(invalid="ignore", over="ignore"):
            eps = delta + U * (np.abs(a) + delta + Dm)
            gone = closed | (a + eps + Dm < -87.0)
            r = np.where(gone, 0.0, np.expm1(np.where(gone, 0.0, eps)) * (1 + 4 * U) + 4 * U)
            floor = np.where(closed, 0.0, np.where(gone, 2.0 ** -125, 0.0)) * np.exp(Dm)
        e = np.exp(a)
        p = e / e.sum(axis=-1, keepdims=True)
        R = (p * r).sum(axis=-1, keepdims=True)
        A = floor.sum(axis=-1, keepdims=True) * np.exp(Dm)
        low = (1.0 - R - A) * (1.0 - gamma(81))
        assert float(low.min()) > 0.5
        dp = p * ((1 + r) * (1 + U) / low - 1.0) + np.where(gone & ~closed, p, 0.0) + floor / low
        av = np.abs(v)
        out = np.einsum("nhqk,nkhd->nqhd", dp, av) + gamma(81) * np.einsum("nhqk,nkhd->nqhd", p + dp, av)
        return out.reshape(-1, 81, self.F)

    def scores(self, q, k, scale=None, bias="own"):
        s = super().scores(q, k, scale, bias) + self._rt
        return s if self.rt_scale is None else s * self.rt_scale

    def emulate(self, inp, fault=None):
        """A plain float32 evaluation in the kernel's order contract: acc scale, + bias, + rtScale rt."""
        f = np.float32
        q, k, v = (inp[n].astype(f) for n in "qkv")
        rs = f(1.0 if self.rt_scale is None else self.rt_scale)
        rt = np.broadcast_to(inp["rt"].astype(f), (q.shape[0], self.H, 81, 81))
        if fault == "rt_transposed":
            rt = rt.transpose(0, 1, 3, 2)
        if fault == "rt_previous_head":
            rt = np.roll(rt, 1, axis=1)
        if fault == "rt_board0":
            rt = np.broadcast_to(rt[:1], rt.shape)
        s = np.einsum("nqhd,nkhd->nhqk", q, k) * (f(self.scale) * rs)
        if self.bias is not None:
            s = s + (self.bias.astype(f) * rs)[None]
        s = s + (rt if fault == "rt_scale_dropped" else rs * rt)
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(s - s.max(axis=-1, keepdims=True))
            p = e / e.sum(axis=-1, keepdims=True, dtype=f)
            return np.einsum("nhqk,nkhd->nqhd", p, v).reshape(-1, 81, self.F)

    def single_rows(self):
        """policy mask [2187] of the outputs whose (head, query) keeps exactly one key, and that key per output."""
        assert self.mask or self.thr is not None
        # (the masked head rows share one constant row, so every head keeps head 0's key)
        shut = np.broadcast_to(self.closed(1 if self.kind == "rows" else self.Hb), (self.H, 81, 81))
        key = np.argmax(~shut, axis=-1)  # [H,81]
        h = self.ch // self.d
        return np.ones(rm.WIN * 81, bool), key[h].reshape(-1)
