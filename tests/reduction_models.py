"""Hand-built ONNX models that show the output of the general graph path's reduction kernels (graphAttention,
graphLayerNorm, graphRmsNorm, graphGroupNorm) unmixed, their float64 references, the per-element error bounds and a
float32 emulation with injectable faults: the shared half of tests/test_reduction_reference.py (host) and
tests/test_gpu_reduction_edges.py (device).

Every model is the exact stem of elt_models.Net (weights and bias small integers times 2^exp, zero on the four
fractional planes: its float32 output is exact in any order of summation), views of it (token rows, Split parts, the
global max over the squares for a flat tensor: all exact), ONE launch of the kernel under test, and a policy that
passes the kernel's output through nothing that rounds: Flatten of 27 channels where the width is 27, otherwise a
Linear / 1x1 conv / Gemm whose weight is a 0/1 selection with zero bias (products by 0 and 1 and sums of zeros are
exact for finite values; a non-finite value anywhere in the selected rows, pad channels included, would come out as
NaN).  Value and draw read the mean of the stem, as in elt_models, and are held to the siblings' 1e-4.

The bounds.  u = 2^-24, gamma(n) = n u / (1 - n u).  Inputs are exact, so every term is a rounding of the kernel:

  * a sum or dot product of n terms, in any order, with or without FMA: |err| <= gamma(n) sum|a_i b_i|;
  * one rounding (relative u) for each multiply, add, divide and square root (correctly rounded divide and sqrtf);
  * expf within 2 ulps (the project asserts twice its measured 0.58): relative 4u, and below 2^-126 an absolute 2^-125.

  Attention, per (board, head), q k v exact, s = scale q.k + bias:
    delta_ij = e_t + u (|s| + e_t),  e_t = scale (gamma(d) sum|q k| + u (|q.k| + gamma(d) sum|q k|))     the score
    (delta = 0 where the scores are exact in float32: d = 4, 16, 64 with a bias on the grid; asserted, not assumed)
    eps_j = delta_j + u (|s_j - m| + delta_j + Dm)      the argument of expf; a common shift of the row cancels in
                                                        the softmax, so the error of the maximum enters only here
    r_j = expm1(eps_j) (1 + 4u) + 4u                    the relative error of e_j (first order: delta_j, so a score
                                                        off by delta moves p_j by about 2 delta p_j with the sum's)
    R = sum_l p_l r_l                                   the relative error of the sum of the e_l, plus gamma(81)
    dp_j = p_j ((1 + r_j)(1 + u) / ((1 - R - A)(1 - gamma(81))) - 1) + abs_j       A, abs_j: the underflow floor
    |o - o64| <= sum_j dp_j |v_j| + gamma(81) sum_j (p_j + dp_j) |v_j|
    A key with bias -inf has e = 0 exactly; a row with one open key has p = 1 and o = v bit for bit.

  LayerNorm / GroupNorm over n elements (two-pass, biased variance), d = x - mean, w = var + eps, inv = w^-1/2:
    dm = gamma(n) sum|x| / n + u |mean|                 the mean; it divides by sigma below, which is why an input
    dd = dm + u (|d| + dm)                              offset by 512 has a bound 2^9 times the centred one's
    dw = (sum(2 |d| dd + dd^2) + gamma(n+1) sum(|d| + dd)^2) / n + 2u w       (dw >= w / 2: no bound; the row is constant
    rinv = (1 - dw / w)^-1/2 (1 + u) / (1 - u) - 1                             and is compared bit for bit instead)
    |y - y64| <= |g| inv (|d| rinv + dd (1 + rinv)) + 3u |g| (|d| + dd) inv (1 + rinv) + u |beta|
    ReLU behind it is exact and 1-Lipschitz: the same bound.

  RMSNorm: every term of sum x^2 is positive, so w = mean(x^2) + eps is relative: rw = (1 + gamma(n+1))(1 + u)^2 - 1,
    rinv as above with rw for dw / w, |y - y64| <= |y64| ((1 + rinv)(1 + u)^2 - 1).

The emulation (`emulate`) is a float32 numpy evaluation of the definitions -- numpy's own order in the matrix products,
one element after another in the normalisations' sums, no copy of the kernels -- and takes one fault by name (FAULTS);
tests/test_reduction_reference.py holds it inside the bound on every case and outside it, with each fault, on the case
built for that fault.

What the bound is worth.  On zero-centred input it is a few 1e-6 of y.  On a group or row offset by 512 it is the
mean's any-order error over sigma: about 512 gamma(n) / sigma, which for the shifted GroupNorm groups (n = 648 .. 1944,
sigma about 0.4) is 0.3 to 1.4 on outputs of order 1.  Those elements are held against gross faults only (E[x^2] -
mean^2, a neighbour's statistics, an index off by a channel); the unshifted groups of the same launch, the centred
cases and the bit-exact anchors carry the precision."""
import numpy as np

import elt_models as em

U = 2.0 ** -24
WIN = 27  # channels a policy shows


def gamma(n):
    return n * U / (1.0 - n * U)


class RNet(em.Net):
    """elt_models.Net that remembers which nodes its float64 interpreter knows (the stem, its views and the heads):
    `known` evaluates those and leaves the kernel under test to the references below."""

    def __init__(self, nsg):
        super().__init__(nsg)
        self.mark, self.known_names = True, set()

    def node(self, op, ins, outs, name=None, **attrs):
        r = super().node(op, ins, outs, name, **attrs)
        if self.mark:
            self.known_names.add(self.nodes[-1][4])
        return r

    def tokens(self, x, C, out):
        """[N,C,9,9] -> [N,C,81] -> [N,81,C]: views, no launch."""
        self.node("Reshape", [x, self.const(out + "_to3", [-1, C, 81], np.int64)], out + "_c3")
        return self.node("Transpose", [out + "_c3"], out, perm=[0, 2, 1])

    def heads_of(self, x, width, seed=1):
        rng = np.random.default_rng(seed)
        self.node("GlobalAveragePool", [x], "gp", name="gap")
        self.node("Flatten", ["gp"], "gpf", name="gflat", axis=1)
        for out in ("value", "draw"):
            self.const(out + "_w", rng.normal(size=(1, width)) * 0.2)
            self.const(out + "_b", [0.1])
            self.node("Gemm", ["gpf", out + "_w", out + "_b"], out + "_z", name=out + "_fc", transB=1)
            self.node("Sigmoid", [out + "_z"], out, name=out + "_sig")

    def known(self, x):
        """The float64 values of every tensor the interpreter knows, on planes x."""
        sub = em.Net.__new__(em.Net)
        sub.consts, sub.nodes = self.consts, [n for n in self.nodes if n[4] in self.known_names]
        return sub.run(x, rounded=False)


def on_grid(a, exp):
    """Multiples of 2^exp below 2^24 steps: float32 holds them, and their sums, exactly."""
    s = np.asarray(a) * 2.0 ** -exp
    return bool((s == np.round(s)).all()) and float(np.abs(s).max()) < 2 ** 24


def window(width, start):
    """The 27 channels a policy shows: start, start + 1, ... modulo the width."""
    return (start + np.arange(WIN)) % width


def starts(width):
    """Window starts that between them show every channel of `width`."""
    return list(range(0, width, WIN))


class Case:
    """One model: `data` (the ONNX bytes), `net`, and on planes x: inputs(x) -> the kernel's exact inputs,
    ref / bound / emulate on those -> the kernel's whole output, select(out) -> the [N,2187] policy."""
    kind = None

    def expected(self, x):
        inp = self.inputs(x)
        return inp, self.select(self.ref(inp)), self.select(self.bound(inp))


def ratio(got, ref, bound):
    """The largest error / bound over the elements with a finite bound; an element at bound 0 must be exact."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    fin = np.isfinite(bound)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.nan_to_num(r[fin], nan=np.inf).max()) if fin.any() else 0.0


def exact_where_unbounded(case, got, ref, bound):
    """A LayerNorm / GroupNorm element without a bound lies in a constant row: the reference is beta there, bit for bit."""
    inf = ~np.isfinite(bound)
    if inf.any():
        assert case.kind in ("layernorm", "groupnorm")
        np.testing.assert_array_equal(np.asarray(got)[inf], ref[inf].astype(np.float32))


# ---- attention -------------------------------------------------------------------------------------------------------
def att_bias(kind, H, seed):
    """[H,81,81] on the grid of 1/16.  "grid": -2..0, no symmetry.  "causal_inf" / "causal_1e9": head h even keeps
    keys <= query, h odd keys >= query; every ninth query row keeps one key only, (5 row + 3) % 81 (rows 0 of the even
    heads and 80 of the odd ones keep one key by the pattern itself)."""
    rng = np.random.default_rng(100 + seed)
    b = rng.integers(-32, 1, size=(H, 81, 81)) / 16.0
    if kind == "grid":
        return b
    fill = -np.inf if kind == "causal_inf" else -1e9
    i, j = np.arange(81)[:, None], np.arange(81)[None, :]
    for h in range(H):
        closed = (j > i) if h % 2 == 0 else (j < i)
        b[h][np.where(i % 9 == 4, j != (5 * i + 3) % 81, closed)] = fill
    return b


def open_keys(bias):
    return (bias > -1e8).sum(axis=-1)  # [H,81]


class AttCase(Case):
    kind = "attention"

    def __init__(self, nsg, F, H, exp=-3, seed=0, offs=None, bias="grid", start=0, stem=64, span=1, exact=False):
        """q, k, v: F channels each of one `stem`-wide token row at offsets offs = (q, k, v); three Split nodes of the
        same tensor give views that may overlap.  exact: the scores are exact in float32 (asserted in inputs)."""
        self.F, self.H, self.d, self.exp, self.exact, self.start = F, H, F // H, exp, exact, start
        self.offs = offs if offs is not None else (0, (stem - F) // 2 // 4 * 4, stem - F)
        self.scale = float(np.float32(self.d ** -0.5))
        self.bias = None if bias is None else att_bias(bias, H, seed).astype(np.float32).astype(np.float64)
        self.bias_kind = bias
        net = self.net = RNet(nsg)
        net.stem(stem, seed, exp, span)
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
        net.const("to4", [-1, 81, H, self.d], np.int64)
        q4, k4, v4 = (net.node("Reshape", [views[off], "to4"], nm + "4") for nm, off in zip("qkv", self.offs))
        qh = net.node("Transpose", [q4], "qh", perm=[0, 2, 1, 3])
        kt = net.node("Transpose", [k4], "kt", perm=[0, 2, 3, 1])
        vh = net.node("Transpose", [v4], "vh", perm=[0, 2, 1, 3])
        a = net.node("MatMul", [qh, kt], "qk")
        a = net.node("Mul", [a, net.const("scale", [self.scale])], "scaled")
        if self.bias is not None:
            a = net.node("Add", [a, net.const("rel", self.bias)], "biased")
        p = net.node("Softmax", [a], "probs", axis=-1)
        o = net.node("MatMul", [p, vh], "oh")
        o = net.node("Transpose", [o], "ot", perm=[0, 2, 1, 3])
        o = net.node("Reshape", [o, net.const("to3", [-1, 81, F], np.int64)], "att")
        self.ch = window(F, start)
        sel = np.zeros((F, WIN))
        sel[self.ch, np.arange(WIN)] = 1.0
        net.node("MatMul", [o, net.const("sel", sel)], "picked", name="select")
        net.node("Transpose", ["picked"], "pt", perm=[0, 2, 1])
        net.node("Reshape", ["pt", net.const("to2", [-1, WIN * 81], np.int64)], "policy", name="pflat")
        net.mark = True
        net.heads_of("s", stem)
        self.data = net.data()

    def inputs(self, x):
        env = self.net.known(x)
        tok = env["tok"]
        assert on_grid(tok, self.exp)
        N = tok.shape[0]
        q, k, v = (tok[:, :, off:off + self.F].reshape(N, 81, self.H, self.d) for off in self.offs)
        if self.exact:  # q.k is a sum of multiples of 4^exp, the scale a power of two, the bias on the grid of 1/16
            assert self.d in (4, 16, 64) and self.scale == self.d ** -0.5
            s = self.scores(q, k)
            assert on_grid(s[np.isfinite(s)], 2 * self.exp - 3 - 4) and np.array_equal(s, em.f32(s))
        return dict(q=q, k=k, v=v, env=env)

    def scores(self, q, k, scale=None, bias="own"):
        s = (self.scale if scale is None else scale) * np.einsum("nqhd,nkhd->nhqk", q, k)
        b = self.bias if isinstance(bias, str) else bias
        return s if b is None else s + b[None]

    def ref(self, inp):
        s = self.scores(inp["q"], inp["k"])
        e = np.exp(s - s.max(axis=-1, keepdims=True))
        p = e / e.sum(axis=-1, keepdims=True)
        return np.einsum("nhqk,nkhd->nqhd", p, inp["v"]).reshape(-1, 81, self.F)

    def bound(self, inp):
        q, k, v, d = inp["q"], inp["k"], inp["v"], self.d
        qk = np.einsum("nqhd,nkhd->nhqk", q, k)
        aqk = np.einsum("nqhd,nkhd->nhqk", np.abs(q), np.abs(k))
        s = self.scores(q, k)
        closed = np.isneginf(s)
        sf = np.where(closed, 0.0, s)
        if self.exact:
            delta = np.zeros_like(sf)
        else:
            e_t = self.scale * (gamma(d) * aqk + U * (np.abs(qk) + gamma(d) * aqk))
            delta = e_t + (U * (np.abs(sf) + e_t) if self.bias is not None else 0.0)
        m = s.max(axis=-1, keepdims=True)
        assert np.isfinite(m).all()
        a = np.where(closed, -np.inf, sf - m)
        # the kernel's maximum is some computed score: one whose true value is within its delta of the true maximum
        top = np.take_along_axis(delta, s.argmax(axis=-1)[..., None], axis=-1)
        near = ~closed & (sf + delta >= m - top)
        Dm = np.where(near, delta, 0.0).max(axis=-1, keepdims=True)
        assert float(Dm.max()) < 0.1
        with np.errstate(invalid="ignore", over="ignore"):
            eps = delta + U * (np.abs(a) + delta + Dm)
            gone = closed | (a + eps + Dm < -87.0)  # below 2^-126 (or exactly zero): an absolute error only
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

    def emulate(self, inp, fault=None):
        f = np.float32
        q, k, v = (inp[n].astype(f) for n in "qkv")
        scale = f(1.0) if fault == "scale_dropped" else f(self.scale)
        s = np.einsum("nqhd,nkhd->nhqk", q, k) * scale
        if self.bias is not None:
            b = self.bias.astype(f)
            s = s + (b.transpose(0, 2, 1) if fault == "bias_transposed" else b)[None]
        if fault == "pad_keys":  # keys 81..95 as zero scores
            s = np.concatenate([s, np.zeros(s.shape[:3] + (15,), f)], axis=-1)
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(s if fault == "no_max" else s - s.max(axis=-1, keepdims=True))
            p = (e / e.sum(axis=-1, keepdims=True, dtype=f))[..., :81]
            if fault == "previous_head_v":
                v = np.roll(v, 1, axis=2)
            return np.einsum("nhqk,nkhd->nqhd", p, v).reshape(-1, 81, self.F)

    def select(self, out):
        """[N,81,F] -> policy[n, j * 81 + sq] = out[n, sq, ch[j]]"""
        return out[:, :, self.ch].transpose(0, 2, 1).reshape(out.shape[0], -1)

    def single_rows(self):
        """policy mask [2187] of the outputs whose (head, query) keeps exactly one key, and that key per output."""
        one = open_keys(self.bias) == 1  # [H,81]
        key = np.argmax(self.bias > -1e8, axis=-1)  # [H,81]
        h = self.ch // self.d
        return one[h].reshape(-1), key[h].reshape(-1)


# ---- the normalisations ----------------------------------------------------------------------------------------------
def norm_ref(x, g, b, eps, rms=False):
    d = x if rms else x - x.mean(axis=-1, keepdims=True)
    return d / np.sqrt((d * d).mean(axis=-1, keepdims=True) + eps) * g + b


def norm_bound(x, g, b, eps, rms=False):
    n = x.shape[-1]
    with np.errstate(invalid="ignore", divide="ignore"):
        if rms:
            rw = (1 + gamma(n + 1)) * (1 + U) ** 2 - 1
            rinv = (1 - rw) ** -0.5 * (1 + U) / (1 - U) - 1
            return np.abs(norm_ref(x, g, b, eps, True)) * ((1 + rinv) * (1 + U) ** 2 - 1)
        mean = x.mean(axis=-1, keepdims=True)
        d = np.abs(x - mean)
        e_s = gamma(n) * np.abs(x).sum(axis=-1, keepdims=True) / n
        dm = e_s + U * (np.abs(mean) + e_s)
        dd = dm + U * (d + dm)
        w = (d * d).mean(axis=-1, keepdims=True) + eps
        dv = ((2 * d * dd + dd * dd).sum(axis=-1, keepdims=True) + gamma(n + 1) * ((d + dd) ** 2).sum(axis=-1, keepdims=True)) / n
        dw = dv * (1 + 2 * U) + 2 * U * (w + dv)
        ok = dw < 0.5 * w  # beyond that first-order reasoning about 1 / sqrt(w) says nothing: no bound
        rinv = np.where(ok, (1 - np.where(ok, dw / w, 0.0)) ** -0.5 * (1 + U) / (1 - U) - 1, np.inf)
        inv = w ** -0.5
        return np.abs(g) * inv * (d * rinv + dd * (1 + rinv)) + ((1 + U) ** 3 - 1) * np.abs(g) * (d + dd) * inv * (1 + rinv) + U * (1 + U) * np.abs(b)


def norm_emulate(x, g, b, eps, rms=False, fault=None, neighbour=None):
    """float32; neighbour: the same rows rolled by one group, whose elements join the statistics (fault)."""
    f = np.float32
    x, g, b, eps = x.astype(f), np.asarray(g, f), np.asarray(b, f), f(eps)

    def total(a):  # one element after another, each partial sum rounded to float32
        return np.cumsum(a, axis=-1, dtype=f)[..., -1:]

    pool = x if fault != "neighbour_group" else np.concatenate([x, neighbour.astype(f)], axis=-1)
    n = f(pool.shape[-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        if rms:
            var, d = total(pool * pool) / n, x
        else:
            mean = total(pool) / n
            d, dp = x - mean, pool - mean
            if fault == "one_pass_variance":
                var = total(pool * pool) / n - mean * mean
            else:
                var = total(dp * dp) / (n - f(1) if fault == "unbiased_variance" else n)
        inv = f(1) / (np.sqrt(var) + eps) if fault == "eps_outside_sqrt" else f(1) / np.sqrt(var + eps)
        return d * inv * g + b


def affine(C, seed, beta=True):
    rng = np.random.default_rng(200 + seed)
    g = em.f32(rng.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 5 == 0, -1.0, 1.0))
    b = em.f32(rng.normal(size=C)) if beta else np.zeros(C)
    return g, b


class RowNormCase(Case):
    """LayerNorm or RMSNorm over C channels read at channel `off` of the stem's rows, on token rows or on the flat
    [N, off + C] global max of the stem.  variant: "centred" | "offset" (every channel + 512) | "constant" (every
    channel has the filter and bias of channel `off`, so each row is one value, another in every row)."""

    def __init__(self, nsg, op, domain, C, variant, eps, start=0, off=3, exp=-4, seed=0):
        self.kind, self.domain, self.C, self.variant, self.eps, self.off, self.exp = op, domain, C, variant, float(np.float32(eps)), off, exp
        self.rms = op == "rmsnorm"
        W = off + C
        net = self.net = RNet(nsg)
        net.stem(W, seed + C, exp)
        w, bs = net.consts["s_w"], net.consts["s_b"]
        if variant == "offset":
            bs[off:] += 512.0
        if variant == "constant":
            w[off:], bs[off:] = w[off], bs[off]
        self.g, self.b = affine(C, C, beta=not self.rms)
        if domain == "token":
            x = net.tokens("s", W, "tok")
            axis = 2
        else:
            net.mark = False
            net.node("GlobalMaxPool", ["s"], "gm", name="gmax")
            x = net.node("Flatten", ["gm"], "flat", axis=1)
            axis = 1
        net.mark = False
        net.const("sizes", [off, C], np.int64)
        x = net.node("Split", [x, "sizes"], ["lead", "x"], name="split", axis=axis)[1]
        if self.rms:
            sq = net.node("Mul", [x, x], "sq")
            ms = net.node("ReduceMean", [sq], "ms", axes=[-1], keepdims=1)
            rt = net.node("Sqrt", [net.node("Add", [ms, net.const("eps", [self.eps])], "mse")], "rt")
            y = net.node("Mul", [net.node("Div", [x, rt], "xn"), net.const("gamma", self.g)], "y")
        else:
            y = net.node("LayerNormalization", [x, net.const("gamma", self.g), net.const("beta", self.b)], "y", axis=-1, epsilon=self.eps)
        if domain == "token":
            self.ch = window(C, start)
            sel = np.zeros((C, WIN))
            sel[self.ch, np.arange(WIN)] = 1.0
            net.node("MatMul", [y, net.const("sel", sel)], "picked", name="select")
            net.node("Transpose", ["picked"], "pt", perm=[0, 2, 1])
            net.node("Reshape", ["pt", net.const("to2", [-1, WIN * 81], np.int64)], "policy", name="pflat")
        else:
            self.ch = np.arange(WIN * 81) % C  # every channel, 2187 / C times
            sel = np.zeros((WIN * 81, C))
            sel[np.arange(WIN * 81), self.ch] = 1.0
            net.node("Gemm", [y, net.const("sel", sel)], "policy", name="select", transB=1)
        net.mark = True
        net.heads_of("s", W)
        self.data = net.data()

    def inputs(self, x):
        env = self.net.known(x)
        s = env["s"]
        assert on_grid(s, self.exp)
        if self.domain == "token":
            rows = s.reshape(s.shape[0], s.shape[1], 81).transpose(0, 2, 1)[:, :, self.off:]
        else:
            rows = s.max(axis=(2, 3))[:, self.off:]
        mean, sd = rows.mean(axis=-1), rows.std(axis=-1)
        if self.variant == "offset":
            assert float((np.abs(mean) / sd).min()) >= 2 ** 9, float((np.abs(mean) / sd).min())
        if self.variant == "constant":
            assert float(sd.max()) == 0.0 and len(np.unique(mean)) > (8 if self.domain == "token" else 3)
        else:  # a few rows of a narrow width may be constant by chance: they are compared as the constant rows are
            assert float((sd > 0.1).mean()) > 0.9, float((sd > 0.1).mean())
        return dict(x=rows, env=env)

    def ref(self, inp):
        return norm_ref(inp["x"], self.g, self.b, self.eps, self.rms)

    def bound(self, inp):
        return norm_bound(inp["x"], self.g, self.b, self.eps, self.rms)

    def emulate(self, inp, fault=None):
        return norm_emulate(inp["x"], self.g, self.b, self.eps, self.rms, fault)

    def select(self, out):
        if self.domain == "token":
            return out[:, :, self.ch].transpose(0, 2, 1).reshape(out.shape[0], -1)
        return out[:, self.ch]


class GroupNormCase(Case):
    """GroupNorm as the exporter writes it (Reshape, InstanceNormalization, Reshape, Mul, Add) and an optional ReLU,
    on C channels at channel `off` of the stem.  Groups 1, 3, 5, ... (group 0 when there is one group) are offset by
    `shift` = 512, with |mean| / sigma >= shift asserted; `constant`: that group has zero weights and one bias, so its
    81 Cg elements are one value.  The one group of 200 channels is offset by 64, not 512: over n = 16200 elements the
    any-order bound of the mean, gamma(n) 512 = 0.5, exceeds sigma (0.4) and leaves no bound on y at all.  64 is the
    largest power of two at which every board keeps a bound (at 128 some lose it); E[x^2] - mean^2 falls outside it
    (both asserted in tests/test_reduction_reference.py).  eps is the default 1e-5, as for the other shapes."""
    kind = "groupnorm"

    def __init__(self, nsg, C, G, eps=1e-5, start=0, off=0, relu=False, constant=None, offset=True, exp=-4, seed=0, shift=512.0):
        self.C, self.G, self.Cg, self.eps, self.off, self.relu, self.exp = C, G, C // G, float(np.float32(eps)), off, relu, exp
        self.constant, self.shift = constant, shift
        W = off + C
        net = self.net = RNet(nsg)
        net.stem(W, seed + C + G, exp)
        w, bs = net.consts["s_w"], net.consts["s_b"]
        self.shifted = [g for g in range(G) if offset and (g % 2 == 1 or G == 1) and g != constant]
        for g in self.shifted:
            bs[off + g * self.Cg: off + (g + 1) * self.Cg] += shift
        if constant is not None:
            w[off + constant * self.Cg: off + (constant + 1) * self.Cg] = 0.0
            bs[off + constant * self.Cg: off + (constant + 1) * self.Cg] = 1.25
        self.g, self.b = affine(C, C + G)
        net.mark = False
        x = "s"
        if off:
            net.const("sizes", [off, C], np.int64)
            x = net.node("Split", ["s", "sizes"], ["lead", "x"], name="split", axis=1)[1]
        net.node("Reshape", [x, net.const("to_groups", [0, G, -1], np.int64)], "grouped")
        net.node("InstanceNormalization", ["grouped", net.const("ones", np.ones(G)), net.const("zeros", np.zeros(G))], "normed", epsilon=self.eps)
        net.node("Reshape", ["normed", net.const("back", [0, C, 9, 9], np.int64)], "n4")
        y = net.node("Add", [net.node("Mul", ["n4", net.const("gamma", self.g.reshape(C, 1, 1))], "scaled"), net.const("beta", self.b.reshape(C, 1, 1))], "y")
        if relu:
            y = net.node("Relu", [y], "act")
        if C == WIN:
            self.ch = np.arange(WIN)
            net.node("Flatten", [y], "policy", name="pflat", axis=1)
        else:
            self.ch = window(C, start)
            sel = np.zeros((WIN, C, 1, 1))
            sel[np.arange(WIN), self.ch] = 1.0
            net.node("Conv", [y, net.const("sel", sel)], "picked", name="select", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
            net.node("Flatten", ["picked"], "policy", name="pflat", axis=1)
        net.mark = True
        net.heads_of("s", W)
        self.data = net.data()

    def grouped(self, a):
        """[N,C,81] -> [N,G,Cg*81]"""
        return a.reshape(a.shape[0], self.G, self.Cg * 81)

    def inputs(self, x):
        env = self.net.known(x)
        s = env["s"]
        assert on_grid(s, self.exp)
        rows = self.grouped(s.reshape(s.shape[0], s.shape[1], 81)[:, self.off:])
        mean, sd = rows.mean(axis=-1), rows.std(axis=-1)
        for g in range(self.G):
            if g == self.constant:
                assert float(sd[:, g].max()) == 0.0
            else:
                assert float(sd[:, g].min()) > 0.05, (g, float(sd[:, g].min()))
                if g in self.shifted:
                    assert float((np.abs(mean[:, g]) / sd[:, g]).min()) >= self.shift
        return dict(x=rows, env=env)

    def per_element(self, v):
        return self.grouped(np.broadcast_to(v.reshape(1, self.C, 1), (1, self.C, 81)))

    def act(self, y):
        return np.maximum(y, 0.0) if self.relu else y

    def ref(self, inp):
        return self.act(norm_ref(inp["x"], self.per_element(self.g), self.per_element(self.b), self.eps))

    def bound(self, inp):
        return norm_bound(inp["x"], self.per_element(self.g), self.per_element(self.b), self.eps)

    def emulate(self, inp, fault=None):
        nb = np.roll(inp["x"], -1, axis=1)
        y = norm_emulate(inp["x"], self.per_element(self.g), self.per_element(self.b), self.eps, False, fault, nb)
        return np.maximum(y, np.float32(0)) if self.relu else y

    def select(self, out):
        """[N,G,Cg*81] -> policy[n, j * 81 + sq] = out[n, ch[j], sq]"""
        return out.reshape(out.shape[0], self.C, 81)[:, self.ch].reshape(out.shape[0], -1)

    def constant_mask(self):
        """policy mask [2187] of the outputs in the constant group, and act(beta) there."""
        m = np.repeat(self.ch // self.Cg == self.constant, 81)
        return m, np.repeat(self.act(self.b)[self.ch], 81)


# ---- the cases of tests/test_gpu_reduction_edges.py, by id -------------------------------------------------------------
# attention: id -> keyword arguments of AttCase; one entry per window start
ATT_SHAPES = {
    # d: (F, H, extra)
    "d4": dict(F=16, H=4, exact=True),
    "d12": dict(F=24, H=2),
    "d20": dict(F=40, H=2),
    "d24": dict(F=48, H=2),
    "d40": dict(F=40, H=1),
    "d48": dict(F=48, H=1),
    "d16": dict(F=32, H=2, exact=True),
    "d64_same_view": dict(F=64, H=1, exact=True, offs=(0, 0, 0)),
    "big_scores": dict(F=32, H=2, exact=True, exp=0, span=2, seed=3),
    "masked_inf": dict(F=24, H=2, bias="causal_inf", seed=5),
    "masked_1e9": dict(F=24, H=2, bias="causal_1e9", seed=5),
    "views": dict(F=16, H=2, offs=(24, 44, 4), seed=7),
}


def att_cases():
    return [(name, st) for name, kw in ATT_SHAPES.items() for st in starts(kw["F"])]


def att_case(nsg, name, start=0):
    return AttCase(nsg, start=start, **ATT_SHAPES[name])


ROW_WIDTHS = [4, 24, 64, 65, 72, 136]
ROW_VARIANTS = {"centred": ("centred", 1e-2), "offset": ("offset", 1e-5), "constant_eps5": ("constant", 1e-5),
                "constant_eps12": ("constant", 1e-12)}


def row_case(nsg, op, domain, C, variant, start=0):
    v, eps = ROW_VARIANTS[variant]
    return RowNormCase(nsg, op, domain, C, v, eps, start=start)


GN_SHAPES = {
    "24x3": dict(C=24, G=3), "24x24": dict(C=24, G=24, relu=True), "24x1": dict(C=24, G=1), "27x3": dict(C=27, G=3, relu=True),
    "72x8": dict(C=72, G=8), "200x1": dict(C=200, G=1, relu=True, shift=64.0), "24x3_at6": dict(C=24, G=3, off=6, relu=True),
    "24x3_const_eps5": dict(C=24, G=3, constant=2, relu=True), "24x3_const_eps12": dict(C=24, G=3, constant=0, eps=1e-12),
    "72x8_const_eps12": dict(C=72, G=8, constant=5, eps=1e-12, relu=True),
    "24x3_centred": dict(C=24, G=3, offset=False, eps=1e-2),
}


def gn_cases():
    return [(name, st) for name, kw in GN_SHAPES.items() for st in (starts(kw["C"]) if kw["C"] != WIN else [0])]


def gn_case(nsg, name, start=0):
    return GroupNormCase(nsg, start=start, **GN_SHAPES[name])


# fault -> the case built for it
ATT_FAULTS = {"no_max": "big_scores", "pad_keys": "d12", "scale_dropped": "d12", "bias_transposed": "d12", "previous_head_v": "d12"}
NORM_FAULTS = ["one_pass_variance", "unbiased_variance", "neighbour_group", "eps_outside_sqrt"]
FAULTS = list(ATT_FAULTS) + NORM_FAULTS

ATT = att_cases()
ROWS = [(op, dom, C, v) for op in ("layernorm", "rmsnorm") for dom in ("token", "flat") for C in ROW_WIDTHS for v in ROW_VARIANTS]
GN = gn_cases()
