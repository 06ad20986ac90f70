"""Hand-built ONNX models that show the output of the general graph path's oldest kernels unmixed -- graphConv<9> and
graphConv<1> (conv and dense layer), graphConvGeo and graphDepthwise of graph_conv.hip, graphPool of graph_pool.hip --
with their float64 references, per-element bounds, a plain float32 evaluation and named faults: the shared half of
tests/test_conv_reference.py (host) and tests/test_gpu_conv_edges.py (device).  DESIGN.md 13.6.1 says what each case is
for.

Every model is the exact stem of elt_models.Net (weights and bias small integers times 2^-3, zero on the four
fractional planes: its float32 output is exact in any order of summation), views of it, ONE launch of the kernel under
test (node "kut"; a fused residual Add "kadd" and ReLU "kact" ride in it) and a policy that does not round: Flatten
where the width is 27, the dense layer's own 2187 outputs, otherwise a 1x1 conv whose weight is a 0/1 selection of 27
channels, one model per window (`parts`), so that every output channel is shown.  A residual is a second exact stem
"r", whole or a Split view of it at channel 27 (an offset 4 does not divide) or 16.  Value and draw read the mean of
the kernel's input, as in the siblings.

Exact cases: integer weights from -2..2 without symmetry, an integer bias and residual on the stem's grid, activation
none or ReLU.  `inputs` asserts in float64 that sum|x w| + |b| + |res| stays below 2^24 quanta for every element: every
partial sum, in any order, is then an integer below 2^24 times the quantum, float32 holds it and the bound is 0.  An
average pool's window sum is exact in the same way; its expected value is the float64 quotient rounded once to
float32, which is the correctly rounded float32 division.

Rounded cases: the same exact inputs, seeded float32 weights of order 1 / sqrt(K), K the real products of an output
(taps x cin; taps for a depthwise conv).  u = 2^-24, gamma(n) = n u / (1 - n u) as in reduction_models:

    e = gamma(K) sum|x_i w_i|                    the chain over the real products in any order (pads add exact zeros)
    d = e + u (|t| + e),  t = sum + b            the bias add
    d' = d + u (|t + r| + d)                     the residual add; ReLU is exact and 1-Lipschitz: the same bound

The bound is derived from the operands, not measured.  Operands truncated to fp16's 11 bits err by up to 2^-10 per
product, all one way: about 5e-4 sum|x w|, against gamma(K) = 2e-5 at K = 360 and 9e-7 at K = 15.

width_from_hy is the kernels' `W = 9 + 2 hx` taken as 9 + 2 hy, in the staging and in the reads alike.  Such an image is
still right whenever 2 hy >= hx (a tap past the right edge lands in the next row's left halo, which is zero too), so the
fault shows only on 3x7, 3x9, 3x3 at dilation (1,4) and 3x5 at dilation (1,2).

The references read a haloed flat image the way the kernels do (square (y, x) at (y + hy) W + x + hx, tap (ky, kx) at
+ ky dh W + kx dw), so that the faults of FAULTS can be stated as what they are; tests/test_conv_reference.py holds
them against torch's own float64 conv2d / avg_pool2d / max_pool2d / linear."""
import numpy as np

import elt_models as em
import reduction_models as rm
from reduction_models import U, WIN, gamma

EXP = -3            # the stems' grid
Q = 2.0 ** EXP
FAULTS = ["group_last_tap_dropped", "kernel_transposed", "dilations_swapped", "width_from_hy", "residual_at_offset_0",
          "include_divisor_for_exclude", "dense_row_81_repeats_row_80"]
HEAD_NAMES = {"gap", "value_fc+value_sig", "draw_fc+draw_sig"}


def halo(k, d):
    return d * (k - 1) // 2


def tap_group(taps):
    """graphConvGeo's weight groups: the fewest groups of at most 8 taps, evened out."""
    groups = -(-taps // 8)
    return -(-taps // groups)


def windows_of(x, kh, kw, dh, dw, fill=0.0, fault=None):
    """Yields (tap, [N,C,81]): what tap (ky, kx), row-major, reads for each square from the haloed image of x [N,C,9,9],
    staged and read as a flat array of row length W = 9 + 2 hx.  width_from_hy: W = 9 + 2 hy."""
    N, C = x.shape[:2]
    hy, hx = halo(kh, dh), halo(kw, dw)
    H, W = 9 + 2 * hy, (9 + 2 * hy if fault == "width_from_hy" else 9 + 2 * hx)
    p = np.arange(H * W)
    sy, sx = p // W - hy, p % W - hx
    on = (sy >= 0) & (sy < 9) & (sx >= 0) & (sx < 9)
    flat = np.full((N, C, H * W + 17 * 17), fill, x.dtype)  # past the staged image: never read without the fault
    flat[:, :, p[on]] = x[:, :, sy[on], sx[on]]
    y, xx = np.divmod(np.arange(81), 9)
    for ky in range(kh):
        for kx in range(kw):
            yield ky * kw + kx, flat[:, :, (y + ky * dh) * W + xx + kx * dw]


def conv_any(x, w, b, dh=1, dw=1, depthwise=False, fault=None):
    """The conv of x [N,Cin,9,9] with w [Cout,Cin or 1,kh,kw] and bias b, pads equal to the halo, in x's dtype, tap after
    tap; one fault by name.  Returns [N,Cout,9,9]."""
    kh, kw = w.shape[2:]
    if fault == "kernel_transposed":
        w, kh, kw = w.transpose(0, 1, 3, 2), kw, kh
    if fault == "dilations_swapped":
        dh, dw = dw, dh
    tg = tap_group(kh * kw)
    out = np.zeros((x.shape[0], w.shape[0], 81), x.dtype)
    for t, win in windows_of(x, kh, kw, dh, dw, 0.0, fault):
        if fault == "group_last_tap_dropped" and (t % tg == tg - 1 or t == kh * kw - 1):
            continue
        wt = w[:, :, t // kw, t % kw].astype(x.dtype)
        out += wt[None, :, 0, None] * win if depthwise else np.einsum("oc,ncs->nos", wt, win)
    return (out + b.astype(x.dtype)[None, :, None]).reshape(x.shape[0], -1, 9, 9)


def pool_any(x, kh, kw, dh, dw, mode, fault=None):
    """mode "max": the window's max.  "avg_include" / "avg_exclude": (the exact float64 window sum, the divisor [81])."""
    if fault == "dilations_swapped":
        dh, dw = dw, dh
    wins = [win for _, win in windows_of(x, kh, kw, dh, dw, -np.inf if mode == "max" else 0.0, fault)]
    if mode == "max":
        return np.max(wins, axis=0).reshape(x.shape)
    y, xx = np.divmod(np.arange(81), 9)
    ny = sum(((y - halo(kh, dh) + ky * dh >= 0) & (y - halo(kh, dh) + ky * dh < 9)).astype(int) for ky in range(kh))
    nx = sum(((xx - halo(kw, dw) + kx * dw >= 0) & (xx - halo(kw, dw) + kx * dw < 9)).astype(int) for kx in range(kw))
    include = mode == "avg_include" or fault == "include_divisor_for_exclude"
    return np.sum(wins, axis=0), (np.full(81, kh * kw) if include else ny * nx).astype(np.float64)


def asymmetric(w):
    """No symmetry: the weight differs from its transpose (where square), its two flips and its rotation."""
    kh, kw = w.shape[2:]
    same = [w[:, :, ::-1], w[:, :, :, ::-1], w[:, :, ::-1, ::-1]] + ([w.transpose(0, 1, 3, 2)] if kh == kw else [])
    return all(not np.array_equal(w, s) for s in same if kh * kw > 1)


class EdgeCase(rm.Case):
    """A case of this file: `parts` are the window starts, model(part) the ONNX bytes that show that window,
    select(out, part) the [N,2187] policy of the kernel's whole output; ref and emulate take the operands of inputs."""
    exact, parts, launches = True, [0], 1

    def expected(self, x, part=0):
        inp = self.inputs(x)
        return inp, self.select(self.ref(inp), part), self.select(self.bound(inp), part)

    def show(self, net, y, C, part):
        """The policy: Flatten of 27 channels, or the 0/1 selection of the window at `part`."""
        if C == WIN:
            return net.node("Flatten", [y], "policy", name="pflat", axis=1)
        sel = np.zeros((WIN, C, 1, 1))
        sel[np.arange(WIN), rm.window(C, part)] = 1.0
        net.node("Conv", [y, net.const("sel", sel)], "picked", name="select", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
        return net.node("Flatten", ["picked"], "policy", name="pflat", axis=1)

    def select(self, out, part=0):
        N, C = out.shape[:2]
        ch = np.arange(WIN) if C == WIN else rm.window(C, part)
        return out.reshape(N, C, 81)[:, ch].reshape(N, -1)

    def every_channel_shows(self, ref):
        """Every output channel takes more than one value over the boards and squares, and the windows cover them."""
        C = ref.shape[1]
        flat = ref.reshape(ref.shape[0], C, -1).transpose(1, 0, 2).reshape(C, -1)
        dull = [c for c in range(C) if float(flat[c].min()) == float(flat[c].max())]
        assert not dull, dull
        if C != WIN:
            assert sorted(set(np.concatenate([rm.window(C, p) for p in self.parts]))) == list(range(C))


# ---- graphConv<9>, graphConv<1>, graphConvGeo, graphDepthwise ---------------------------------------------------------------
class ConvCase(EdgeCase):
    """kind "tile" | "geo" | "depthwise": cin -> cout channels (cin = None: straight from the 86 planes; depthwise: cin =
    cout), kernel k = (kh, kw) at dilations d = (dh, dw).  res: None, or the channel of the second stem "r" the residual
    of cout channels starts at (0: "r" whole); relu: a ReLU behind it (the default with a residual)."""

    def __init__(self, nsg, kind, cin, cout, k=(3, 3), d=(1, 1), res=None, relu=None, exact=True, seed=0):
        self.nsg, self.kind, self.cin, self.cout, self.k, self.d, self.res, self.exact, self.seed = nsg, kind, cin, cout, k, d, res, exact, seed
        self.relu = (res is not None) if relu is None else relu
        self.planes = cin is None
        self.C = 86 if self.planes else cin
        self.depthwise = kind == "depthwise"
        assert not self.depthwise or cin == cout
        kh, kw = k
        per = 1 if self.depthwise else self.C
        self.K = kh * kw * (1 if self.depthwise else self.C - (4 if self.planes else 0))  # the real products of an output
        rng = np.random.default_rng(7000 + seed + 13 * cout + kh * 31 + kw)
        if exact:
            w = rng.integers(-2, 3, size=(cout, per, kh, kw)).astype(np.float64)
            b = rng.integers(-8, 9, size=cout) * (1.0 if self.planes else Q)
        else:
            w = em.f32(rng.normal(size=(cout, per, kh, kw)) / np.sqrt(self.K))
            b = em.f32(rng.normal(size=cout) * 0.2)
        if self.planes:
            w[:, 82:] = 0.0  # the four planes that hold fractions
        assert asymmetric(w)
        self.w, self.b = w, b
        self.parts = [0] if cout == WIN else rm.starts(cout)
        self.net = self.build(0)
        if self.relu and not self.planes:
            # Centre every channel on the ReLU's kink, from the models' own constants: the stems are their bias plus a
            # sparse zero-mean conv, so without this a channel whose weights happen to lean one way is closed (or open) on
            # every square of every board and shows nothing of the ReLU.
            c = self.net.consts
            sb = c["s_b"].astype(np.float64)
            lean = self.w.sum(axis=(1, 2, 3)) * sb if self.depthwise else self.w.sum(axis=(2, 3)) @ sb
            if self.res is not None:
                lean = lean + c["r_b"].astype(np.float64)[self.res:self.res + cout]
            self.b = em.f32(self.b - lean)
            self.net = self.build(0)

    def build(self, part):
        net = rm.RNet(self.nsg)
        (kh, kw), (dh, dw) = self.k, self.d
        x = "input" if self.planes else net.stem(self.C, self.seed, EXP)
        rv = None
        if self.res is not None:
            rv = net.stem(self.res + self.cout, self.seed + 50, EXP, out="r")
            if self.res:
                net.const("r_sizes", [self.res, self.cout], np.int64)
                rv = net.node("Split", ["r", "r_sizes"], ["r_lead", "r_view"], name="r_split", axis=1)[1]
        net.mark = False
        net.const("k_w", self.w)
        net.const("k_b", self.b)
        attrs = dict(kernel_shape=[kh, kw], pads=[halo(kh, dh), halo(kw, dw)] * 2, dilations=[dh, dw])
        if self.depthwise:
            attrs["group"] = self.cout
        y = net.node("Conv", [x, "k_w", "k_b"], "k_y", name="kut", **attrs)
        if rv is not None:
            y = net.node("Add", [y, rv], "k_sum", name="kadd")
        if self.relu:
            y = net.node("Relu", [y], "k_act", name="kact")
        self.show(net, y, self.cout, part)
        net.mark = True
        net.heads_of(x, self.C)
        return net

    def model(self, part=0):
        return self.build(part).data()

    def inputs(self, x):
        env = self.net.known(x)
        X = np.asarray(x, np.float64) if self.planes else env["s"]
        R = None if self.res is None else env["r"]
        if not self.planes:
            assert rm.on_grid(X, EXP)
        inp = dict(x=X, r=R, env=env)
        if R is not None:
            assert rm.on_grid(R, EXP)
        if self.exact:  # every partial sum of every element, in any order, is an integer below 2^24 times the quantum
            q = 1.0 if self.planes else Q  # (0/1 planes; the fractional ones meet zero weights only)
            assert self.planes or rm.on_grid(X, EXP)
            assert not self.planes or (set(np.unique(X[:, :82])) <= {0.0, 1.0} and not self.w[:, 82:].any())
            assert rm.on_grid(self.w, 0) and rm.on_grid(self.b / q, 0)
            mass = conv_any(np.abs(X), np.abs(self.w), np.abs(self.b), *self.d, self.depthwise)
            if R is not None:
                mass = mass + np.abs(self.residual(inp))
            assert float(mass.max()) / q < 2 ** 24, float(mass.max())
        return inp

    def residual(self, inp, fault=None):
        off = 0 if fault == "residual_at_offset_0" else self.res
        return inp["r"][:, off:off + self.cout]

    def ref(self, inp, fault=None):
        y = conv_any(inp["x"], self.w, self.b, *self.d, self.depthwise, fault)
        if self.res is not None:
            y = y + self.residual(inp, fault)
        return np.maximum(y, 0.0) if self.relu else y

    def bound(self, inp):
        if self.exact:
            return np.zeros((len(inp["x"]), self.cout, 9, 9))
        t = conv_any(inp["x"], self.w, self.b, *self.d, self.depthwise)
        e = gamma(self.K) * conv_any(np.abs(inp["x"]), np.abs(self.w), np.zeros_like(self.b), *self.d, self.depthwise)
        dlt = e + U * (np.abs(t) + e)
        if self.res is not None:
            dlt = dlt + U * (np.abs(t + self.residual(inp)) + dlt)
        return dlt

    def emulate(self, inp):
        """float32 numpy: tap after tap, numpy's own order inside a tap."""
        f = np.float32
        y = conv_any(inp["x"].astype(f), self.w.astype(f), self.b.astype(f), *self.d, self.depthwise)
        if self.res is not None:
            y = y + self.residual(inp).astype(f)
        return np.maximum(y, f(0)) if self.relu else y

    def plan(self):
        """What plan_dump's line of the launch must hold."""
        (kh, kw), (dh, dw) = self.k, self.d
        tile = kh == kw and kh in (1, 3) and (dh, dw) == (1, 1)
        assert (self.kind == "tile") == (tile and not self.depthwise)
        want = [" kind=0 ", " dense=0 ", f" depthwise={int(self.depthwise)} ", f" taps={kh * kw} ", f" k={kh}x{kw} ", f" d={dh}x{dw} ",
                f" act={int(self.relu)} ", " groups=1 ", f" cinPad={(self.C + 15) // 16 * 16} "]
        if not self.depthwise:
            want.append(f" coutTiles={(self.cout + 63) // 64} ")
        return want, (r" res=-2/0/0/0/f " if self.res is None else rf" res=\d+/{(self.res + self.cout + 15) // 16 * 16}/{self.res}/{self.cout}/s ")

    def others(self):
        return HEAD_NAMES | {"s", "r", "select", "pflat"}


# ---- graphPool ------------------------------------------------------------------------------------------------------------
class PoolCase(EdgeCase):
    """mode "max" | "avg_include" | "avg_exclude" over k at dilations d, on `src`: "view18" (18 channels at channel 6 of a
    27-wide stem) or "w64" (a 64-wide stem)."""
    kind = "pool"

    def __init__(self, nsg, mode, k, d=(1, 1), src="view18", seed=0):
        self.nsg, self.mode, self.k, self.d, self.src, self.seed = nsg, mode, k, d, src, seed
        self.W, self.off, self.C = (27, 6, 18) if src == "view18" else (64, 0, 64)
        self.parts = rm.starts(self.C)
        self.net = self.build(0)

    def build(self, part):
        net = rm.RNet(self.nsg)
        (kh, kw), (dh, dw) = self.k, self.d
        x = net.stem(self.W, self.seed, EXP)
        if self.off:
            net.const("x_sizes", [self.off, self.C, self.W - self.off - self.C], np.int64)
            x = net.node("Split", ["s", "x_sizes"], ["x_lead", "x_view", "x_rest"], name="x_split", axis=1)[1]
        net.mark = False
        attrs = dict(kernel_shape=[kh, kw], pads=[halo(kh, dh), halo(kw, dw)] * 2, strides=[1, 1])
        if (dh, dw) != (1, 1):
            attrs["dilations"] = [dh, dw]
        if self.mode != "max":
            attrs["count_include_pad"] = int(self.mode == "avg_include")
        y = net.node("MaxPool" if self.mode == "max" else "AveragePool", [x], "k_y", name="kut", **attrs)
        self.show(net, y, self.C, part)
        net.mark = True
        net.heads_of("s", self.W)
        return net

    def model(self, part=0):
        return self.build(part).data()

    def inputs(self, x):
        env = self.net.known(x)
        assert rm.on_grid(env["s"], EXP)
        X = env["s"][:, self.off:self.off + self.C]
        if self.mode != "max":  # the window sum is an integer below 2^24 quanta in any order
            mass, _ = pool_any(np.abs(X), *self.k, *self.d, "avg_include")
            assert float(mass.max()) / Q < 2 ** 24
        return dict(x=X, env=env)

    def quotient(self, inp, fault=None):
        s, div = pool_any(inp["x"], *self.k, *self.d, self.mode, fault)
        return (s / div[None, None]).reshape(inp["x"].shape)

    def ref(self, inp, fault=None):
        if self.mode == "max":
            return pool_any(inp["x"], *self.k, *self.d, "max", fault)
        return em.f32(self.quotient(inp, fault))  # ONE division, correctly rounded

    def bound(self, inp):
        return np.zeros(inp["x"].shape)

    def emulate(self, inp):
        f = np.float32
        if self.mode == "max":
            return pool_any(inp["x"].astype(f), *self.k, *self.d, "max")
        s, div = pool_any(inp["x"].astype(f), *self.k, *self.d, self.mode)
        return (s / div.astype(f)[None, None]).reshape(inp["x"].shape)

    def plan(self):
        (kh, kw), (dh, dw) = self.k, self.d
        mode = ["max", "avg_include", "avg_exclude"].index(self.mode)
        return ([" kind=7 ", f" k={kh}x{kw} ", f" d={dh}x{dw} ", f" poolMode={mode} "],
                rf" in=\d+/{(self.W + 15) // 16 * 16}/{self.off}/{self.C}/s ")

    def others(self):
        return HEAD_NAMES | {"s", "select", "pflat"}


# ---- the dense layer (graphConv<1> over groups of 81 rows) ------------------------------------------------------------------
class DenseCase(EdgeCase):
    """Gemm K -> 2187 on the flat global max of a K-wide stem: the policy itself, 35 output tiles, the last with 11
    channels.  hidden: a first Gemm K -> hidden with ReLU in front of it (two launches of the kernel)."""
    kind = "dense"

    def __init__(self, nsg, K, hidden=None, exact=True, seed=0):
        self.nsg, self.K, self.hidden, self.exact, self.seed = nsg, K, hidden, exact, seed
        self.launches = 2 if hidden else 1
        rng = np.random.default_rng(9000 + seed + K)

        def weights(o, i):
            if exact:
                return rng.integers(-2, 3, size=(o, i)).astype(np.float64), rng.integers(-8, 9, size=o) * Q
            return em.f32(rng.normal(size=(o, i)) / np.sqrt(i)), em.f32(rng.normal(size=o) * 0.2)

        self.w1, self.b1 = weights(hidden, K) if hidden else (None, None)
        self.w, self.b = weights(WIN * 81, hidden or K)
        self.net = self.build(0)

    def build(self, part):
        net = rm.RNet(self.nsg)
        net.stem(self.K, self.seed, EXP)
        net.mark = False
        net.node("GlobalMaxPool", ["s"], "gm", name="gmax")
        x = net.node("Flatten", ["gm"], "flat", name="gmflat", axis=1)
        if self.hidden:
            net.node("Gemm", [x, net.const("k1_w", self.w1), net.const("k1_b", self.b1)], "h_z", name="kut1", transB=1)
            x = net.node("Relu", ["h_z"], "h", name="kact1")
        net.node("Gemm", [x, net.const("k_w", self.w), net.const("k_b", self.b)], "policy", name="kut", transB=1)
        net.mark = True
        net.heads_of("s", self.K)
        return net

    def model(self, part=0):
        return self.build(part).data()

    def inputs(self, x):
        env = self.net.known(x)
        assert rm.on_grid(env["s"], EXP)
        X = env["s"].max(axis=(2, 3))
        if self.exact:
            h = np.abs(X)
            if self.hidden:
                h = h @ np.abs(self.w1).T + np.abs(self.b1)
                assert float(h.max()) / Q < 2 ** 24
            mass = h @ np.abs(self.w).T + np.abs(self.b)
            assert float(mass.max()) / Q < 2 ** 24, float(mass.max())
        return dict(x=X, env=env)

    def ref(self, inp, fault=None):
        x = inp["x"]
        if self.hidden:
            x = np.maximum(x @ self.w1.T + self.b1, 0.0)
        y = x @ self.w.T + self.b
        if fault == "dense_row_81_repeats_row_80" and len(y) > 81:
            y = y.copy()
            y[81] = y[80]
        return y

    def bound(self, inp):
        y = self.ref(inp)
        if self.exact:
            return np.zeros_like(y)
        assert not self.hidden
        e = gamma(self.K) * (np.abs(inp["x"]) @ np.abs(self.w).T)
        return e + U * (np.abs(y) + e)

    def emulate(self, inp):
        f = np.float32
        x = inp["x"].astype(f)
        if self.hidden:
            x = np.maximum(x @ self.w1.astype(f).T + self.b1.astype(f), f(0))
        return x @ self.w.astype(f).T + self.b.astype(f)

    def select(self, out, part=0):
        return out

    def every_channel_shows(self, ref):
        assert float((ref.max(axis=0) - ref.min(axis=0)).min()) > 0.0

    def plan(self):
        return [" kind=0 ", " dense=1 ", " depthwise=0 ", " taps=1 ", " k=1x1 ", f" cinPad={((self.hidden or self.K) + 15) // 16 * 16} ", " coutTiles=35 ", " act=0 "], r" res=-2/0/0/0/f "

    def others(self):
        return HEAD_NAMES | {"s", "gmax"}


# ---- the cases, by id -----------------------------------------------------------------------------------------------------
RES = {"bare": None, "own": 0, "at27": 27, "at16": 16}
TILE_SHAPES = [(4, 27), (17, 27), (64, 64), (24, 65), (40, 72), (136, 129)]
GEOMETRIES = [(3, 5, 1, 1), (5, 3, 1, 1), (3, 7, 1, 1), (7, 3, 1, 1), (5, 7, 1, 1), (5, 9, 1, 1), (9, 5, 1, 1), (7, 9, 1, 1), (9, 7, 1, 1),
              (3, 9, 1, 1), (3, 3, 1, 2), (3, 3, 2, 1), (3, 3, 4, 1), (3, 3, 1, 4), (5, 3, 2, 1), (3, 5, 1, 2), (5, 5, 2, 1)]
DW_WIDTHS = [27, 30, 65]
DW_GEOMETRIES = [(9, 9, 1, 1), (3, 5, 1, 1), (5, 3, 1, 1), (3, 3, 1, 2), (3, 3, 4, 1)]
DW_RES = {"bare": None, "at16": 16, "at27": 27}  # at16: the float4 read of the residual; at27: the scalar one
POOL_WINDOWS = [(3, 3, 1, 1), (9, 9, 1, 1), (3, 5, 1, 1), (5, 3, 1, 1), (3, 3, 1, 2), (3, 3, 4, 1)]
DENSE_BATCHES = (1, 80, 81, 82, 163)


def gname(g):
    kh, kw, dh, dw = g
    return f"{kh}x{kw}d{dh}x{dw}"


TILE = {f"t{t}_{ci}x{co}_{r}": dict(kind="tile", cin=ci, cout=co, k=(k, k), res=RES[r])
        for t, k in ((9, 3), (1, 1)) for ci, co in TILE_SHAPES for r in RES}
GEO = {f"g{gname(g)}": dict(kind="geo", cin=None, cout=WIN, k=g[:2], d=g[2:]) for g in GEOMETRIES}
GEO.update({f"g{gname(g)}_40x72_own": dict(kind="geo", cin=40, cout=72, k=g[:2], d=g[2:], res=0) for g in ((3, 5, 1, 1), (3, 3, 2, 1))})
DW = {f"dw{C}_{gname(g)}_{r}": dict(kind="depthwise", cin=C, cout=C, k=g[:2], d=g[2:], res=DW_RES[r])
      for C in DW_WIDTHS for g in DW_GEOMETRIES for r in DW_RES}
ROUNDED = {
    "r_t9_40x72_at27": dict(kind="tile", cin=40, cout=72, res=27, exact=False),
    "r_t1_136x129_bare": dict(kind="tile", cin=136, cout=129, k=(1, 1), exact=False),
    "r_g3x5d1x1": dict(kind="geo", cin=None, cout=WIN, k=(3, 5), exact=False),
    "r_g3x3d2x1_40x72_own": dict(kind="geo", cin=40, cout=72, d=(2, 1), res=0, exact=False),
    "r_dw30_9x9d1x1_bare": dict(kind="depthwise", cin=30, cout=30, k=(9, 9), exact=False),
    "r_dw65_3x5d1x1_at27": dict(kind="depthwise", cin=65, cout=65, k=(3, 5), res=27, exact=False),
}
CONV = dict(TILE, **GEO, **DW, **ROUNDED)
POOL = {f"p_{m}_{gname(g)}_{src}": dict(mode=m, k=g[:2], d=g[2:], src=src)
        for m in ("avg_include", "avg_exclude", "max") for g in POOL_WINDOWS for src in ("view18", "w64")}
DENSE = {"d27": dict(K=27), "d64": dict(K=64), "d130": dict(K=130), "d64_h65": dict(K=64, hidden=65), "r_d130": dict(K=130, exact=False)}
# geo and pooling cases are about indexing: batches of 1 and 3; everything else 1 and 19
INDEXING = set(GEO) | set(POOL)

# fault -> the device cases built for it (tests/test_conv_reference.py shows that each is caught)
FAULT_CASES = {
    "group_last_tap_dropped": ["g3x5d1x1", "g7x9d1x1", "g3x3d1x2", "r_g3x5d1x1", "r_g3x3d2x1_40x72_own"],
    "kernel_transposed": ["g3x5d1x1", "g9x5d1x1", "g3x3d2x1", "g5x5d2x1", "r_g3x5d1x1", "dw30_3x5d1x1_bare", "dw65_9x9d1x1_bare"],
    "dilations_swapped": ["g3x3d1x2", "g3x3d4x1", "g5x3d2x1", "g5x5d2x1", "r_g3x3d2x1_40x72_own", "dw27_3x3d1x2_bare", "p_avg_exclude_3x3d4x1_view18",
                          "p_max_3x3d1x2_w64"],
    "width_from_hy": ["g3x7d1x1", "g3x9d1x1", "g3x3d1x4", "g3x5d1x2"],
    "residual_at_offset_0": ["t9_24x65_at27", "t1_136x129_at16", "dw65_3x3d4x1_at27", "dw30_9x9d1x1_at16", "r_t9_40x72_at27", "r_dw65_3x5d1x1_at27"],
    "include_divisor_for_exclude": ["p_avg_exclude_3x3d1x1_view18", "p_avg_exclude_9x9d1x1_w64", "p_avg_exclude_3x3d1x2_w64"],
    "dense_row_81_repeats_row_80": ["d27", "d130", "d64_h65", "r_d130"],
}

def case(nsg, name):
    if name in CONV:
        return ConvCase(nsg, **CONV[name])
    if name in POOL:
        return PoolCase(nsg, **POOL[name])
    return DenseCase(nsg, **DENSE[name])
