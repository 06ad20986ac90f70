"""Models around the general graph path's product of two run-time token tensors (kLaunchBmm, DESIGN.md sections 13.3
and 13.4), their float64 references, per-element bounds and a float32 emulation with injectable faults: the shared half
of tests/test_onnx_bmm.py (host) and tests/test_gpu_onnx_bmm.py (device).

The hand-built half.  Every model is the exact stem of elt_models.Net (weights and bias small integers times 2^exp:
its float32 output is exact in any order of summation), the token view of it, `Slice`s of the token rows as operands,
ONE product (or an NT product feeding an NN product), and a policy that shows the result through nothing that rounds:

  NT  MatMul(A [N,81,K], Transpose(B [N,81,K]))  ->  [N,81,81]; the policy is a Slice of 27 of the 81 columns, transposed
      back and reshaped to [N,2187]: one model per third of the columns
  NN  MatMul(P [N,81,81], V [N,81,M])  ->  [N,81,M]; the policy is the same view where M = 27, otherwise a 0/1 selection
      MatMul of 27 channels (products by 0 and 1 and sums of zeros are exact), one model per window start

Value and draw read the mean of the stem, as in elt_models.

Exact cases: stem values are multiples of q = 2^exp, products multiples of q^2 (q^3 behind NT -> NN), and the test
asserts on the float64 side that sum|a b| / q^2 < 2^24 for every element: every partial sum, in any order, is then an
integer below 2^24 times the quantum and float32 holds it exactly.  The device must give the float64 product bit for bit.

Rounded cases: the stem stays on a grid (the operands must be known exactly for the bound to be one) but a fine one, 2^-11
with weights up to 2047, so its values are fractions of 15 to 17 significant bits and no product of two fits float32.
u = 2^-24, gamma(n) = n u / (1 - n u) as in reduction_models.  With exact operands, in any order, with or without FMA:

  |sum - sum64| <= gamma(K) sum|a b| = e                                 the chain
  t = sum * scale:  |t - t64| <= |scale| e + u (|t64| + |scale| e) = d   one more rounding, "one u for the scale"
  Relu is exact and 1-Lipschitz: d.  Sigmoid: d * max s'(x) over |x - t64| <= d, s' = s (1 - s), plus 2 * 1.28 ulps of
  the reference (twice DESIGN.md 13.3's measured 1.28, which is what the sibling tests assert).

The torch half: `HeadNet`, an attention policy head (two token Linears, from . to^T / sqrt(d), a table of 81 x 81 logits
per board of which the policy shows 27 columns) behind a conv stem plus a sigmoid-attention block sigmoid(q k^T / sqrt(d))
v without a head split.  It is exported at test time; nothing is added to tests/golden."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import elt_models as em  # noqa: E402
import reduction_models as rm  # noqa: E402
from reduction_models import U, gamma  # noqa: E402

WIN = rm.WIN
SIGMOID_ULPS = 2 * 1.28  # measured 1.28, asserted at twice that
ACT_ONNX = {"sigmoid": "Sigmoid", "relu": "Relu", "exp": "Exp", "recip": "Reciprocal"}
ACT64 = {"sigmoid": em.ACT64["sigmoid"], "relu": em.ACT64["relu"], "exp": np.exp, "recip": lambda a: 1.0 / a, None: lambda a: a}


def ulp32(a):
    """The float32 ulp at |a| (float64 in, float64 out)."""
    a32 = np.abs(np.asarray(a, np.float64)).astype(np.float32)
    return (np.nextafter(a32, np.float32(np.inf)) - a32).astype(np.float64)


class BmmCase(rm.Case):
    """form: "nt" (A . B^T), "nn" (P . V), "ntnn" ((A . B^T) . V).  offs: the channel offsets of the operands in the
    stem's rows -- (A, B) for nt, (P, V) for nn, (A, B, V) for ntnn; A and B at the same offset are one tensor (x x^T).
    b_from: "tokens" (Transpose of a token view) or "spatial" (the Reshape of the whole stem to [N,C,81]).  scale: a
    constant scalar behind the product, written as Div by 1 / scale (div) or as Mul; act: one activation behind that.
    part: the third of the columns (nt) or the window start (nn, ntnn, M != 27) the policy shows."""
    kind = "bmm"

    def __init__(self, nsg, form, K=0, M=0, offs=(0, 0), exp=-3, span=1, seed=0, scale=None, div=True, act=None, part=0,
                 b_from="tokens", exact=True, width=None, show="view", positive=False):
        self.form, self.K, self.M, self.offs, self.exp, self.scale, self.act, self.part, self.exact = form, K, M, offs, exp, scale, act, part, exact
        widths = {"nt": (K, K), "nn": (81, M), "ntnn": (K, K, M)}[form]
        self.widths = widths
        W = self.W = width or max(o + w for o, w in zip(offs, widths))
        net = self.net = rm.RNet(nsg)
        net.stem(W, seed, exp, span)
        if positive:  # every stem value, and so every product, is above zero
            net.consts["s_w"], net.consts["s_b"] = np.abs(net.consts["s_w"]), np.abs(net.consts["s_b"]) + np.float32(2.0 ** exp)
        net.tokens("s", W, "tok")
        net.mark = False
        names = {}
        for i, (o, w) in enumerate(zip(offs, widths)):
            if (o, w) in names:
                continue
            if o == 0 and w == W:
                names[(o, w)] = "tok"
                continue
            for nm, val in (("st", [o]), ("en", [o + w]), ("ax", [2])):
                net.const(f"op{i}_{nm}", val, np.int64)
            names[(o, w)] = net.node("Slice", ["tok", f"op{i}_st", f"op{i}_en", f"op{i}_ax"], f"op{i}", name=f"slice{i}")
        ops = [names[(o, w)] for o, w in zip(offs, widths)]
        if form in ("nt", "ntnn"):
            if b_from == "spatial":
                assert offs[1] == 0 and widths[1] == W
                bt = net.node("Reshape", ["s", net.const("b_to3", [-1, W, 81], np.int64)], "bt", name="b_c3")
            else:
                bt = net.node("Transpose", [ops[1]], "bt", name="b_t", perm=[0, 2, 1])
            y = net.node("MatMul", [ops[0], bt], "prod", name="product")
        else:
            y = net.node("MatMul", [ops[0], ops[1]], "prod", name="product")
        if scale is not None:
            if div:
                y = net.node("Div", [y, net.const("inv_scale", [1.0 / scale])], "scaled", name="scale")
            else:
                y = net.node("Mul", [y, net.const("the_scale", [scale])], "scaled", name="scale")
        if act is not None:
            y = net.node(ACT_ONNX[act], [y], "acted", name="act")
        if form == "ntnn":
            y = net.node("MatMul", [y, ops[2]], "prod2", name="product2")
        self.C = 81 if form == "nt" else M
        if show == "conv":  # the whole rows, pad channels included, through a 1x1 conv that selects 27 channels
            self.ch = part * WIN + np.arange(WIN)
            sel = np.zeros((WIN, self.C, 1, 1))
            sel[np.arange(WIN), self.ch] = 1.0
            net.node("Transpose", [y], "rt", name="rows_t", perm=[0, 2, 1])
            net.node("Reshape", ["rt", net.const("to4", [-1, self.C, 9, 9], np.int64)], "r4", name="rows_4d")
            net.node("Conv", ["r4", net.const("sel", sel)], "picked", name="select", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
            net.node("Flatten", ["picked"], "policy", name="pflat", axis=1)
            net.mark = True
            net.heads_of("s", W)
            self.data = net.data()
            return
        if form == "nt" or self.C == WIN:
            self.ch = (part * WIN + np.arange(WIN)) if form == "nt" else np.arange(WIN)
            if form == "nt":
                for nm, val in (("st", [part * WIN]), ("en", [part * WIN + WIN]), ("ax", [2])):
                    net.const("show_" + nm, val, np.int64)
                y = net.node("Slice", [y, "show_st", "show_en", "show_ax"], "shown", name="show")
        else:
            self.ch = rm.window(self.C, part)
            sel = np.zeros((self.C, WIN))
            sel[self.ch, np.arange(WIN)] = 1.0
            y = net.node("MatMul", [y, net.const("sel", sel)], "picked", name="select")
        net.node("Transpose", [y], "pt", perm=[0, 2, 1])
        net.node("Reshape", ["pt", net.const("to2", [-1, WIN * 81], np.int64)], "policy", name="pflat")
        net.mark = True
        net.heads_of("s", W)
        self.data = net.data()

    def scale32(self):
        """The scale as the device holds it: the double product of the folded float32 scalars, rounded once to float32."""
        if self.scale is None:
            return 1.0
        if "inv_scale" in self.net.consts:
            return float(np.float32(1.0 / np.float64(self.net.consts["inv_scale"][0])))
        return float(self.net.consts["the_scale"][0])

    def inputs(self, x):
        env = self.net.known(x)
        tok = env["tok"]
        assert rm.on_grid(tok, self.exp)
        ops = [tok[:, :, o:o + w] for o, w in zip(self.offs, self.widths)]
        inp = dict(ops=ops, tok=tok, env=env)
        if self.exact:  # every partial sum of every element, in any order, is an integer below 2^24 times the quantum
            q2 = 2.0 ** (2 * self.exp)
            if self.form == "nn":
                mass = np.einsum("nij,njc->nic", np.abs(ops[0]), np.abs(ops[1])) / q2
            else:
                mass = np.einsum("nik,njk->nij", np.abs(ops[0]), np.abs(ops[1])) / q2
            assert float(mass.max()) < 2 ** 24, float(mass.max())
            if self.form == "ntnn":
                s = np.abs(self.first(ops))
                assert np.array_equal(s, em.f32(s))
                mass = np.einsum("nij,njc->nic", s, np.abs(ops[2])) / (q2 * 2.0 ** self.exp)
                assert float(mass.max()) < 2 ** 24, float(mass.max())
            if self.scale is not None:  # a power of two
                assert np.log2(self.scale32()) == np.round(np.log2(self.scale32()))
        return inp

    def first(self, ops, scale=None, act="own"):
        """The first (or only) product with its epilogue, in float64."""
        s = np.einsum("nij,njc->nic", ops[0], ops[1]) if self.form == "nn" else np.einsum("nik,njk->nij", ops[0], ops[1])
        return ACT64[self.act if act == "own" else act](s * (self.scale32() if scale is None else scale))

    def ref(self, inp):
        y = self.first(inp["ops"])
        return np.einsum("nij,njc->nic", y, inp["ops"][2]) if self.form == "ntnn" else y

    def bound(self, inp):
        ops = inp["ops"]
        if self.exact and self.act in (None, "relu"):
            return np.zeros_like(self.ref(inp))
        assert self.form != "ntnn"
        n = 81 if self.form == "nn" else self.K
        mass = np.einsum("nij,njc->nic", np.abs(ops[0]), np.abs(ops[1])) if self.form == "nn" else np.einsum("nik,njk->nij", np.abs(ops[0]), np.abs(ops[1]))
        e = 0.0 if self.exact else gamma(n) * mass
        sc = abs(self.scale32())
        t = self.first(ops, act=None)
        d = sc * e + (U * (np.abs(t) + sc * e) if self.scale is not None and not self.exact else 0.0)
        if self.act in (None, "relu"):
            return d
        y = self.ref(inp)
        if self.act == "sigmoid":
            near = np.maximum(np.abs(t) - d, 0.0)  # s' is largest at the point of the interval nearest 0
            sg = em.ACT64["sigmoid"](near)
            return d * sg * (1.0 - sg) * (1.0 + 2.0 * d) + SIGMOID_ULPS * ulp32(y)
        if self.act == "recip":  # the division is the correctly rounded one
            assert self.exact and float(np.abs(t).min()) > 0.0
            return 0.5 * ulp32(y)
        assert self.act == "exp"
        return np.abs(y) * np.expm1(d) + 2.0 * ulp32(y)  # expf is held to 2 ulps, as reduction_models holds it

    def emulate(self, inp, fault=None):
        """float32 numpy, numpy's own order in the products; one fault by name (FAULTS)."""
        f = np.float32
        ops = [o.astype(f) for o in inp["ops"]]
        scale = f(self.scale32())

        def act(a):
            with np.errstate(over="ignore"):
                if self.act == "sigmoid":
                    return (f(1) / (f(1) + np.exp(-a))).astype(f)
                if self.act == "recip":
                    return f(1) / a
                return np.maximum(a, f(0)) if self.act == "relu" else np.exp(a).astype(f) if self.act == "exp" else a

        if self.form == "nn":
            p, v = ops
            if fault == "transposed":
                p = p.transpose(0, 2, 1)
            if fault == "last_k_dropped":  # the 21st k-step holds key 80
                p, v = p[:, :, :80], v[:, :80]
            if fault == "next_board_rows":  # keys 81..83: P's row read on into its neighbours' channels, V's rows the next board's
                tok = inp["tok"].astype(f)
                o = self.offs[0]
                more = tok[:, :, o + 81:o + 84]
                assert more.shape[2] == 3, "the case for this fault keeps three channels behind P"
                p = np.concatenate([p, more], axis=2)
                v = np.concatenate([v, np.roll(v, -1, axis=0)[:, :3]], axis=1)
            s = np.einsum("nij,njc->nic", p, v)
        else:
            a, b = ops[0], ops[1]
            if fault == "transposed":
                a, b = b, a
            if fault == "last_k_dropped":
                keep = (self.K + 3) // 4 * 4 - 4
                a, b = a[:, :, :keep], b[:, :, :keep]
            s = np.einsum("nik,njk->nij", a, b)
        y = act(s) * scale if fault == "scale_after_act" else act(s * scale)
        return np.einsum("nij,njc->nic", y, ops[2]) if self.form == "ntnn" else y

    def select(self, out):
        """[N,81,C] -> policy[n, j * 81 + sq] = out[n, sq, ch[j]]"""
        return out[:, :, self.ch].transpose(0, 2, 1).reshape(out.shape[0], -1)


# ---- the cases, by id ------------------------------------------------------------------------------------------------
EXACT = {
    "nt_k4": dict(form="nt", K=4, offs=(0, 4)),
    "nt_k16": dict(form="nt", K=16, offs=(16, 0)),
    "nt_k20_at4": dict(form="nt", K=20, offs=(4, 24)),
    "nt_k64_at20": dict(form="nt", K=64, offs=(20, 0), scale=0.125, act="relu"),
    "nt_k80": dict(form="nt", K=80, offs=(0, 80), scale=0.25, div=False),
    "gram_k80": dict(form="nt", K=80, offs=(0, 0)),                       # x x^T: both operands one tensor
    "gram_k81_spatial": dict(form="nt", K=81, offs=(0, 0), b_from="spatial"),  # K = 81: [N,C,81] makes it NT
    "nt_k20_at2": dict(form="nt", K=20, offs=(2, 23)),                    # neither offset a multiple of 4: two copies
    "nn_m16": dict(form="nn", M=16, offs=(16, 0)),
    "nn_m27_at4": dict(form="nn", M=27, offs=(32, 4), scale=0.5),
    "nn_m68_at20": dict(form="nn", M=68, offs=(88, 20), act="relu"),
    "nn_m81": dict(form="nn", M=81, offs=(84, 0)),                        # K = 81: a token tensor makes it NN
    "ntnn": dict(form="ntnn", K=4, M=27, offs=(0, 4, 8), exp=-1),         # NT feeding NN in one model
}
# the stem: 2^-11 times integers up to 2047
FINE = dict(exp=-11, span=2047, exact=False)
ROUNDED = {
    "nt_k64": dict(form="nt", K=64, offs=(0, 64), **FINE),
    "nt_k64_sigmoid": dict(form="nt", K=64, offs=(0, 64), scale=1.0 / 45, act="sigmoid", **FINE),
    "nt_k64_scale": dict(form="nt", K=64, offs=(64, 0), scale=1.0 / 3.0, div=False, **FINE),
    "nt_k256": dict(form="nt", K=256, offs=(0, 256), **FINE),
    "nt_k256_relu": dict(form="nt", K=256, offs=(0, 256), scale=0.1, act="relu", **FINE),
    "nt_k256_sigmoid": dict(form="nt", K=256, offs=(256, 0), scale=1.0 / 100, act="sigmoid", **FINE),
    "nn_m64": dict(form="nn", M=64, offs=(64, 0), **FINE),
    "nn_m64_sigmoid": dict(form="nn", M=64, offs=(64, 0), scale=1.0 / 48, act="sigmoid", **FINE),
}
CASES = dict(EXACT, **ROUNDED)

# fault -> the case built for it: the transposition needs A != B; the next board's rows show where P is a view with
# channels behind it (nn_behind, below) and the scale's place where a Sigmoid follows a scale
FAULTS = {"last_k_dropped": ["nt_k20_at4", "nt_k64", "nn_m64"], "transposed": ["nt_k16", "nt_k256", "nn_m64"],
          "next_board_rows": ["nn_behind"], "scale_after_act": ["nt_k64_sigmoid", "nn_m64_sigmoid"]}
CASES["nn_behind"] = dict(form="nn", M=16, offs=(16, 0), width=100, **FINE)  # three channels behind P's 81
# the pad channels 81..95 of an NT result, and 27..31 of an NN result, behind Exp and Reciprocal, read by a 1x1 conv's
# 16-channel chunks.  exp(0) = 1 in a pad meets a zero weight and stays hidden unless it is not finite; 1 / 0 = inf
# times that zero weight is NaN in every selected channel, which is why the positive-stem Reciprocal cases stand beside
# the Exp ones
CASES["nt_exp_conv"] = dict(form="nt", K=4, offs=(0, 4), scale=2.0 ** -4, act="exp", show="conv")
CASES["nt_recip_conv"] = dict(form="nt", K=4, offs=(0, 4), scale=2.0 ** -4, act="recip", show="conv", positive=True)
CASES["nn_recip_conv"] = dict(form="nn", M=27, offs=(28, 0), act="recip", show="conv", positive=True)
PAD_CASES = ["nt_exp_conv", "nt_recip_conv", "nn_recip_conv"]


def case(nsg, name, part=0):
    return BmmCase(nsg, part=part, **CASES[name])


def parts_of(name):
    kw = CASES[name]
    C = 81 if kw["form"] == "nt" else kw["M"]
    return [0, 1, 2] if kw["form"] == "nt" else [0] if C == WIN else rm.starts(C)


def baseline(nsg, W):
    """The same model without a product: stem, token view, a 27-channel Slice as the policy."""
    net = rm.RNet(nsg)
    net.stem(max(W, WIN), 0)
    net.tokens("s", max(W, WIN), "tok")
    for nm, val in (("st", [0]), ("en", [WIN]), ("ax", [2])):
        net.const("show_" + nm, val, np.int64)
    net.node("Slice", ["tok", "show_st", "show_en", "show_ax"], "shown", name="show")
    net.node("Transpose", ["shown"], "pt", perm=[0, 2, 1])
    net.node("Reshape", ["pt", net.const("to2", [-1, WIN * 81], np.int64)], "policy", name="pflat")
    net.heads_of("s", max(W, WIN))
    return net.data()


# ---- the torch module ------------------------------------------------------------------------------------------------
def head_net(F=32, d=16, seed=0):
    import torch
    import torch.nn as nn

    class HeadNet(nn.Module):
        """stem -> tokens -> x + proj(sigmoid(q k^T / sqrt(F)) v) -> the policy head: from = Linear(F, d), dst = Linear(F, d),
        logits = from . to^T / sqrt(d) ([N,81,81]: from-square by to-square), of which the policy is the first 27 to-columns."""

        def __init__(self):
            super().__init__()
            self.stem = nn.Conv2d(86, F, 3, padding=1)
            self.q, self.k, self.v, self.proj = nn.Linear(F, F), nn.Linear(F, F), nn.Linear(F, F), nn.Linear(F, F)
            self.frm, self.dst = nn.Linear(F, d), nn.Linear(F, d)
            self.fc_v, self.fc_d = nn.Linear(F, 1), nn.Linear(F, 1)

        def forward(self, x):
            N = x.size(0)
            x = torch.tanh(self.stem(x)).flatten(2).transpose(1, 2)
            w = torch.sigmoid(self.q(x) @ self.k(x).transpose(1, 2) / float(F) ** 0.5)
            x = x + self.proj(w @ self.v(x)) / 81.0
            logits = self.frm(x) @ self.dst(x).transpose(1, 2) * float(d) ** -0.5
            policy = logits[:, :, :WIN].transpose(1, 2).reshape(N, 2187)
            h = x.mean(dim=1)
            return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))

    torch.manual_seed(seed)
    import make_onnx_attention_golden as gen
    net = gen.randomize(HeadNet(), seed + 1).eval()
    with torch.no_grad():  # logits and sigmoid arguments of order 1: a dropped or misplaced product moves the outputs
        for m in (net.q, net.k, net.frm, net.dst):
            m.weight *= 6.0
    return net


def export(net, path, opset):
    import make_onnx_norm_golden as ng
    return ng.export_model(net, str(path), opset=opset)
