"""Models around the general graph path's Gather with constant indices and its board flips (kLaunchGather, DESIGN.md
sections 13.3 and 13.4) and their float64 references: the shared half of tests/test_onnx_gather.py (host) and
tests/test_gpu_onnx_gather.py (device).

The hand-built half.  Every model is the exact stem of elt_models.Net on the fine grid of bmm_models (2^-11 times
integers up to 2047: a board's values are nearly all distinct, and float32 holds every one of them exactly in any order
of summation), views of it (token rows, a `Slice` in front, the token rows flattened), ONE Gather or flip (a few models
hold two), and a policy that shows the result through nothing that rounds: the tensor itself where it has 27 channels
or 2187 values, otherwise a 0/1 selection (1x1 conv, MatMul or Gemm; products by 0 and 1 and sums of zeros are exact
for finite values, and a non-finite value anywhere in the rows read, pad channels included, comes out as NaN).  Value
and draw read the mean of the stem, as in elt_models.  A gather moves bits, so the reference is `numpy.take` on the
float64 stem and the device must give it bit for bit.

The pad cases.  The source is 1 / stem with the stem's channel 0 exactly zero: every row of the source holds +inf at
channel 0, which no index reads.  colTab's pad entries are 0, so a kernel that loaded for its pad lanes would fetch
that inf, and the 1x1 conv that reads the whole rows would turn it into NaN in every output.  A Reciprocal behind the
conv returns to the stem's values (two correctly rounded divisions: within 2.5 ulps, see PadCase).

The torch half: `GatherNet`, a conv stem, a channel index, a left-right symmetrised conv block written with
x.flip(3), a per-square policy Linear in square-major order mapped to the engine's order by logits[:, MAP], and
value / draw read as o[:, 0] / o[:, 1] of one Linear, as the reference network writes its value head.  It is exported
at test time; nothing is added to tests/golden."""
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

WIN = rm.WIN
EXP, SPAN = -11, 2047  # the fine grid of bmm_models.FINE
INT64_LOW = -(2 ** 63 - 1)  # the `ends` the exporter writes for x.flip()


def indices(pattern, K, M, seed=0):
    """M indices into an axis of extent K."""
    i = np.arange(M)
    if pattern == "reversed":  # the last ones first; wraps where M > K
        return (K - 1 - i) % K
    if pattern == "repeated":  # every index twice, in steps of three
        return (i // 2 * 3 + 1) % K
    if pattern == "equal":
        return np.full(M, K // 2)
    if pattern == "negative":  # counted from the end, down to -K
        return -1 - (i * 5) % K
    if pattern == "mixed":  # negative and positive, with repeats
        v = np.random.default_rng(50 + seed).integers(-K, K, size=M)
        v[0], v[-1] = -K, K - 1
        return v
    raise KeyError(pattern)


def square_perm(pattern):
    sq = np.arange(81)
    if pattern == "reversed":
        return sq[::-1].copy()
    if pattern == "flip_files":
        return sq // 9 * 9 + 8 - sq % 9
    if pattern == "repeated":  # some squares twice, some never, some counted from the end
        v = np.random.default_rng(7).integers(-81, 81, size=81)
        v[0], v[80] = 80, -81
        return v
    raise KeyError(pattern)


def policy_map(width=27):
    """MAP[dir * 81 + to] = to * width + dir: a square-major policy read in the engine's order."""
    d, to = np.divmod(np.arange(2187), 81)
    return to * width + d


class GNet(rm.RNet):
    """RNet whose 0-d constants are written as ONNX scalars (no dims), which is what the exporter writes for x[:, i]."""

    def data(self):
        io = self.io
        plain = io._tensor

        def tensor(name, arr):  # onnx_io writes a 0-d array as [1]: drop that one dim (field 1, value 1)
            body = plain(name, arr)
            if np.ndim(arr) == 0:
                assert body[:2] == bytes([0x08, 0x01]), body[:2]
                body = body[2:]
            return body

        io._tensor = tensor
        try:
            data = super().data()
        finally:
            io._tensor = plain

        def opset_import(v):
            return io._f_bytes(8, io._f_bytes(1, "") + io._f_varint(2, v))

        tail = opset_import(17)  # what elt_models.Net writes
        assert data.endswith(tail)
        return data[:-len(tail)] + opset_import(self.opset)

    opset = 17


class GatherCase(rm.Case):
    """form, on a stem of W channels with an optional `Slice` [off, off + K) of the channels in front:
         chan      x[:, IDX]         spatial [N,K,9,9] -> [N,M,9,9]
         tokchan   tok[:, :, IDX]    token [N,81,K] -> [N,81,M]
         toksq     tok[:, PERM]      token [N,81,K] -> [N,81,K], PERM of 81 squares
         tok_s     tok[:, s]         token -> flat [N,K]
         tok_c     tok[:, :, c]      token -> flat [N,81]
         flat      v[:, IDX]         flat [N,81*W] (the token rows flattened, W a multiple of 16) sliced to [off, off + K)
         flatview  x.flatten(1)[:, IDX]   the flattened view [N,K*81] of the spatial tensor
         flip      x.flip(axes)      spatial, axes of (2, 3); `twice`: applied twice
       idx: the index list (or the scalar for tok_s / tok_c)."""
    kind = "gather"

    def __init__(self, nsg, form, W, idx=None, off=0, K=None, axes=(3,), twice=False, seed=0, ends=INT64_LOW, one_slice=True, opset=17):
        self.form, self.W, self.off, self.axes, self.twice = form, W, off, tuple(axes), twice
        self.full = 81 * W if form == "flat" else W  # the extent of the axis the Slice in front cuts
        K = self.K = (self.full - off) if K is None else K
        self.idx = None if idx is None else np.asarray(idx, np.int64)
        net = self.net = GNet(nsg)
        net.opset = opset
        net.stem(W, seed, EXP, SPAN)
        self.build(net, "s", ends, one_slice)
        net.mark = True
        net.heads_of("s", W)
        self.data = net.data()

    # ---- the model
    def sliced(self, net, x, axis, lo, hi, tag="front"):
        for nm, val in (("st", [lo]), ("en", [hi]), ("ax", [axis])):
            net.const(f"{tag}_{nm}", val, np.int64)
        return net.node("Slice", [x, f"{tag}_st", f"{tag}_en", f"{tag}_ax"], tag, name=tag)

    def build(self, net, src, ends, one_slice):
        form, W, off, K = self.form, self.W, self.off, self.K
        part = off != 0 or K != self.full
        if form in ("tokchan", "toksq", "tok_s", "tok_c"):
            x = net.tokens(src, W, "tok")
            net.mark = False
            if part:
                x = self.sliced(net, x, 2, off, off + K)
            axis = 1 if form in ("toksq", "tok_s") else 2
            g = net.node("Gather", [x, net.const("idx", self.idx, np.int64)], "g", name="gather", axis=axis)
            if form in ("tokchan", "toksq"):
                return self.show_tokens(net, g, len(self.idx) if form == "tokchan" else K)
            return self.show_flat(net, g, K if form == "tok_s" else 81)
        if form == "flat":
            assert W % 16 == 0
            x = net.tokens(src, W, "tok")
            net.mark = False
            x = net.node("Reshape", [x, net.const("to_flat", [-1, 81 * W], np.int64)], "tokflat", name="tokflat")
            if part:
                x = self.sliced(net, x, 1, off, off + K)
            g = net.node("Gather", [x, net.const("idx", self.idx, np.int64)], "g", name="gather", axis=1)
            return self.show_flat(net, g, len(self.idx))
        net.mark = False
        x = self.sliced(net, src, 1, off, off + K) if part else src
        if form == "chan":
            g = net.node("Gather", [x, net.const("idx", self.idx, np.int64)], "g", name="gather", axis=1)
            return self.show_spatial(net, g, len(self.idx))
        if form == "flatview":
            x = net.node("Flatten", [x], "xf", name="xflat", axis=1)
            g = net.node("Gather", [x, net.const("idx", self.idx, np.int64)], "g", name="gather", axis=-1)
            return self.show_flat(net, g, len(self.idx))
        assert form == "flip"
        for rep in range(2 if self.twice else 1):
            groups = [self.axes] if one_slice else [(a,) for a in self.axes]
            for j, ax in enumerate(groups):
                t = f"flip{rep}{j}"
                net.const(t + "_st", [-1] * len(ax), np.int64)
                net.const(t + "_en", [ends] * len(ax), np.int64)
                net.const(t + "_ax", list(ax), np.int64)
                net.const(t + "_sp", [-1] * len(ax), np.int64)
                x = net.node("Slice", [x, t + "_st", t + "_en", t + "_ax", t + "_sp"], t, name=t)
        return self.show_spatial(net, x, K)

    def show_spatial(self, net, y, C):
        self.C, self.ch, self.out_kind = C, rm.window(C, 0), "spatial"
        if C == WIN:
            return net.node("Flatten", [y], "policy", name="pflat", axis=1)
        sel = np.zeros((WIN, C, 1, 1))
        sel[np.arange(WIN), self.ch] = 1.0
        net.node("Conv", [y, net.const("sel", sel)], "picked", name="select", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
        return net.node("Flatten", ["picked"], "policy", name="pflat", axis=1)

    def show_tokens(self, net, y, C):
        self.C, self.ch, self.out_kind = C, rm.window(C, 0), "token"
        if C != WIN:
            sel = np.zeros((C, WIN))
            sel[self.ch, np.arange(WIN)] = 1.0
            y = net.node("MatMul", [y, net.const("sel", sel)], "picked", name="select")
        net.node("Transpose", [y], "pt", perm=[0, 2, 1])
        return net.node("Reshape", ["pt", net.const("to2", [-1, WIN * 81], np.int64)], "policy", name="pflat")

    def show_flat(self, net, y, C):
        self.C, self.ch, self.out_kind = C, np.arange(WIN * 81) % C, "flat"
        if C == WIN * 81:
            return net.node("Identity", [y], "policy", name="pflat")
        sel = np.zeros((WIN * 81, C))
        sel[np.arange(WIN * 81), self.ch] = 1.0
        return net.node("Gemm", [y, net.const("sel", sel)], "policy", name="select", transB=1)

    # ---- the reference: numpy.take on the float64 stem
    def inputs(self, x):
        env = self.net.known(x)
        assert rm.on_grid(env["s"], EXP)
        return dict(s=env["s"], env=env)

    def ref(self, inp):
        s, off, K, form = inp["s"], self.off, self.K, self.form
        N = s.shape[0]
        tok = s.reshape(N, self.W, 81).transpose(0, 2, 1)
        if form == "chan":
            return np.take(s[:, off:off + K], self.idx, axis=1)
        if form in ("tokchan", "tok_c"):
            return np.take(tok[:, :, off:off + K], self.idx, axis=2)
        if form in ("toksq", "tok_s"):
            return np.take(tok[:, :, off:off + K], self.idx, axis=1)
        if form == "flat":
            return np.take(tok.reshape(N, -1)[:, off:off + K], self.idx, axis=1)
        if form == "flatview":
            return np.take(s[:, off:off + K].reshape(N, -1), self.idx, axis=1)
        y = s[:, off:off + K]
        return y if self.twice else np.flip(y, self.axes)

    def bound(self, inp):
        return np.zeros_like(self.ref(inp))

    def select(self, out):
        if self.out_kind == "spatial":
            return out[:, self.ch].reshape(out.shape[0], -1)
        if self.out_kind == "token":
            return out[:, :, self.ch].transpose(0, 2, 1).reshape(out.shape[0], -1)
        return out[:, self.ch]


class PadCase(GatherCase):
    """1 / stem (channel 0 of the stem exactly zero: +inf in every row of the source) -> Slice at channel 4 -> Gather of M
    channels -> a 1x1 conv over the whole rows that selects 27 -> Reciprocal -> the policy.  With x the stem's value,
    y1 = fl(1 / x) and y2 = fl(1 / y1) are correctly rounded divisions: y2 = x (1 + e2) / (1 + e1), |e| <= 2^-24, so
    |y2 - x| <= (2^-23 + 2^-46) |x| < 2.5 ulp(x)."""

    def __init__(self, nsg, M, pattern, W=32, off=4):
        self.form, self.W, self.off, self.K, self.axes, self.twice = "chan", W, off, W - off, (), False
        self.idx = np.asarray(indices(pattern, W - off, M), np.int64)
        net = self.net = GNet(nsg)
        net.stem(W, 0, EXP, SPAN)
        w, b = net.consts["s_w"], net.consts["s_b"]
        net.consts["s_w"], net.consts["s_b"] = np.abs(w), np.abs(b) + np.float32(2.0 ** EXP)  # every value above zero ...
        net.consts["s_w"][0], net.consts["s_b"][0] = 0.0, 0.0  # ... but channel 0, which is zero
        net.mark = False
        net.node("Reciprocal", ["s"], "inv", name="inv")
        x = self.sliced(net, "inv", 1, off, W)
        g = net.node("Gather", [x, net.const("idx", self.idx, np.int64)], "g", name="gather", axis=1)
        self.C, self.ch, self.out_kind = M, rm.window(M, 0), "spatial"
        sel = np.zeros((WIN, M, 1, 1))
        sel[np.arange(WIN), self.ch] = 1.0
        net.node("Conv", [g, net.const("sel", sel)], "picked", name="select", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
        net.node("Reciprocal", ["picked"], "back", name="back")
        net.node("Flatten", ["back"], "policy", name="pflat", axis=1)
        net.mark = True
        net.heads_of("s", W)
        self.data = net.data()

    def inputs(self, x):
        inp = super().inputs(x)
        s = inp["s"]
        assert not s[:, 0].any() and float(s[:, 1:].min()) > 0.0
        return inp

    def bound(self, inp):
        return 2.5 * ulp32(self.ref(inp))


# ---- the cases, by id ------------------------------------------------------------------------------------------------
# M in {1, 3, 4, 5, 16, 17, 27} from sources of width 20, 24 and 97; a Slice in front at channel offsets 0, 4 and 5
def _c(form, W, M, pattern, off=0, **kw):
    return dict(form=form, W=W, off=off, idx=indices(pattern, W - off, M), **kw)


CHANNELS = {
    "chan_w20_m1": _c("chan", 20, 1, "negative"),
    "chan_w20_m3_at4": _c("chan", 20, 3, "reversed", off=4),
    "chan_w24_m4": _c("chan", 24, 4, "repeated"),
    "chan_w24_m5_at5": _c("chan", 24, 5, "equal", off=5),
    "chan_w97_m16": _c("chan", 97, 16, "reversed"),
    "chan_w97_m17_at4": _c("chan", 97, 17, "negative", off=4),
    "chan_w97_m27_at5": _c("chan", 97, 27, "mixed", off=5),
    "chan_w20_m27": _c("chan", 20, 27, "reversed"),            # more indices than channels: every channel, some twice
    "tokchan_w24_m1_at5": _c("tokchan", 24, 1, "equal", off=5),
    "tokchan_w20_m5_at4": _c("tokchan", 20, 5, "negative", off=4),
    "tokchan_w97_m17": _c("tokchan", 97, 17, "repeated"),
    "tokchan_w24_m16_at5": _c("tokchan", 24, 16, "reversed", off=5),
    "tokchan_w97_m27_at4": _c("tokchan", 97, 27, "mixed", off=4),
}
SQUARES = {
    "toksq_w24_reversed": dict(form="toksq", W=24, idx=square_perm("reversed")),
    "toksq_w24_repeated_at5": dict(form="toksq", W=24, off=5, idx=square_perm("repeated")),
    "toksq_w20_files_at4": dict(form="toksq", W=20, off=4, idx=square_perm("flip_files")),
    "tok_s0_w97": dict(form="tok_s", W=97, idx=0),
    "tok_s40_w97": dict(form="tok_s", W=97, idx=40),
    "tok_s80_w97": dict(form="tok_s", W=97, idx=80),
    "tok_s_last_w40_at5": dict(form="tok_s", W=40, off=5, idx=-1),
    "tok_c0_w20_at4": dict(form="tok_c", W=20, off=4, idx=0),
    "tok_c_last_w20_at4": dict(form="tok_c", W=20, off=4, idx=15),
    "tok_c_negative_w24": dict(form="tok_c", W=24, idx=-2),
}
FLAT = {
    "flat_policy_map": dict(form="flat", W=32, K=2592, idx=policy_map(32)),               # square-major to * 32 + dir
    "flat_policy_perm_at5": dict(form="flat", W=32, off=5, K=2187, idx=np.random.default_rng(3).permutation(2187)),
    "flat_m27_at4": dict(form="flat", W=16, off=4, K=1000, idx=indices("mixed", 1000, 27)),
    "flatview_policy_perm": dict(form="flatview", W=27, idx=np.random.default_rng(4).permutation(2187)),
    "flatview_policy_map_at4": dict(form="flatview", W=32, off=4, K=27, idx=policy_map(27)[::-1].copy()),
    "flatview_m27_negative": dict(form="flatview", W=24, idx=indices("negative", 24 * 81, 27) * 37 % (24 * 81) - 24 * 81),
}
FLIPS = {
    "flip_files_w24": dict(form="flip", W=24, axes=(3,)),
    "flip_ranks_w24": dict(form="flip", W=24, axes=(2,), ends=-10),
    "flip_both_w24": dict(form="flip", W=24, axes=(2, 3)),
    "flip_files_w27": dict(form="flip", W=27, axes=(3,), ends=-10),
    "flip_ranks_w27_at5": dict(form="flip", W=32, off=5, axes=(2,)),
    "flip_both_w27": dict(form="flip", W=27, axes=(3, 2)),
    "flip_files_twice_w27": dict(form="flip", W=27, axes=(3,), twice=True),
    "flip_both_twice_w24": dict(form="flip", W=24, axes=(2, 3), twice=True, one_slice=False),
}
CASES = dict(CHANNELS, **SQUARES, **FLAT, **FLIPS)
PADS = {"pad_m27": (27, "mixed"), "pad_m17": (17, "reversed"), "pad_m1": (1, "negative"), "pad_m5": (5, "repeated")}
NEIGHBOURS = ["chan_w97_m17_at4", "tokchan_w20_m5_at4", "toksq_w24_repeated_at5", "tok_s80_w97", "tok_c_last_w20_at4",
              "flat_policy_perm_at5", "flatview_policy_perm", "flip_both_w24"]


def case(nsg, name, opset=17):
    return GatherCase(nsg, opset=opset, **CASES[name])


def pad_case(nsg, name):
    return PadCase(nsg, *PADS[name])


def gathers_of(name):
    """kLaunchGather records the case plans to."""
    kw = CASES[name]
    if kw["form"] != "flip":
        return 1
    return (2 if kw.get("twice") else 1) * (1 if kw.get("one_slice", True) else len(kw["axes"]))


def selects_of(c):
    """The selection launch of the policy, where there is one."""
    return 0 if c.C == (WIN * 81 if c.out_kind == "flat" else WIN) else 1


def baseline(nsg, W):
    """The same model without a gather: the stem, 27 of its channels as the policy, the heads."""
    net = rm.RNet(nsg)
    net.stem(max(W, WIN), 0, EXP, SPAN)
    for nm, val in (("st", [0]), ("en", [WIN]), ("ax", [1])):
        net.const("show_" + nm, val, np.int64)
    net.node("Slice", ["s", "show_st", "show_en", "show_ax"], "shown", name="show")
    net.node("Flatten", ["shown"], "policy", name="pflat", axis=1)
    net.heads_of("s", max(W, WIN))
    return net.data()


def two_heads(nsg, how, W=27):
    """value = sigmoid(o[:, 0]), draw = sigmoid(o[:, 1]) of one Gemm o [N,2]: with `how` = "gather" the integer indexing
    the exporter writes (a scalar Gather), with "slice" the twin o[:, 0:1] / o[:, 1:2]."""
    net = GNet(nsg)
    net.stem(W, 0, EXP, SPAN)
    net.node("Flatten", ["s"], "policy", name="pflat", axis=1)
    net.node("GlobalAveragePool", ["s"], "gp", name="gap")
    net.node("Flatten", ["gp"], "gpf", name="gflat", axis=1)
    rng = np.random.default_rng(1)
    net.const("fc_w", rng.normal(size=(2, W)) * 0.2)
    net.const("fc_b", [0.1, -0.2])
    net.node("Gemm", ["gpf", "fc_w", "fc_b"], "o", name="fc", transB=1)
    net.const("ax1", [1], np.int64)
    for i, out in enumerate(("value", "draw")):
        if how == "gather":
            net.node("Gather", ["o", net.const(f"i{i}", i, np.int64)], out + "_z", name=out + "_pick", axis=1)
        else:
            net.const(f"st{i}", [i], np.int64)
            net.const(f"en{i}", [i + 1], np.int64)
            net.node("Slice", ["o", f"st{i}", f"en{i}", "ax1"], out + "_z", name=out + "_pick")
        net.node("Sigmoid", [out + "_z"], out, name=out + "_sig")
    return net


# ---- the torch module ------------------------------------------------------------------------------------------------
def gather_net(F=32, seed=0, slice_heads=False):
    import torch
    import torch.nn as nn

    class GatherNet(nn.Module):
        """stem -> a channel index (24 of F channels, reversed, some twice) -> 0.5 (f(x) + f(x.flip(3)).flip(3)) -> per-square
        policy Linear(F, 32) in square-major order to * 32 + dir, read as logits[:, MAP] -> value, draw = sigmoid(o[:, 0]),
        sigmoid(o[:, 1]) of one Linear(F, 2) on the mean over the squares."""

        def __init__(self):
            super().__init__()
            self.stem = nn.Conv2d(86, F, 3, padding=1)
            self.f = nn.Conv2d(24, F, 3, padding=1)
            self.pol = nn.Linear(F, 32)
            self.fc = nn.Linear(F, 2)
            self.register_buffer("idx", torch.tensor([(F - 1 - i // 2 * 3) % F for i in range(24)], dtype=torch.long))
            self.register_buffer("map", torch.from_numpy(policy_map(32)))

        def block(self, x):
            return torch.tanh(self.f(x))

        def forward(self, x):
            N = x.size(0)
            h = torch.relu(self.stem(x))[:, self.idx]
            g = 0.5 * (self.block(h) + self.block(h.flip(3)).flip(3))
            tok = g.flatten(2).transpose(1, 2)
            policy = self.pol(tok).reshape(N, 81 * 32)[:, self.map]
            o = self.fc(tok.mean(dim=1))
            if slice_heads:
                return policy, torch.sigmoid(o[:, 0:1]), torch.sigmoid(o[:, 1:2])
            return policy, torch.sigmoid(o[:, 0]), torch.sigmoid(o[:, 1])

    torch.manual_seed(seed)
    import make_onnx_attention_golden as gen
    net = gen.randomize(GatherNet(), seed + 1).eval()
    with torch.no_grad():  # logits of order 1: a dropped or misplaced index moves the outputs
        net.pol.weight *= 4.0
        net.fc.weight *= 4.0
    return net


def export(net, path, opset):
    import make_onnx_norm_golden as ng
    return ng.export_model(net, str(path), opset=opset)
