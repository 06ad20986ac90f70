"""Models around one-channel maps on the general graph path: the reduction over the channels of a row (graphChanReduce,
kLaunchChanReduce) and the broadcast of a one-channel tensor over the channels of an elementwise result (kSrcRowOne,
kSrcBoardOne, kSrcSquare).  The shared half of tests/test_onnx_gate.py (host) and tests/test_gpu_onnx_gate.py (device).

Every hand-built model is the exact stem of elt_models.Net (small integers times 2^exp: exact in float32 in any order of
summation), views of it, the ops under test, and a policy that shows 27 channels through nothing that rounds: Flatten of
27 spatial channels, Transpose + Reshape of 27 token channels, or a 0/1 selection Gemm of 27 flat channels.

  * GNet: elt_models.Net with the ops of this family added to its float64 interpreter.  With `rounded` a sum is the
    float64 sum rounded to float32 once (exact whenever every partial sum is on the grid, which `sums_exact` asserts on
    the float64 side), a mean is that times float32(1 / C) rounded once, max and min are exact.
  * bcast_model: every binary op with a one-channel operand on either side, the gate a Slice of one stem channel (a
    view at channel 5: exact) behind Abs + 1, an open one-channel elementwise group that must be launched, not inlined.
  * reduce_model: ReduceMax / ReduceMin / ReduceSum / ReduceMean over views of C in WIDTHS channels at one offset, all in one
    model; the channel behind the widest view holds 1e30 on every square (a leak past offset + C shows in every result).
  * the bound of a float32 sum of C terms in any order: gamma(C) sum|x| (u = 2^-24); the mean: gamma(C) sum|x| / C plus
    one u |mean| for its factor (sum_bound).
  * emulate_reduce: a float32 numpy evaluation (one element after another), with one fault by name (FAULTS).
"""
import numpy as np

import elt_models as em
import reduction_models as rm

U = 2.0 ** -24
F = em.F
WIDTHS = [1, 3, 4, 16, 17, 27, 64, 100]
OFFSETS = [0, 1, 4, 20]
OPS = ["ReduceMax", "ReduceMin", "ReduceSum"]
BINARY = ["Add", "Sub", "Mul", "Div", "Max", "Min"]
POISON = 1e30
gamma = rm.gamma


def _axes(at, a, rank):
    ax = at["axes"] if "axes" in at else a[1]
    return tuple(int(v) % rank for v in ax)


class GNet(rm.RNet):
    """elt_models.Net plus Slice, Concat, Expand, MatMul, GlobalMaxPool, the reductions over the channels, and Exp /
    Sigmoid kept in float64."""

    def run(self, x, rounded=True):
        r = em.f32 if rounded else (lambda a: np.asarray(a, np.float64))
        env = {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in self.consts.items()}
        env["input"] = np.asarray(x, np.float64)
        for node in self.nodes:
            op, ins, outs, at, _ = node
            a = [env[i] if i else None for i in ins]
            if op in ("ReduceMax", "ReduceMin", "ReduceSum", "ReduceMean"):
                ax = _axes(at, a, a[0].ndim)
                keep = bool(at.get("keepdims", 1))
                if op == "ReduceMax":
                    y = a[0].max(axis=ax, keepdims=keep)
                elif op == "ReduceMin":
                    y = a[0].min(axis=ax, keepdims=keep)
                else:
                    y = r(a[0].sum(axis=ax, keepdims=keep))
                    if op == "ReduceMean":
                        y = y * em.f32(1.0 / a[0].shape[ax[0]]) if rounded else y / a[0].shape[ax[0]]
            elif op == "Slice":
                sl = [slice(None)] * a[0].ndim
                for st, en, ax in zip(a[1], a[2], a[3]):
                    sl[int(ax)] = slice(int(st), int(en))
                y = a[0][tuple(sl)]
            elif op == "Concat":
                y = np.concatenate(a, axis=at["axis"])
            elif op == "Expand":
                shape = [a[0].shape[0] if i == 0 else int(d) for i, d in enumerate(a[1])]
                y = np.broadcast_to(a[0], np.broadcast_shapes(a[0].shape, tuple(shape)))
            elif op == "MatMul":
                y = a[0] @ a[1]
            elif op == "GlobalMaxPool":
                y = a[0].max(axis=(2, 3), keepdims=True)
            elif op == "Exp":
                env[outs[0]] = np.exp(a[0])  # one Act code: float64, not rounded
                continue
            else:  # an op of elt_models: evaluated there, on the operands as they are
                sub = em.Net.__new__(em.Net)
                sub.consts = {i: env[i] for i in ins if i and i != "input"}
                sub.nodes = [node]
                res = sub.run(env["input"], rounded)
                for o in outs:
                    env[o] = res[o]
                continue
            env[outs[0]] = r(y)
        return env

    def slice(self, x, lo, hi, axis, out):
        for nm, v in (("_st", [lo]), ("_en", [hi]), ("_ax", [axis])):
            self.const(out + nm, v, np.int64)
        return self.node("Slice", [x, out + "_st", out + "_en", out + "_ax"], out)

    def reduce(self, op, x, out, axis, keepdims=1, as_input=None):
        """The axes as an input where the op's opset-17 form has one (ReduceSum), as an attribute otherwise; as_input forces either."""
        if (op == "ReduceSum") if as_input is None else as_input:
            return self.node(op, [x, self.const(out + "_axes", [axis], np.int64)], out, keepdims=keepdims)
        return self.node(op, [x], out, axes=[axis], keepdims=keepdims)

    def flat_max(self, x, out="fm"):
        """[N,W,9,9] -> the global max over the squares as a flat [N,W]: exact."""
        self.node("GlobalMaxPool", [x], out + "_4", name=out + "_gmax")
        return self.node("Flatten", [out + "_4"], out, axis=1)

    def show(self, y, kind):
        """policy from 27 channels of `kind` rows, through nothing that rounds."""
        if kind == "spatial":
            return self.node("Flatten", [y], "policy", name="pflat", axis=1)
        if kind == "token":
            self.node("Transpose", [y], "pt", perm=[0, 2, 1])
            return self.node("Reshape", ["pt", self.const("to2", [-1, F * 81], np.int64)], "policy", name="pflat")
        sel = np.zeros((F * 81, F))
        sel[np.arange(F * 81), np.arange(F * 81) % F] = 1.0
        return self.node("Gemm", [y, self.const("sel", sel)], "policy", name="select", transB=1)

    def widen(self, r1, kind, out="wide"):
        """A one-channel tensor broadcast to 27 channels by adding a per-channel constant of zeros: exact."""
        z = np.zeros({"spatial": (F, 1, 1), "token": (F,), "flat": (F,)}[kind])
        return self.node("Add", [r1, self.const(out + "_zeros", z)], out)


def rows_of(net, kind, width):
    """The stem as rows of `kind`: (tensor, channel axis)."""
    if kind == "spatial":
        return "s", 1
    if kind == "token":
        return net.tokens("s", width, "tok"), 2
    return net.flat_max("s"), 1


# ---- broadcasts of an exact gate -----------------------------------------------------------------------------------------
def bcast_model(nsg, kind, op, side, plain_gate=False, expand=False):
    """y = op(x, g) or op(g, x): x the 27 stem channels as `kind` rows ("board": spatial rows against a flat [N,1,1,1]
    gate), g = |channel 5| + 1 as a one-channel tensor (plain_gate: the bare Slice, a view at channel offset 5)."""
    net = GNet(nsg)
    net.stem(F)
    rows = "spatial" if kind == "board" else kind
    x, axis = rows_of(net, rows, F)
    if kind == "board":
        g = net.slice(net.flat_max("s"), 5, 6, 1, "g0")
        g = net.node("Reshape", [g, net.const("to4", [-1, 1, 1, 1], np.int64)], "g4")
    else:
        g = net.slice(x, 5, 6, axis, "g0")
    if not plain_gate:
        g = net.node("Add", [net.node("Abs", [g], "g_abs"), net.const("one", [1.0])], "gate")
    if expand:
        shape = {"spatial": [1, F, 9, 9], "board": [1, F, 9, 9], "token": [1, 81, F], "flat": [1, F]}[kind]
        g = net.node("Expand", [g, net.const("shape", shape, np.int64)], "g_exp")
    if op == "Div" and side == "left":  # g / x: the denominator |x| + 1, an open 27-channel group, inlined as ever
        x = net.node("Add", [net.node("Abs", [x], "x_abs"), net.const("x_one", [1.0])], "x_den")
    y = net.node(op, [x, g] if side == "right" else [g, x], "y")
    net.show(y, rows)
    net.heads_of("s", F)
    return net, net.data()


def square_const_model(nsg, kind, op="Mul"):
    """x op m with m one value per square: [1,1,9,9] on the spatial stem, [1,81,1] on its token rows."""
    net = GNet(nsg)
    net.stem(F)
    x, _ = rows_of(net, kind, F)
    m = (np.arange(81) % 7 - 3) * 0.25
    y = net.node(op, [x, net.const("mask", m.reshape((1, 1, 9, 9) if kind == "spatial" else (1, 81, 1)))], "y")
    net.show(y, kind)
    net.heads_of("s", F)
    return net, net.data()


def score_model(nsg, sigmoid=False):
    """The token-score gate tok * [sigmoid](tok @ w), w a constant [27,1] of small integers times 2^-2: the score
    [N,81,1] is written by a dense launch (the Sigmoid rides in it) and read through kSrcRowOne.  Without the Sigmoid every
    sum and product is on the grid of 2^-8, exact in float32."""
    net = GNet(nsg)
    net.stem(F)
    tok = net.tokens("s", F, "tok")
    w = (np.arange(F) % 5 - 2).reshape(F, 1) * 0.25
    g = net.node("MatMul", [tok, net.const("score_w", w)], "score")
    if sigmoid:
        g = net.node("Sigmoid", [g], "gate")
    net.show(net.node("Mul", [tok, g], "y"), "token")
    net.heads_of("s", F)
    return net, net.data()


def value_gate_model(nsg):
    """kSrcBoardOne from the value head: policy = Flatten(s * value[N,1] as [N,1,1,1])."""
    net = GNet(nsg)
    net.stem(F)
    net.heads_of("s", F)
    v4 = net.node("Reshape", ["value", net.const("to4", [-1, 1, 1, 1], np.int64)], "v4")
    net.show(net.node("Mul", ["s", v4], "y"), "spatial")
    return net, net.data()


# ---- reductions over the channels ---------------------------------------------------------------------------------------
def fine_bias(width):
    """Per-channel offsets of up to 2^12 on the 2^-11 grid: partial sums leave the 2^24 quanta a float32 holds."""
    return np.where(np.arange(width) % 3 == 1, 4096.0 - 37 * 2.0 ** -11, np.where(np.arange(width) % 3 == 2, -1024.0 - 2.0 ** -11, 0.0))


def reduce_model(nsg, kind, off, ops=OPS, widths=WIDTHS, exp=-3, fine=False, seed=0, poison=True):
    """Every op of `ops` over the views [off, off + C) for C in `widths` of one stem, one kLaunchChanReduce each; the
    results are the first len(ops) * len(widths) of the 27 channels shown, the rest zeros.  Returns (net, data, names):
    names[i] = (op, C) of shown channel i."""
    assert kind in ("spatial", "token", "flat") and len(ops) * len(widths) <= F
    end = off + max(widths)  # the poisoned channel, right behind the widest view
    W = max(end + (1 if poison else 0), F)
    net = GNet(nsg)
    net.stem(W, seed=seed + off, exp=exp)
    w, b = net.consts["s_w"], net.consts["s_b"]
    if fine:
        b[:end] += fine_bias(end).astype(np.float32)
    if poison:
        w[end], b[end] = 0.0, POISON
    x, axis = rows_of(net, kind, W)
    names, parts = [], []
    for op in ops:
        for C in widths:
            v = net.slice(x, off, off + C, axis, f"v_{op}_{C}")
            parts.append(net.reduce(op, v, f"r_{op}_{C}", axis if C % 2 else axis - x_rank(kind)))
            names.append((op, C))
    if kind == "token":  # no Concat along the token's channels: each result times a one-hot per-channel constant, summed
        y = None
        for i, p in enumerate(parts):
            t = net.node("Mul", [p, net.const(f"hot{i}", np.eye(F)[i])], f"h{i}")
            y = t if y is None else net.node("Add", [y, t], f"acc{i}")
    else:
        zeros = net.const("fill", np.zeros((F - len(parts), 1, 1) if kind == "spatial" else (F - len(parts),)))
        fill = net.node("Mul", [net.slice(x, 0, F - len(parts), 1, "lead"), zeros], "filled") if len(parts) < F else None
        groups = [parts[i:i + 8] for i in range(0, len(parts), 8)]
        cats = [net.node("Concat", g, f"cat{i}", axis=1) if len(g) > 1 else g[0] for i, g in enumerate(groups)]
        y = net.node("Concat", cats + ([fill] if fill else []), "y", axis=1)
    net.show(y, kind)
    net.heads_of("s", W)
    return net, net.data(), names


def x_rank(kind):
    return {"spatial": 4, "token": 3, "flat": 2}[kind]


def reduce_inputs(net, x, kind, off, width):
    """The float64 rows [..., width] the reductions of reduce_model read at `off`."""
    s = net.run(x, rounded=False)["s"]
    rows = s.transpose(0, 2, 3, 1).reshape(s.shape[0], 81, -1) if kind != "flat" else s.max(axis=(2, 3))
    return rows[..., off:off + width]


def sums_exact(rows, exp):
    """Every partial sum of the rows, in any order, is an integer below 2^24 quanta of 2^exp: sum|x| bounds them all."""
    q = rows * 2.0 ** -exp
    return bool((q == np.round(q)).all()) and float(np.abs(q).sum(axis=-1).max()) < 2 ** 24


def sum_bound(rows, mean=False):
    """|float32 sum in any order - float64 sum| <= gamma(n) sum|x|; the mean: that over n, plus one u |mean| for its
    factor.  (A sum of n terms needs gamma(n - 1) only; the step to gamma(n) is worth u sum|x| / n >= u |mean|, which pays
    for the second rounding, of the constant 1/n: DESIGN.md 13.3.)"""
    n = rows.shape[-1]
    e = gamma(n) * np.abs(rows).sum(axis=-1)
    if not mean:
        return e
    return e / n + U * np.abs(rows.sum(axis=-1)) / n


FAULTS = ["wrong_channel", "next_board", "drop_last", "tail_past", "mean_before_last_add"]


def emulate_reduce(buf, off, C, op, fault=None):
    """float32, one element after another, on rows buf [N,81,W] read at [off, off + C): [N,81].  Faults: drop_last (the
    last element of the view is not read), tail_past (the element at off + C is), mean_before_last_add (1/C multiplies
    the partial sum before the last element joins), next_board (board n reads board n + 1's rows)."""
    f = np.float32
    b = buf.astype(f)
    if fault == "next_board":
        b = np.roll(b, -1, axis=0)
    lo, hi = off, off + C - (1 if fault == "drop_last" else 0) + (1 if fault == "tail_past" else 0)
    v = b[..., lo:hi]
    if op == "ReduceMax":
        return v.max(axis=-1)
    if op == "ReduceMin":
        return v.min(axis=-1)
    if op == "ReduceMean" and fault == "mean_before_last_add":
        return np.cumsum(v[..., :-1], axis=-1, dtype=f)[..., -1] * f(1.0 / C) + v[..., -1]
    t = np.cumsum(v, axis=-1, dtype=f)[..., -1]
    return t * f(1.0 / C) if op == "ReduceMean" else t


def emulate_bcast(x, gate, fault=None):
    """x [N,81,C] * gate [N,81,G] read at channel 0 (wrong_channel: channel c of the gate's row)."""
    f = np.float32
    g = gate.astype(f)
    if fault == "next_board":
        g = np.roll(g, -1, axis=0)
    return x.astype(f) * (g[..., :x.shape[-1]] if fault == "wrong_channel" else g[..., :1])


# ---- exported torch modules ----------------------------------------------------------------------------------------------
def gate_net(block="scse", C=86, Fw=32, expand=False):
    """3x3 stem + ReLU, one gate block, 1x1 policy conv and mean heads.  "scse": x * sigmoid(fc2(relu(fc1(mean(x))))) +
    x * sigmoid(conv1x1_{F->1}(x)) (Roy et al. 2018); expand: the spatial gate through .expand_as(x).  "cbam": CBAM's
    spatial attention (Woo et al. 2018) with the channel mean written as sum / C: x * sigmoid(conv7x7([sum / C, amax]))."""
    import torch
    import torch.nn as nn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Conv2d(C, Fw, 3, padding=1)
            self.fc1, self.fc2 = nn.Linear(Fw, Fw // 4), nn.Linear(Fw // 4, Fw)
            self.sq = nn.Conv2d(Fw, 1, 1)
            self.sp = nn.Conv2d(2, 1, 7, padding=3)
            self.policy = nn.Conv2d(Fw, 27, 1)
            self.fc_v, self.fc_d = nn.Linear(Fw, 1), nn.Linear(Fw, 1)
            self.block, self.F = block, Fw

        def forward(self, x):
            x = torch.relu(self.stem(x))
            if block == "scse":
                c = torch.sigmoid(self.fc2(torch.relu(self.fc1(x.mean(dim=(2, 3)))))).reshape(-1, Fw, 1, 1)
                g = torch.sigmoid(self.sq(x))
                x = x * c + x * (g.expand_as(x) if expand else g)
            else:
                m = torch.cat([x.sum(1, keepdim=True) * (1.0 / Fw), x.amax(1, keepdim=True)], dim=1)
                x = x * torch.sigmoid(self.sp(m))
            h = x.mean(dim=(2, 3))
            return torch.flatten(self.policy(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))

    return Net()


def gate_bench_net(C=86, Fw=256, blocks=20):
    """The residual net of scripts/graph_bench.py --gate: a 3x3 stem, `blocks` blocks of conv3x3-BN-ReLU-conv3x3-BN with
    an scSE gate (x * cSE + x * sigmoid(conv1x1_{F->1}(x))) in front of the residual add and the ReLU, 1x1 policy conv and
    mean heads."""
    import torch
    import torch.nn as nn

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.b1 = nn.Conv2d(Fw, Fw, 3, padding=1, bias=False), nn.BatchNorm2d(Fw)
            self.c2, self.b2 = nn.Conv2d(Fw, Fw, 3, padding=1, bias=False), nn.BatchNorm2d(Fw)
            self.fc1, self.fc2 = nn.Linear(Fw, Fw // 8), nn.Linear(Fw // 8, Fw)
            self.sq = nn.Conv2d(Fw, 1, 1)

        def forward(self, x):
            y = self.b2(self.c2(torch.relu(self.b1(self.c1(x)))))
            c = torch.sigmoid(self.fc2(torch.relu(self.fc1(y.mean(dim=(2, 3)))))).reshape(-1, Fw, 1, 1)
            return torch.relu(x + y * c + y * torch.sigmoid(self.sq(y)))

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Conv2d(C, Fw, 3, padding=1)
            self.blocks = nn.Sequential(*[Block() for _ in range(blocks)])
            self.policy = nn.Conv2d(Fw, 27, 1)
            self.fc_v, self.fc_d = nn.Linear(Fw, 1), nn.Linear(Fw, 1)

        def forward(self, x):
            x = self.blocks(torch.relu(self.stem(x)))
            h = x.mean(dim=(2, 3))
            return torch.flatten(self.policy(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))

    return Net()


def randomize(net, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * ((1.5 / p[0].numel() ** 0.5) if p.dim() > 1 else 0.3))
    return net.eval()
