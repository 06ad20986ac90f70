"""Models around the L1 / L2 norms, the sum of squares and the log-sum-exp over the channels of a row (graphChanReduce's
kRedL1, kRedSumSq, kRedL2, kRedLogSumExp) and the fused F.normalize launch (graphNormalize, kLaunchNormalize): the shared
half of tests/test_onnx_normalize.py (host) and tests/test_gpu_onnx_normalize.py (device).

Every hand-built model is the exact stem of elt_models.Net, views of it, the ops under test and a policy that shows
their results through nothing that rounds (gate_models).  NNet gives the four reductions their float64 definitions and
defers every other node to gate_models.GNet; with `rounded` each result is the float64 value rounded to float32 once:

  * L1 and SumSquare on a grid where every partial sum is exact: the float32 result in any order of summation;
  * L2 of an exact sum of squares: sqrt in float64 then one rounding is the correctly rounded float32 sqrtf (53 >= 2 * 24
    + 2 bits: the double rounding is innocuous), likewise x / max(n, eps) of two float32 values.  So on such a grid the
    whole F.normalize output has one right answer in float32, and the device must give it bit for bit.

pack_model puts up to 27 one-channel results of (op, offset, C) side by side; normalize_model normalises one view and
shows all its channels; `twin` gives the norm a second reader (+ 0 * n, exact), which keeps the chain from fusing."""
import numpy as np

import elt_models as em
import gate_models as gm

F = gm.F
U = gm.U
REDUCE = ["ReduceL1", "ReduceSumSquare", "ReduceL2", "ReduceLogSumExp"]
MODE = {"ReduceMax": 0, "ReduceMin": 1, "ReduceSum": 2, "ReduceL1": 3, "ReduceSumSquare": 4, "ReduceL2": 5, "ReduceLogSumExp": 6}
WIDTHS = [1, 3, 4, 5, 15, 16, 17, 24, 63, 64, 65, 100]
OFFSETS = [0, 1, 2, 3, 4]


def reduce64(op, a, ax):
    """The float64 definition over axis `ax`, keepdims."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if op == "ReduceL1":
            return np.abs(a).sum(axis=ax, keepdims=True)
        if op == "ReduceSumSquare":
            return (a * a).sum(axis=ax, keepdims=True)
        if op == "ReduceL2":
            return np.sqrt((a * a).sum(axis=ax, keepdims=True))
        m = a.max(axis=ax, keepdims=True)
        fin = np.isfinite(m)
        s = np.exp(a - np.where(fin, m, 0.0)).sum(axis=ax, keepdims=True)
        return np.where(fin, np.where(fin, m, 0.0) + np.log(s), m)  # a row of -inf: -inf; a row with +inf: +inf


class NNet(gm.GNet):
    def run(self, x, rounded=True):
        r = em.f32 if rounded else (lambda a: np.asarray(a, np.float64))
        env = {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in self.consts.items()}
        env["input"] = np.asarray(x, np.float64)
        for node in self.nodes:
            op, ins, outs, at, _ = node
            if op in REDUCE:
                a = env[ins[0]]
                ax = tuple(int(v) % a.ndim for v in (at["axes"] if "axes" in at else env[ins[1]]))
                assert at.get("keepdims", 1) == 1
                with np.errstate(over="ignore"):
                    env[outs[0]] = r(reduce64(op, a, ax))
                continue
            sub = gm.GNet.__new__(gm.GNet)
            sub.consts = {i: env[i] for i in ins if i and i != "input"}
            sub.nodes = [node]
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                res = gm.GNet.run(sub, env["input"], rounded)
            for o in outs:
                env[o] = res[o]
        return env

    def reduce(self, op, x, out, axis, keepdims=1, as_input=None):
        """ReduceL1 / L2 / SumSquare / LogSumExp carry `axes` as an attribute up to opset 17; as_input forces the input form."""
        if op in REDUCE and as_input is None:
            as_input = False
        return super().reduce(op, x, out, axis, keepdims, as_input)

    def normalize(self, x, axis, out, p=2, eps=1e-12, expand_to=None, twin=False, clip_max=None, shape=None):
        """The exporter's F.normalize chain on x.  twin: the norm is read once more (y + 0 * n), so nothing fuses."""
        n = self.reduce("ReduceL1" if p == 1 else "ReduceL2", x, out + "_n", axis)
        lo = self.const(out + "_eps", np.asarray(eps, np.float32).reshape(()))
        hi = self.const(out + "_max", np.asarray(clip_max, np.float32).reshape(())) if clip_max is not None else ""
        c = self.node("Clip", [n, lo, hi], out + "_c")
        if expand_to is not None:
            c = self.node("Expand", [c, self.const(out + "_shape", expand_to, np.int64)], out + "_e")
        y = self.node("Div", [x, c], out + ("_y" if twin else ""))
        if twin:
            y = self.node("Add", [y, self.node("Mul", [n, self.const(out + "_zero", [0.0])], out + "_n0")], out)
        return y


def set_channels(net, values):
    """Stem channels {index: value}: zero weights and that bias, so the channel holds the value on every square."""
    for ch, v in values.items():
        net.consts["s_w"][ch] = 0.0
        net.consts["s_b"][ch] = v


def pack_model(nsg, kind, items, width, exp=-3, seed=0, fine=False, channels=None, span=1):
    """items: up to 27 (op, off, C); result i is shown channel i (token rows: through one-hot products, so finite results
    only).  Returns (net, data)."""
    assert kind in ("spatial", "token", "flat") and len(items) <= F
    W = max(width, F)
    net = NNet(nsg)
    net.stem(W, seed=seed, exp=exp, span=span)
    if fine:
        net.consts["s_b"][:] += gm.fine_bias(W).astype(np.float32)
    set_channels(net, channels or {})
    x, axis = gm.rows_of(net, kind, W)
    parts = []
    for i, (op, off, C) in enumerate(items):
        v = net.slice(x, off, off + C, axis, f"v{i}")
        parts.append(net.reduce(op, v, f"r{i}", axis if i % 2 else axis - gm.x_rank(kind)))
    if kind == "token":
        y = None
        for i, p in enumerate(parts):
            t = net.node("Mul", [p, net.const(f"hot{i}", np.eye(F)[i])], f"h{i}")
            y = t if y is None else net.node("Add", [y, t], f"acc{i}")
    else:
        zeros = net.const("fill", np.zeros((F - len(parts), 1, 1) if kind == "spatial" else (F - len(parts),)))
        fill = net.node("Mul", [net.slice(x, W - (F - len(parts)), W, 1, "lead"), zeros], "filled") if len(parts) < F else None
        groups = [parts[i:i + 8] for i in range(0, len(parts), 8)]
        cats = [net.node("Concat", g, f"cat{i}", axis=1) if len(g) > 1 else g[0] for i, g in enumerate(groups)]
        y = net.node("Concat", cats + ([fill] if fill else []), "y", axis=1) if len(cats) > 1 or fill else cats[0]
    net.show(y, kind)
    net.heads_of("s", W)
    return net, net.data()


def rows64(net, x, kind):
    """The stem's float64 rows [N,81,W] (flat: [N,W], the global max over the squares)."""
    s = net.run(x, rounded=False)["s"]
    return s.transpose(0, 2, 3, 1).reshape(s.shape[0], 81, -1) if kind != "flat" else s.max(axis=(2, 3))


def normalize_model(nsg, kind, off, C, p=2, eps=1e-12, twin=False, expand=True, exp=-3, seed=0, fine=False, channels=None,
                    width=None, clip_max=None, start=0):
    """F.normalize of the view [off, off + C) of the stem's `kind` rows.  Spatial and token rows show 27 channels (C = 27:
    all of them through nothing at all; otherwise the window from `start` through a 0/1 selection, which reads the pad
    channels against zero weights); flat rows show every channel, 2187 / C times, through a 0/1 selection Gemm."""
    W = max(width or off + C, F)
    net = NNet(nsg)
    net.stem(W, seed=seed, exp=exp)
    if fine:
        net.consts["s_b"][:] += gm.fine_bias(W).astype(np.float32)
    set_channels(net, channels or {})
    x, axis = gm.rows_of(net, kind, W)
    v = net.slice(x, off, off + C, axis, "v") if (off, C) != (0, W) else x
    shape = {"spatial": [1, C, 9, 9], "token": [1, 81, C], "flat": [1, C]}[kind]
    y = net.normalize(v, axis, "y", p, eps, shape if expand else None, twin, clip_max)
    ch = np.arange(F * 81) % C if kind == "flat" else (start * (C != F) + np.arange(F)) % C
    if kind == "flat":
        sel = np.zeros((F * 81, C))
        sel[np.arange(F * 81), ch] = 1.0
        net.node("Gemm", [y, net.const("sel", sel)], "policy", name="select", transB=1)
    elif C == F:
        net.show(y, kind)
    elif kind == "spatial":
        sel = np.zeros((F, C, 1, 1))
        sel[np.arange(F), ch] = 1.0
        net.node("Conv", [y, net.const("sel", sel)], "picked", name="select", kernel_shape=[1, 1], pads=[0, 0, 0, 0])
        net.show("picked", kind)
    else:
        sel = np.zeros((C, F))
        sel[ch, np.arange(F)] = 1.0
        net.show(net.node("MatMul", [y, net.const("sel", sel)], "picked", name="select"), kind)
    net.heads_of("s", W)
    return net, net.data(), ch


def shown_normalize(out, kind, ch):
    """The reference policy [N,2187] of a normalised tensor `out` ([N,81,C] rows or [N,C]) as normalize_model shows it."""
    if kind == "flat":
        return out[:, ch]
    return out[:, :, ch].transpose(0, 2, 1).reshape(out.shape[0], -1)


def normalize64(rows, p, eps):
    n = np.abs(rows).sum(axis=-1, keepdims=True) if p == 1 else np.sqrt((rows * rows).sum(axis=-1, keepdims=True))
    return rows / np.maximum(n, np.float64(np.float32(eps)))


def ulps(got, ref):
    """|got - ref| in float32 ulps of the float64 reference (one denormal step as the floor of an ulp)."""
    ref = np.asarray(ref, np.float64)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126)))
    return np.abs(np.asarray(got, np.float64) - ref) / 2.0 ** (np.maximum(e, -126) - 23)


# ---- the exported end-to-end model --------------------------------------------------------------------------------------
def cosine_net(C=86, E=32):
    """3x3 stem + ReLU; from / to embeddings over the tokens, L2-normalised (F.normalize), their cosine similarity as
    an [N,81,81] product; a policy conv; a value head on x - logsumexp(x) over the channels."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Conv2d(C, E, 3, padding=1)
            self.q, self.k = nn.Linear(E, E), nn.Linear(E, E)
            self.mix = nn.Linear(81, 27)
            self.fc_v, self.fc_d = nn.Linear(E, 1), nn.Linear(E, 1)

        def forward(self, x):
            x = torch.relu(self.stem(x))
            tok = x.flatten(2).transpose(1, 2)                       # [N,81,E]
            q = Fn.normalize(self.q(tok), dim=-1)
            k = Fn.normalize(self.k(tok), dim=-1)
            sim = torch.matmul(q, k.transpose(1, 2))                 # [N,81,81]: cosines
            pol = self.mix(sim).transpose(1, 2)                      # [N,27,81]
            logp = x - torch.logsumexp(x, 1, keepdim=True)           # a log-softmax over the channels
            h = torch.exp(logp).mean(dim=(2, 3))
            return torch.flatten(pol, 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))

    return Net()
