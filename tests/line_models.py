"""Models around rank and file pooling (graphLinePool) and the line tensors behind it: the shared half of
tests/test_onnx_linepool.py (host) and tests/test_gpu_onnx_linepool.py (device).

  * CoordAttNet: a torch module with a coordinate-attention block (Hou et al., CVPR 2021): 3x3 stem, pool along the
    files and along the ranks, concat to 18 lines, shared 1x1 conv + BatchNorm + hardswish, split, two 1x1 convs +
    sigmoid, both gates multiplied onto the board; 1x1 policy conv and mean heads.
  * LNet: elt_models.Net with the line ops added to its float64 interpreter.  A mean is the exact sum (float64, rounded
    to float32: nine-term sums of the exact stem are exact) divided by float32 9 and rounded once; a max is exact.
  * ca_forward: the CoordAttNet in float64 numpy with a running absolute error bound for a float32 evaluation, derived
    from the operands (below).

The bound (u = 2^-24, gamma(n) = n u / (1 - n u)).  Every tensor carries e >= |float32 result - float64 result|:
  linear (conv, dense), n terms, the weights rounded to float32 once after BatchNorm is folded into them in double:
      e_out = |W| e_in + gamma(n + 3) (|W| (|x| + e_in) + |b|)
  mean of 9 or 81: e_out = mean(e_in) + gamma(n + 1) mean(|x| + e_in);   max: e_out = max over the line of e_in
  relu: e_out = e_in.   hardswish: slope at most 1.5, and 1 ulp: e_out = 1.5 e_in + 2u (|y| + 1.5 e_in)
  sigmoid: slope at most 1/4, and 1.28 ulp: e_out = e_in / 4 + 2 * 1.28 u
  product: e_out = |a| e_b + |b| e_a + e_a e_b + u (|a b| + ...)
"""
import numpy as np

import elt_models as em

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- the torch module ------------------------------------------------------------------------------------------------
def coord_att_net(form="reduce", C=86, F=32, R=8, act="hardswish"):
    """form: how the two poolings are written -- "reduce" (x.mean(3, keepdim=True) / x.mean(2, keepdim=True)),
    "adaptive" (adaptive_avg_pool2d), "max" (amax)."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as Fn

    class CoordAtt(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(F, R, 1), nn.BatchNorm2d(R)
            self.conv_h, self.conv_w = nn.Conv2d(R, F, 1), nn.Conv2d(R, F, 1)

        def forward(self, x):
            if form == "adaptive":
                xh, xw = Fn.adaptive_avg_pool2d(x, (9, 1)), Fn.adaptive_avg_pool2d(x, (1, 9))
            elif form == "max":
                xh, xw = x.amax(3, keepdim=True), x.amax(2, keepdim=True)
            else:
                xh, xw = x.mean(3, keepdim=True), x.mean(2, keepdim=True)
            y = torch.cat([xh, xw.permute(0, 1, 3, 2)], dim=2)
            y = self.bn1(self.conv1(y))
            y = Fn.hardswish(y) if act == "hardswish" else torch.relu(y)
            yh, yw = torch.split(y, [9, 9], dim=2)
            ah = torch.sigmoid(self.conv_h(yh))
            aw = torch.sigmoid(self.conv_w(yw.permute(0, 1, 3, 2)))
            return x * ah * aw

    class CoordAttNet(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Conv2d(C, F, 3, padding=1)
            self.att = CoordAtt()
            self.policy = nn.Conv2d(F, 27, 1)
            self.fc_v, self.fc_d = nn.Linear(F, 1), nn.Linear(F, 1)
            self.form, self.F, self.R, self.C = form, F, R, C

        def forward(self, x):
            x = self.att(torch.relu(self.stem(x)))
            h = x.mean(dim=(2, 3))
            return torch.flatten(self.policy(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))

    return CoordAttNet()


def randomize(net, seed):
    """Random weights at a scale that keeps activations of order 1, and BatchNorm statistics that are not the identity."""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() > 1:
                fan = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / fan ** 0.5))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3 + (1.0 if name.endswith("bn1.weight") else 0.0))
        bn = net.att.bn1
        bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.2)
        bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) + 0.5)
    return net.eval()


def ca_forward(net, x):
    """CoordAttNet (form "reduce" or "max") on planes x [N,C,9,9] in float64 numpy: (policy, value, draw) and the bounds
    (e_policy, e_value, e_draw) of a float32 evaluation in any order of summation."""
    sd = {k: v.detach().numpy().astype(np.float64) for k, v in net.state_dict().items()}
    x = np.asarray(x, np.float64)
    e = np.zeros_like(x)

    def linear(x, e, w, b):  # w [O,I,kh,kw] on [N,I,9,W]: 1x1 or 3x3 (pad 1)
        k = w.shape[2]
        h = k // 2
        pad = ((0, 0), (0, 0), (h, h), (h, h))
        xp, ap = np.pad(x, pad), np.pad(np.abs(x) + e, pad)
        ep = np.pad(e, pad)
        H, W = x.shape[2], x.shape[3]
        y, a, eo = 0.0, 0.0, 0.0
        for dy in range(k):
            for dx in range(k):
                y = y + np.einsum("oc,ncyx->noyx", w[:, :, dy, dx], xp[:, :, dy:dy + H, dx:dx + W])
                a = a + np.einsum("oc,ncyx->noyx", np.abs(w[:, :, dy, dx]), ap[:, :, dy:dy + H, dx:dx + W])
                eo = eo + np.einsum("oc,ncyx->noyx", np.abs(w[:, :, dy, dx]), ep[:, :, dy:dy + H, dx:dx + W])
        bb = b.reshape(1, -1, 1, 1)
        n = w.shape[1] * k * k
        # the planner rounds the folded weights to float32 once: u |W| |x| more, inside gamma(n + 3)
        return y + bb, eo + gamma(n + 3) * (a + np.abs(bb))

    def line(x, e, axis):
        if net.form == "max":
            return x.max(axis=axis, keepdims=True), e.max(axis=axis, keepdims=True)
        return x.mean(axis=axis, keepdims=True), e.mean(axis=axis, keepdims=True) + gamma(10) * (np.abs(x) + e).mean(axis=axis, keepdims=True)

    def sigmoid(x, e):
        return em._sigmoid(x), e / 4 + 2 * 1.28 * U

    def mul(a, ea, b, eb):
        y = a * b
        return y, np.abs(a) * eb + np.abs(b) * ea + ea * eb + U * (np.abs(y) + np.abs(a) * eb + np.abs(b) * ea + ea * eb)

    s, e = linear(x, e, sd["stem.weight"], sd["stem.bias"])
    s = np.maximum(s, 0.0)
    xh, eh = line(s, e, 3)
    xw, ew = line(s, e, 2)
    y = np.concatenate([xh, xw.transpose(0, 1, 3, 2)], axis=2)
    ey = np.concatenate([eh, ew.transpose(0, 1, 3, 2)], axis=2)
    sc = sd["att.bn1.weight"] / np.sqrt(sd["att.bn1.running_var"] + net.att.bn1.eps)
    w1 = sd["att.conv1.weight"] * sc.reshape(-1, 1, 1, 1)
    b1 = (sd["att.conv1.bias"] - sd["att.bn1.running_mean"]) * sc + sd["att.bn1.bias"]
    y, ey = linear(y, ey, w1, b1)
    y = em.ACT64["hardswish"](y)
    ey = 1.5 * ey + 2 * U * (np.abs(y) + 1.5 * ey)
    ah, eah = sigmoid(*linear(y[:, :, :9], ey[:, :, :9], sd["att.conv_h.weight"], sd["att.conv_h.bias"]))
    aw, eaw = sigmoid(*linear(y[:, :, 9:].transpose(0, 1, 3, 2), ey[:, :, 9:].transpose(0, 1, 3, 2), sd["att.conv_w.weight"], sd["att.conv_w.bias"]))
    g, eg = mul(s, e, ah, eah)
    g, eg = mul(g, eg, aw, eaw)
    p, ep = linear(g, eg, sd["policy.weight"], sd["policy.bias"])
    h = g.mean(axis=(2, 3))
    eh_ = eg.mean(axis=(2, 3)) + gamma(82) * (np.abs(g) + eg).mean(axis=(2, 3))
    outs, errs = [p.reshape(len(x), -1)], [ep.reshape(len(x), -1)]
    for nm in ("fc_v", "fc_d"):
        w = sd[nm + ".weight"]
        z = h @ w.T + sd[nm + ".bias"]
        ez = eh_ @ np.abs(w).T + gamma(net.F + 3) * ((np.abs(h) + eh_) @ np.abs(w).T + np.abs(sd[nm + ".bias"]))
        v, ev = sigmoid(z, ez)
        outs.append(v)
        errs.append(ev)
    return outs, errs


# ---- hand-built models and their interpreter ---------------------------------------------------------------------------
LINE_ACTS = {"Exp": np.exp, "Reciprocal": lambda a: 1.0 / a}


class LNet(em.Net):
    """elt_models.Net plus ReduceMean / ReduceMax along one board axis, AveragePool / MaxPool of one rank or file,
    Concat, 1x1 Conv on any tensor, Exp, Reciprocal and Sigmoid / HardSwish kept in float64."""

    def run(self, x, rounded=True):
        r = em.f32 if rounded else (lambda a: np.asarray(a, np.float64))
        env = {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in self.consts.items()}
        env["input"] = np.asarray(x, np.float64)
        for node in self.nodes:
            op, ins, outs, at, _ = node
            a = [env[i] if i else None for i in ins]
            if op in ("ReduceMean", "ReduceMax"):
                ax = tuple(int(v) % 4 for v in (at["axes"] if "axes" in at else a[1]))
                y = a[0].max(axis=ax, keepdims=True) if op == "ReduceMax" else r(r(a[0].sum(axis=ax, keepdims=True)) / 9.0)
            elif op in ("AveragePool", "MaxPool") and tuple(at["kernel_shape"]) in ((1, 9), (9, 1)) and not any(at.get("pads", [0])):
                ax = 3 if tuple(at["kernel_shape"]) == (1, 9) else 2
                y = a[0].max(axis=ax, keepdims=True) if op == "MaxPool" else r(r(a[0].sum(axis=ax, keepdims=True)) / 9.0)
            elif op == "Concat":
                y = np.concatenate(a, axis=at["axis"])
            elif op == "Conv" and tuple(at["kernel_shape"]) == (1, 1):
                y = np.einsum("oc,ncyx->noyx", a[1][:, :, 0, 0], a[0]) + (a[2].reshape(1, -1, 1, 1) if len(a) > 2 else 0.0)
            elif op in LINE_ACTS:
                with np.errstate(over="ignore", divide="ignore"):
                    env[outs[0]] = LINE_ACTS[op](a[0])  # one Act code: float64, not rounded
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

    def line(self, x, out, how, files=False):
        """One rank / file pooling of x.  how: "mean", "max" (the Reduce ops), "avgpool", "maxpool" (the exporter's adaptive pools)."""
        if how in ("mean", "max"):
            return self.node("ReduceMean" if how == "mean" else "ReduceMax", [x], out, axes=[2 if files else 3], keepdims=1)
        ks = [9, 1] if files else [1, 9]
        return self.node("AveragePool" if how == "avgpool" else "MaxPool", [x], out, kernel_shape=ks, strides=ks, pads=[0, 0, 0, 0])
