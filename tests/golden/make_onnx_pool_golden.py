"""Generates the pooling fixture of the general graph path (run from the repo root:
`python tests/golden/make_onnx_pool_golden.py`): net_graph_pool.onnx, net_pool.npz (float64 value and draw) and the
float64 policy in two files, net_graph_pool_policy_{0,1}.npz (positions 0-31 and 32-63, as for the other general-graph
fixtures: one file would exceed the repository's 1 MiB limit).

net_graph_pool is an 86-plane model of trunk width 48 built from the ops of two families of board-game nets:

  * a 3x3 stem with BatchNorm and hardswish;
  * a KataGo-style block: a 3x3 conv whose 48 outputs are `split` into [32, 16]; the 16 go through
    concat(mean, max over the squares) and a Linear into a per-channel bias on the 32; relu, a 3x3 conv back to 48, residual;
  * an inverted-residual block: 1x1 expand -> BatchNorm -> relu6, depthwise 3x3 -> BatchNorm -> hardswish, an SE gate
    with hardsigmoid, 1x1 project with the residual;
  * an inception-style block: cat(maxpool3x3 -> 1x1, avgpool3x3 (count_include_pad=False) -> 1x1, leaky_relu(conv3x3)),
    PReLU behind the concat, residual;
  * a 1x1 policy head, and a value head on concat(mean, max) of the trunk -> fc -> sigmoid value and sigmoid draw.

It is exported with make_onnx_geometry_golden.export_model (legacy TorchScript exporter, opset 17, dynamic batch axis,
BatchNormalization nodes kept).  The positions are the 86-plane positions of net_graph.npz.  The generator asserts
that float32 PyTorch agrees with the float64 outputs it stores to better than 1e-5.

The module classes are importable: tests/test_onnx_pool.py and tests/test_gpu_onnx_pool.py export small models built
from them at test time.
"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from make_onnx_geometry_golden import MeanHeads, conv, export_model, halo, pair, randomize  # noqa: E402,F401


class DilatedMaxPool(torch.autograd.Function):
    """A dilated max pool that keeps the board.  torch's max_pool2d refuses pads above half the kernel, whatever the
    dilation, so the halo is padded with -inf by hand; the exporter writes the one ONNX MaxPool node that this is
    (pads equal to the halo, like a dilated Conv)."""

    @staticmethod
    def forward(ctx, x, kh, kw, dh, dw):
        hy, hx = halo((kh, kw), (dh, dw))
        return Fn.max_pool2d(Fn.pad(x, (hx, hx, hy, hy), value=float("-inf")), (kh, kw), stride=1, dilation=(dh, dw))

    @staticmethod
    def symbolic(g, x, kh, kw, dh, dw):
        hy, hx = halo((kh, kw), (dh, dw))
        return g.op("MaxPool", x, kernel_shape_i=[kh, kw], pads_i=[hy, hx, hy, hx], dilations_i=[dh, dw],
                    strides_i=[1, 1], ceil_mode_i=0)


def pool(x, kind, k, d=1):
    """Pooling that keeps the 9x9 board.  kind: "max" (d = dilation), or "avg" (d = count_include_pad)."""
    if kind == "max" and pair(d) != (1, 1):
        return DilatedMaxPool.apply(x, *pair(k), *pair(d))
    if kind == "max":
        return Fn.max_pool2d(x, pair(k), stride=1, padding=halo(k))
    return Fn.avg_pool2d(x, pair(k), stride=1, padding=halo(k), count_include_pad=bool(d))


def mean_max(x):
    """KataGo's global pooling pair: [N, 2C]."""
    return torch.cat([x.mean(dim=(2, 3)), x.amax(dim=(2, 3))], dim=1)


class GPoolBlock(nn.Module):
    def __init__(self, F=48, G=16):
        super().__init__()
        self.F, self.G = F, G
        self.c1, self.b1 = conv(F, F, 3, bias=False), nn.BatchNorm2d(F)
        self.fc = nn.Linear(2 * G, F - G)
        self.c2, self.b2 = conv(F - G, F, 3, bias=False), nn.BatchNorm2d(F)

    def forward(self, x):
        a, g = torch.split(torch.relu(self.b1(self.c1(x))), [self.F - self.G, self.G], dim=1)
        a = torch.relu(a + self.fc(mean_max(g))[:, :, None, None])
        return torch.relu(x + self.b2(self.c2(a)))


class InvertedResidual(nn.Module):
    def __init__(self, F=48, E=96, R=24):
        super().__init__()
        self.ex, self.ex_bn = conv(F, E, 1, bias=False), nn.BatchNorm2d(E)
        self.dw, self.dw_bn = conv(E, E, 3, groups=E, bias=False), nn.BatchNorm2d(E)
        self.se1, self.se2 = nn.Linear(E, R), nn.Linear(R, E)
        self.pj, self.pj_bn = conv(E, F, 1, bias=False), nn.BatchNorm2d(F)

    def forward(self, x):
        h = Fn.relu6(self.ex_bn(self.ex(x)))
        h = Fn.hardswish(self.dw_bn(self.dw(h)))
        s = Fn.hardsigmoid(self.se2(torch.relu(self.se1(h.mean(dim=(2, 3))))))
        return x + self.pj_bn(self.pj(h * s[:, :, None, None]))


class InceptionBlock(nn.Module):
    def __init__(self, F=48):
        super().__init__()
        self.m1, self.a1, self.c3 = conv(F, F // 3, 1), conv(F, F // 3, 1), conv(F, F // 3, 3)
        self.prelu = nn.PReLU(F)

    def forward(self, x):
        y = torch.cat([self.m1(pool(x, "max", 3)), self.a1(pool(x, "avg", 3, 0)), Fn.leaky_relu(self.c3(x), 0.1)], dim=1)
        return x + self.prelu(y)


class PoolNet(nn.Module):
    """The fixture."""

    def __init__(self, C=86, F=48, VH=32):
        super().__init__()
        self.stem, self.stem_bn = conv(C, F, 3, bias=False), nn.BatchNorm2d(F)
        self.b1, self.b2, self.b3 = GPoolBlock(F), InvertedResidual(F), InceptionBlock(F)
        self.p = conv(F, 27, 1)
        self.fc1 = nn.Linear(2 * F, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        x = Fn.hardswish(self.stem_bn(self.stem(x)))
        x = self.b3(self.b2(self.b1(x)))
        h = torch.relu(self.fc1(mean_max(x)))
        return torch.flatten(self.p(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class PoolBenchNet(nn.Module):
    """scripts/graph_bench.py's pooling row: a 3x3 stem and `blocks` residual blocks of width F that alternate the
    KataGo-style pooled bias (two 3x3 convs) and the inception-style pooling branch (3x3 max and average pools, 1x1 and
    3x3 convs); the fixture's heads."""

    def __init__(self, C=86, F=256, blocks=20, G=64, VH=256):
        super().__init__()
        self.stem, self.stem_bn = conv(C, F, 3, bias=False), nn.BatchNorm2d(F)
        self.blocks = nn.ModuleList([GPoolBlock(F, G) if i % 2 == 0 else InceptionBlockWide(F) for i in range(blocks)])
        self.p = conv(F, 27, 1)
        self.fc1 = nn.Linear(2 * F, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        x = Fn.hardswish(self.stem_bn(self.stem(x)))
        for b in self.blocks:
            x = b(x)
        h = torch.relu(self.fc1(mean_max(x)))
        return torch.flatten(self.p(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class InceptionBlockWide(nn.Module):
    """The inception block at a width that 4 divides: max-pool and average-pool branches of F/4 channels each behind a
    pool of the whole trunk, a 3x3 branch of F/2."""

    def __init__(self, F=256):
        super().__init__()
        self.m1, self.a1, self.c3 = conv(F, F // 4, 1), conv(F, F // 4, 1), conv(F, F // 2, 3)
        self.prelu = nn.PReLU(F)

    def forward(self, x):
        y = torch.cat([self.m1(pool(x, "max", 3)), self.a1(pool(x, "avg", 3, 0)), Fn.leaky_relu(self.c3(x), 0.1)], dim=1)
        return torch.relu(x + self.prelu(y))


def integer_(m, g, lo=-2, hi=2, bias=3):
    with torch.no_grad():
        m.weight.copy_(torch.randint(lo, hi + 1, m.weight.shape, generator=g).float())
        if m.bias is not None:
            m.bias.copy_(torch.randint(-bias, bias + 1, m.bias.shape, generator=g).float())


class PoolTapNet(nn.Module):
    """The pooling op straight on the 0/1 input planes, then an integer-weight 1x1 conv to 27 channels (zero on the last
    `scalars` planes, which hold fractions: see make_onnx_geometry_golden.TapNet); value and draw from the mean of the
    planes.  kind "max": d is the dilation, every value is a small integer; kind "avg": d is count_include_pad.
    `cut` (the tests' float64 counter-example, never exported) pools over the window's centre row and column only; a
    window that is one row or one column loses its two outermost taps instead."""

    def __init__(self, kind, k, d=1, C=86, seed=0, scalars=4):
        super().__init__()
        self.kind, self.k, self.d, self.cut = kind, k, d, False
        self.p = conv(C, 27, 1)
        self.heads = MeanHeads(C)
        integer_(self.p, torch.Generator().manual_seed(seed))
        with torch.no_grad():
            self.p.weight[:, C - scalars:] = 0

    def pooled(self, x):
        if not self.cut:
            return pool(x, self.kind, self.k, self.d)
        assert self.kind == "max"
        (kh, kw) = pair(self.k)
        if kh > 1 and kw > 1:  # the centre row and the centre column
            return torch.maximum(pool(x, "max", (kh, 1), self.d), pool(x, "max", (1, kw), self.d))
        return pool(x, "max", (max(kh - 2, 1), max(kw - 2, 1)), self.d)  # a row or a column: without its two ends

    def forward(self, x):
        return (torch.flatten(self.p(self.pooled(x)), 1),) + self.heads(x)


class PoolBlockNet(nn.Module):
    """3x3 stem to C channels with BatchNorm and ReLU, `split` into [split, C - split], the second part pooled (kind
    None: left as it is), concat, then a 1x1 policy head and mean heads.  The planner test's variants: `through` feeds
    the first part to a 1x1 conv instead of the pool and the concat (split = C: no split at all), and `sliced` writes
    the split as two slices."""

    def __init__(self, C, split, kind, k=3, d=None, planes=86, through=False, sliced=False):
        super().__init__()
        self.C, self.split, self.kind, self.k, self.through, self.sliced = C, split, kind, k, through, sliced
        self.d = d if d is not None else (1 if kind == "max" else 0)
        self.stem, self.bn = conv(planes, C, 3, bias=False), nn.BatchNorm2d(C)
        W = split if through else C
        self.mid = conv(W, W, 1) if through else None
        self.p = conv(W, 27, 1)
        self.heads = MeanHeads(W)

    def halves(self, x):
        if self.split == self.C:
            return x, None
        if self.sliced:
            return x[:, :self.split], x[:, self.split:]
        return torch.split(x, [self.split, self.C - self.split], dim=1)

    def forward(self, x):
        a, b = self.halves(torch.relu(self.bn(self.stem(x))))
        if self.through:
            x = torch.relu(self.mid(a))
        else:
            x = torch.cat([a, pool(b, self.kind, self.k, self.d) if self.kind else b], dim=1)
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


class GlobalMaxNet(nn.Module):
    """An integer 3x3 stem on the 0/1 planes, the global max both ways the exporter writes it -- amax(dim=(2, 3)) is a
    ReduceMax, adaptive_max_pool2d(x, 1) a GlobalMaxPool -- and an integer Linear of the two into the policy: integers
    throughout.  Value and draw come from the mean of the planes."""

    def __init__(self, F=24, C=86, seed=0, scalars=4):
        super().__init__()
        self.stem = conv(C, F, 3)
        self.fc = nn.Linear(2 * F, 2187)
        self.heads = MeanHeads(C)
        g = torch.Generator().manual_seed(seed)
        integer_(self.stem, g)
        integer_(self.fc, g)
        with torch.no_grad():
            self.stem.weight[:, C - scalars:] = 0

    def forward(self, x):
        s = self.stem(x)
        h = torch.cat([s.amax(dim=(2, 3)), torch.flatten(Fn.adaptive_max_pool2d(s, 1), 1)], dim=1)
        return (self.fc(h),) + self.heads(x)


# name -> (function of (net, pre-activation, second operand), the pre-activation's kinks; binary: the kink is a = b)
ACTS = {
    "relu6": (lambda n, a, b: Fn.relu6(a), (0.0, 6.0)),
    "hardswish": (lambda n, a, b: Fn.hardswish(a), (-3.0, 3.0)),
    "hardsigmoid": (lambda n, a, b: Fn.hardsigmoid(a), (-3.0, 3.0)),
    "hardtanh": (lambda n, a, b: Fn.hardtanh(a, -1.0, 2.0), (-1.0, 2.0)),
    "clamp_min": (lambda n, a, b: torch.clamp(a, min=-0.5), (-0.5,)),
    "leaky_relu": (lambda n, a, b: Fn.leaky_relu(a, 0.1), (0.0,)),
    "prelu": (lambda n, a, b: n.prelu(a), (0.0,)),
    "maximum": (lambda n, a, b: torch.maximum(a, b), None),
    "minimum": (lambda n, a, b: torch.minimum(a, b), None),
    "abs": (lambda n, a, b: torch.abs(a), (0.0,)),
    "neg": (lambda n, a, b: torch.neg(a), ()),
}


class ActNet(nn.Module):
    """One activation of ACTS behind a 3x3 stem s = relu(stem(planes)) of width F:

      where = "epilogue": y = act(bn(c(s))), the activation straight behind a conv with BatchNorm;
      where = "chain":    t = bn(c(s)) also feeds the value heads, so the residual s + t is an elementwise Add at run
                          time and y = act(s + t) joins its chain.

    The second operand of maximum / minimum is a 1x1 conv of s.  `gain` and `shift` are a fixed per-channel gain and
    offset on the conv's input side of the activation (they are the BatchNorm's scale and bias, over moments measured
    on `calib`): channel c's pre-activations have deviation gain[c] in [1, 5] around shift[c] in [-3, 6], so that they
    fall on both sides of every kink.  pre(x) returns the pre-activation (for binary ops: a - b)."""

    def __init__(self, act, where, calib, F=24, C=86, seed=0):
        super().__init__()
        assert where in ("epilogue", "chain") and act in ACTS
        self.act, self.where = act, where
        self.stem = conv(C, F, 3)
        self.c, self.bn = conv(F, F, 3, bias=False), nn.BatchNorm2d(F)
        self.other = conv(F, F, 1)
        self.prelu = nn.PReLU(F)
        self.p = conv(F, 27, 1)
        self.heads = MeanHeads(F)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.prelu.weight.copy_(torch.rand(F, generator=g) * 2.0 - 0.5)
            u = self.c(torch.relu(self.stem(calib.float())))
            self.bn.running_mean.copy_(u.mean(dim=(0, 2, 3)))
            self.bn.running_var.copy_(u.var(dim=(0, 2, 3)))
            self.bn.weight.copy_(torch.linspace(1.0, 5.0, F)[torch.randperm(F, generator=g)])
            self.bn.bias.copy_(torch.linspace(-3.0, 6.0, F))

    def parts(self, x):
        s = torch.relu(self.stem(x))
        t = self.bn(self.c(s))
        a = t if self.where == "epilogue" else s + t
        return s, t, a, self.other(s)

    def pre(self, x):
        s, t, a, b = self.parts(x)
        return a - b if ACTS[self.act][1] is None else a

    def forward(self, x):
        s, t, a, b = self.parts(x)
        y = ACTS[self.act][0](self, a, b)
        return (torch.flatten(self.p(y), 1),) + self.heads(t if self.where == "chain" else y)


NAME = "net_graph_pool"


def main():
    nsg = importlib.import_module("nshogi-engine_amd")
    bb = np.load(os.path.join(HERE, "net_graph.npz"))["bitboards86"]
    x32 = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float32))
    torch.manual_seed(351)
    net = randomize(PoolNet(), 51).eval()
    with torch.no_grad():
        net.b3.prelu.weight.copy_(torch.rand(48) * 2.0 - 0.5)
    data = export_model(net, os.path.join(HERE, NAME + ".onnx"))
    assert b"BatchNormalization" in data
    with torch.no_grad():
        o32 = [t.numpy().astype(np.float64) for t in net(x32)]
        o64 = [t.numpy() for t in net.double()(x32.double())]
    err = max(float(np.abs(a.reshape(-1) - b.reshape(-1)).max()) for a, b in zip(o32, o64))
    assert err < 1e-5, err
    pol = o64[0].reshape(len(bb), -1)
    for half in range(2):
        np.savez_compressed(os.path.join(HERE, f"{NAME}_policy_{half}.npz"), policy=pol[32 * half:32 * (half + 1)])
    np.savez_compressed(os.path.join(HERE, "net_pool.npz"),
                        **{NAME + "_value": o64[1].reshape(-1), NAME + "_draw": o64[2].reshape(-1)})
    print(NAME, "onnx bytes", len(data), "float32 vs float64", f"{err:.2e}", "policy range", float(pol.min()),
          float(pol.max()))


if __name__ == "__main__":
    main()
