"""Models around the general graph path's grouped convolution (1 < group < Cin, DESIGN.md sections 13.2 to 13.4): the
shared half of tests/test_onnx_groupconv.py (host) and tests/test_gpu_onnx_groupconv.py (device).  Torch modules,
exported at test time through make_onnx_geometry_golden.export_model; nothing is added to tests/golden.

SHAPES is the table of (Cin, Cout, groups) the kernel can go wrong at:

  (32, 32, 8)    4 per group: eight groups inside one 16-channel chunk and one 16-channel output fragment
  (24, 24, 3)    pad channels 24..31; a half-empty last chunk
  (72, 48, 3)    24 inputs per group straddle chunk borders; Cin != Cout
  (64, 128, 4)   two tiles of 64 outputs; the second tile's chunk range does not start at chunk 0
  (128, 64, 4)   a wave's sub-range is two chunks of the tile's eight
  (160, 160, 2)  a group wider than a tile: the waves of tile 1 belong to two groups and have different sub-ranges
  (32, 24, 2)    12 outputs per group: a 16-channel output fragment straddles two groups
"""
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

import make_onnx_geometry_golden as gen  # noqa: E402
from make_onnx_geometry_golden import MeanHeads, conv  # noqa: E402

SHAPES = [(32, 32, 8), (24, 24, 3), (72, 48, 3), (64, 128, 4), (128, 64, 4), (160, 160, 2), (32, 24, 2)]
GEOMETRIES = [(1, 1), (5, 1), ((1, 9), 1), (3, 2)]  # beside 3x3: (kernel, dilation)
WIN = 27


def sid(v):
    return str(v).replace(" ", "").replace("(", "").replace(")", "").replace(",", "_")


def export(net, path, planes=86):
    return gen.export_model(net.float().eval(), str(path), planes)


def conv_flops(m):
    kh, kw = m.kernel_size
    return 2 * 81 * kh * kw * (m.in_channels // m.groups) * m.out_channels


def windows(cout):
    """Window starts of 27 channels that together show every output channel (the last one may overlap its neighbour)."""
    if cout <= WIN:
        return [0]
    return sorted(set(list(range(0, cout - WIN, WIN)) + [cout - WIN]))


class GroupTapNet(nn.Module):
    """The exact case, in TapNet's style: an integer 3x3 stem on the 0/1 planes (weights from {-1, 0, 1}, zero on the
    four planes that hold fractions) with ReLU, the grouped conv under test with weights from {-2..2} and an integer
    bias, and a 0/1 selection 1x1 conv that shows the 27 output channels from `start` (zero rows past Cout).  Every
    value is an integer; bound() is the largest magnitude a partial sum of the grouped conv can reach in any order."""

    def __init__(self, cin, cout, groups, k=3, d=1, start=0, seed=0, C=86, scalars=4):
        super().__init__()
        self.stem = conv(C, cin, 3)
        self.g = conv(cin, cout, k, d, groups=groups)
        self.sel = conv(cout, WIN, 1, bias=False)
        self.heads = MeanHeads(C)
        r = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.stem.weight.copy_(torch.randint(-1, 2, self.stem.weight.shape, generator=r).float())
            self.stem.weight[:, C - scalars:] = 0
            self.stem.bias.copy_(torch.randint(-3, 4, self.stem.bias.shape, generator=r).float())
            self.g.weight.copy_(torch.randint(-2, 3, self.g.weight.shape, generator=r).float())
            self.g.bias.copy_(torch.randint(-3, 4, self.g.bias.shape, generator=r).float())
            self.show(start)

    def show(self, start):
        with torch.no_grad():
            self.sel.weight.zero_()
            for j in range(min(WIN, self.g.out_channels - start)):
                self.sel.weight[j, start + j] = 1.0

    def bound(self):
        """max over outputs of sum |w| * (the stem's largest value) + |bias|, with the stem's own bound: sum |w| + |bias|
        on 0/1 planes."""
        with torch.no_grad():
            s = float((self.stem.weight.abs().sum(dim=(1, 2, 3)) + self.stem.bias.abs()).max())
            return s, float((self.g.weight.abs().sum(dim=(1, 2, 3)) * s + self.g.bias.abs()).max())

    def grouped(self, x):
        return self.g(torch.relu(self.stem(x)))

    def forward(self, x):
        return (torch.flatten(self.sel(self.grouped(x)), 1),) + self.heads(x)


class GroupNet(nn.Module):
    """3x3 stem to Cin, the grouped conv under test with its bias, a 1x1 policy head and mean heads over its output:
    every output depends on every channel of the grouped conv.  twin = True writes the same function as Split -> one
    group-1 Conv per group -> Concat, which runs on the dense kernels (twin_of copies the weights)."""

    def __init__(self, cin, cout, groups, k=3, d=1, twin=False, C=86):
        super().__init__()
        self.twin, self.groups, self.shape = twin, groups, (cin, cout, groups, k, d)
        self.stem = conv(C, cin, 3)
        if twin:
            self.parts = nn.ModuleList([conv(cin // groups, cout // groups, k, d) for _ in range(groups)])
        else:
            self.g = conv(cin, cout, k, d, groups=groups)
        self.p = conv(cout, WIN, 1)
        self.heads = MeanHeads(cout)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        if self.twin:
            xs = torch.split(x, x.shape[1] // self.groups, dim=1)
            x = torch.cat([m(part) for m, part in zip(self.parts, xs)], dim=1)
        else:
            x = self.g(x)
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


def twin_of(net):
    """The Split / Concat twin of a GroupNet, with the same weights."""
    twin = GroupNet(*net.shape, twin=True)
    co = net.g.out_channels // net.groups
    with torch.no_grad():
        for name in ("stem", "p", "heads"):
            getattr(twin, name).load_state_dict(getattr(net, name).state_dict())
        for i, m in enumerate(twin.parts):
            m.weight.copy_(net.g.weight[i * co:(i + 1) * co])
            m.bias.copy_(net.g.bias[i * co:(i + 1) * co])
    return twin


class GroupBlockNet(nn.Module):
    """3x3 stem, then relu(bn(g(x)) + x) with the grouped conv g (Cin = Cout): BatchNorm, a run-time residual and an
    activation in the grouped launch's epilogue.  full = False: the bare conv."""

    def __init__(self, F, groups, k=3, full=True, C=86):
        super().__init__()
        self.full = full
        self.stem = conv(C, F, 3)
        self.g = conv(F, F, k, groups=groups, bias=not full)
        self.bn = nn.BatchNorm2d(F) if full else None
        self.p = conv(F, WIN, 1)
        self.heads = MeanHeads(F)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        x = torch.relu(self.bn(self.g(x)) + x) if self.full else self.g(x)
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


class ResNeXtNet(nn.Module):
    """A ResNeXt-style net of width F: `blocks` blocks of 1x1 -> BatchNorm -> act -> k x k grouped -> BatchNorm -> act ->
    1x1 -> BatchNorm, the residual and act (ReLU, or swish in every second block when `swish`); GeomNet's heads.
    groups = 1 is its dense twin (scripts/graph_bench.py's row)."""

    def __init__(self, F=32, groups=4, blocks=3, k=3, swish=True, C=86, VC=4, VH=32):
        super().__init__()
        self.swish = swish
        self.stem, self.stem_bn = conv(C, F, 3, bias=False), nn.BatchNorm2d(F)
        self.a = nn.ModuleList([conv(F, F, 1, bias=False) for _ in range(blocks)])
        self.g = nn.ModuleList([conv(F, F, k, groups=groups, bias=False) for _ in range(blocks)])
        self.b = nn.ModuleList([conv(F, F, 1, bias=False) for _ in range(blocks)])
        self.a_bn, self.g_bn, self.b_bn = (nn.ModuleList([nn.BatchNorm2d(F) for _ in range(blocks)]) for _ in range(3))
        self.p = conv(F, WIN, 1)
        self.v = conv(F, VC, 1)
        self.fc1 = nn.Linear(VC * 81, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        x = torch.relu(self.stem_bn(self.stem(x)))
        for i, (a, g, b, a_bn, g_bn, b_bn) in enumerate(zip(self.a, self.g, self.b, self.a_bn, self.g_bn, self.b_bn)):
            act = Fn.silu if self.swish and i % 2 else torch.relu
            x = act(x + b_bn(b(act(g_bn(g(act(a_bn(a(x)))))))))
        policy = torch.flatten(self.p(x), 1)
        h = torch.relu(self.fc1(torch.flatten(torch.relu(self.v(x)), 1)))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class IsolationNet(nn.Module):
    """relu(stem) + a per-channel constant -> (64 -> 64, group 4) 3x3 -> the first 48 channels -> a 1x1 policy conv; value
    and draw read the stem in front of the Add.  With the constant inf in channels 48..63 (group 3, chunk 3) nothing the
    outputs read belongs to a group that shares a chunk with those channels."""

    def __init__(self, poison, C=86, F=64, groups=4, keep=48):
        super().__init__()
        self.keep = keep
        self.stem = conv(C, F, 3)
        c = torch.zeros(1, F, 1, 1)
        if poison:
            c[:, keep:] = float("inf")
        self.register_buffer("c", c)
        self.g = conv(F, F, 3, groups=groups)
        self.p = conv(keep, WIN, 1)
        self.heads = MeanHeads(F)

    def forward(self, x):
        s = torch.relu(self.stem(x))
        y = self.g(s + self.c)
        return (torch.flatten(self.p(y[:, :self.keep]), 1),) + self.heads(s)


class PadNet(nn.Module):
    """3x3 stem to 24 channels -> (24 -> 24, group 3) 3x3 with an activation fused -> a dense 3x3 conv to the policy: the
    dense conv's second chunk holds the grouped conv's pad channels 24..31, which must be zeros.  act "exp": a pad that
    went through the activation would be 1.  act "recip": integer weights >= 0 and a bias of 1 on the ReLU stem keep the
    grouped conv's outputs at 1 or above; a pad that went through it would be 1 / 0 = inf, and inf times the dense
    conv's zero weight is NaN in every policy channel."""

    def __init__(self, act, C=86, F=24, groups=3, seed=0):
        super().__init__()
        self.act = act
        self.stem = conv(C, F, 3)
        self.g = conv(F, F, 3, groups=groups)
        self.c2 = conv(F, WIN, 3)
        self.heads = MeanHeads(F)
        if act == "recip":
            r = torch.Generator().manual_seed(seed)
            with torch.no_grad():
                self.g.weight.copy_(torch.randint(0, 3, self.g.weight.shape, generator=r).float())
                self.g.bias.fill_(1.0)

    def forward(self, x):
        y = self.g(torch.relu(self.stem(x)))
        y = torch.exp(y) if self.act == "exp" else torch.reciprocal(y)
        return (torch.flatten(self.c2(y), 1),) + self.heads(y)


def randomize(net, seed):
    return gen.randomize(net, seed)
