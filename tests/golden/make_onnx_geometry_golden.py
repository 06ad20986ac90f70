"""Generates the convolution-geometry fixture of the general graph path (run from the repo root:
`python tests/golden/make_onnx_geometry_golden.py`): net_graph_geom.onnx, net_geom.npz (float64 value and draw) and the
float64 policy in two files, net_graph_geom_policy_{0,1}.npz (positions 0-31 and 32-63, as for the other general-graph
fixtures: one file would exceed the repository's 1 MiB limit).

net_graph_geom is an 86-plane model of width F = 32 built from the convolutions outside 1x1 and 3x3 at dilation 1:

  * a 5x5 stem with BatchNorm and ReLU;
  * a "cross" residual block, relu(x + row(x) + col(x)) with a 1x9 and a 9x1 conv (files and ranks of the 9x9 board);
  * a depthwise 7x7 -> BatchNorm -> pointwise 1x1 block with a swish residual, swish(x + pw(bn(dw(x))));
  * a dilated 3x3 (dilation 2) residual block;
  * a 1x1 policy head and a value / draw head over a flattened 1x1 conv.

It is exported with the recipe of make_onnx_golden.py (legacy TorchScript exporter, opset 17, dynamic batch axis) with
the BatchNormalization nodes kept, so that the planner folds them: behind the depthwise conv they go into its
per-channel taps.  The positions are the 86-plane positions of net_graph.npz.  The generator asserts that float32
PyTorch agrees with the float64 outputs it stores to better than 1e-5.

The module classes are importable: tests/test_onnx_geometry.py and tests/test_gpu_onnx_geometry.py export small
variants of them at test time.
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

import make_onnx_golden  # noqa: E402  (the shared exporter recipe)
from make_onnx_graph_golden import randomize_bn  # noqa: E402


def pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def halo(k, d=1):
    (kh, kw), (dh, dw) = pair(k), pair(d)
    return dh * (kh - 1) // 2, dw * (kw - 1) // 2


def conv(cin, cout, k, d=1, groups=1, bias=True):
    """A conv that keeps the 9x9 board: kernel k (an int or (kh, kw)), dilation d, pads equal to the halo."""
    return nn.Conv2d(cin, cout, pair(k), padding=halo(k, d), dilation=pair(d), groups=groups, bias=bias)


class MeanHeads(nn.Module):
    """Value and draw from the mean over the squares: the smallest head the tensor contract allows."""

    def __init__(self, F):
        super().__init__()
        self.fc_v, self.fc_d = nn.Linear(F, 1), nn.Linear(F, 1)

    def forward(self, x):
        h = x.mean(dim=(2, 3))
        return torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class GeomNet(nn.Module):
    """The fixture."""

    def __init__(self, C=86, F=32, VC=4, VH=32):
        super().__init__()
        self.stem, self.stem_bn = conv(C, F, 5, bias=False), nn.BatchNorm2d(F)
        self.row, self.col = conv(F, F, (1, 9)), conv(F, F, (9, 1))
        self.dw, self.dw_bn, self.pw = conv(F, F, 7, groups=F, bias=False), nn.BatchNorm2d(F), conv(F, F, 1)
        self.d1, self.d1_bn, self.d2 = conv(F, F, 3, 2, bias=False), nn.BatchNorm2d(F), conv(F, F, 3, 2)
        self.p = conv(F, 27, 1)
        self.v = conv(F, VC, 1)
        self.fc1 = nn.Linear(VC * 81, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        x = torch.relu(self.stem_bn(self.stem(x)))
        x = torch.relu(x + self.row(x) + self.col(x))
        x = Fn.silu(x + self.pw(self.dw_bn(self.dw(x))))
        x = torch.relu(x + self.d2(torch.relu(self.d1_bn(self.d1(x)))))
        policy = torch.flatten(self.p(x), 1)
        h = torch.relu(self.fc1(torch.flatten(torch.relu(self.v(x)), 1)))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class GeomBenchNet(nn.Module):
    """scripts/graph_bench.py's geometry row: a 5x5 stem and `blocks` residual blocks of width F, every `wide_every`-th
    one two 5x5 convs with BatchNorm and ReLU, the others depthwise 7x7 -> BatchNorm -> pointwise 1x1 with a swish
    residual; the fixture's heads.  No 3x3 conv, so a kernel trace tells its launches from the family net's."""

    def __init__(self, C=86, F=256, blocks=20, wide_every=5, VC=32, VH=256):
        super().__init__()
        self.stem, self.stem_bn = conv(C, F, 5, bias=False), nn.BatchNorm2d(F)
        self.wide = [i % wide_every == 0 for i in range(blocks)]
        self.a = nn.ModuleList([conv(F, F, 5, bias=False) if w else conv(F, F, 7, groups=F, bias=False) for w in self.wide])
        self.a_bn = nn.ModuleList([nn.BatchNorm2d(F) for _ in self.wide])
        self.b = nn.ModuleList([conv(F, F, 5, bias=False) if w else conv(F, F, 1) for w in self.wide])
        self.b_bn = nn.ModuleList([nn.BatchNorm2d(F) if w else nn.Identity() for w in self.wide])
        self.p = conv(F, 27, 1)
        self.v = conv(F, VC, 1)
        self.fc1 = nn.Linear(VC * 81, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        x = torch.relu(self.stem_bn(self.stem(x)))
        for w, a, a_bn, b, b_bn in zip(self.wide, self.a, self.a_bn, self.b, self.b_bn):
            if w:
                x = torch.relu(x + b_bn(b(torch.relu(a_bn(a(x))))))
            else:
                x = Fn.silu(x + b(a_bn(a(x))))
        policy = torch.flatten(self.p(x), 1)
        h = torch.relu(self.fc1(torch.flatten(torch.relu(self.v(x)), 1)))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class StemNet(nn.Module):
    """relu(stem(planes)), a 1x1 policy head and mean heads around any first conv: the refusal tests' model."""

    def __init__(self, stem):
        super().__init__()
        self.stem = stem
        self.p = nn.Conv2d(stem.out_channels, 27, 1)
        self.heads = MeanHeads(stem.out_channels)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


class TapNet(nn.Module):
    """policy = Conv(86 -> 27, kernel k, dilation d) applied to the 0/1 planes with integer weights from {-2..2} and an
    integer bias: every partial sum is a small integer, so float32 in any order must give the float64 result.  The last
    `scalars` planes of the feature set hold fractions, not 0/1 (86 planes: the four hand-count and ply planes): their
    taps are zero, and 0 * x leaves the integers alone."""

    def __init__(self, k, d=1, C=86, seed=0, scalars=4):
        super().__init__()
        self.p = conv(C, 27, k, d)
        self.heads = MeanHeads(C)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.p.weight.copy_(torch.randint(-2, 3, self.p.weight.shape, generator=g).float())
            self.p.weight[:, C - scalars:] = 0
            self.p.bias.copy_(torch.randint(-3, 4, self.p.bias.shape, generator=g).float())

    def forward(self, x):
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


class DwTapNet(nn.Module):
    """The exact depthwise case: integer per-channel taps over the 86 planes, then an integer 1x1 to 27 channels (zero
    on the last `scalars` planes, see TapNet)."""

    def __init__(self, k, d=1, C=86, seed=0, scalars=4):
        super().__init__()
        self.dw = conv(C, C, k, d, groups=C)
        self.p = conv(C, 27, 1)
        self.heads = MeanHeads(C)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for m in (self.dw, self.p):
                m.weight.copy_(torch.randint(-2, 3, m.weight.shape, generator=g).float())
                m.bias.copy_(torch.randint(-3, 4, m.bias.shape, generator=g).float())
            self.p.weight[:, C - scalars:] = 0

    def forward(self, x):
        return (torch.flatten(self.p(self.dw(x)), 1),) + self.heads(x)


class RingNet(nn.Module):
    """A two-block residual net of width F whose convs all have kernel k (3 or 5)."""

    def __init__(self, k, F=24, C=86, blocks=2):
        super().__init__()
        self.stem = conv(C, F, k)
        self.c1 = nn.ModuleList([conv(F, F, k) for _ in range(blocks)])
        self.c2 = nn.ModuleList([conv(F, F, k) for _ in range(blocks)])
        self.p = conv(F, 27, 1)
        self.heads = MeanHeads(F)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        for a, b in zip(self.c1, self.c2):
            x = torch.relu(x + b(torch.relu(a(x))))
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


def zero_ring_copy(small, k=5):
    """The RingNet of kernel k that holds `small`'s 3x3 kernels at its centres and zeros around them."""
    big = RingNet(k, F=small.stem.out_channels, blocks=len(small.c1))
    sd, r = small.state_dict(), (k - 3) // 2
    with torch.no_grad():
        for name, t in big.state_dict().items():
            s = sd[name]
            if s.shape == t.shape:
                t.copy_(s)
            else:
                t.zero_()
                t[:, :, r:r + 3, r:r + 3] = s
    return big


class BlockNet(nn.Module):
    """3x3 stem to Cin, then relu(bn(conv(x)) + skip(x)) with the conv under test (Cin -> Cout, kernel k, dilation d)
    and a 1x1 skip: BatchNorm, a runtime residual and an activation in the new kernel's epilogue."""

    def __init__(self, cin, cout, k, d=1, C=86):
        super().__init__()
        self.stem = conv(C, cin, 3)
        self.skip = conv(cin, cout, 1)
        self.c, self.bn = conv(cin, cout, k, d, bias=False), nn.BatchNorm2d(cout)
        self.p = conv(cout, 27, 1)
        self.heads = MeanHeads(cout)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        x = torch.relu(self.bn(self.c(x)) + self.skip(x))
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


class DwNet(nn.Module):
    """3x3 stem to F channels, then the depthwise conv under test: bare with its bias (full = False), or
    swish(x + bn(dw(x))) (full = True)."""

    def __init__(self, F, k, d=1, full=True, C=86):
        super().__init__()
        self.full = full
        self.stem = conv(C, F, 3)
        self.dw = conv(F, F, k, d, groups=F, bias=not full)
        self.bn = nn.BatchNorm2d(F) if full else None
        self.p = conv(F, 27, 1)
        self.heads = MeanHeads(F)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        x = Fn.silu(x + self.bn(self.dw(x))) if self.full else self.dw(x)
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


def randomize(net, seed):
    """BatchNorm statistics and every bias away from their defaults."""
    randomize_bn(net, seed)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.Linear, nn.Conv2d)) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return net


def export_model(net, path, planes=86, fold=False):
    """fold = False keeps the BatchNormalization nodes in the file: the planner folds them."""
    make_onnx_golden.C = planes  # the exporter's dummy input shape
    return make_onnx_golden.export(net, path, fold)


NAME = "net_graph_geom"


def main():
    nsg = importlib.import_module("nshogi-engine_amd")
    bb = np.load(os.path.join(HERE, "net_graph.npz"))["bitboards86"]
    x32 = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float32))
    torch.manual_seed(341)
    net = randomize(GeomNet(), 41).eval()
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
    np.savez_compressed(os.path.join(HERE, "net_geom.npz"),
                        **{NAME + "_value": o64[1].reshape(-1), NAME + "_draw": o64[2].reshape(-1)})
    print(NAME, "onnx bytes", len(data), "float32 vs float64", f"{err:.2e}", "policy range", float(pol.min()),
          float(pol.max()))


if __name__ == "__main__":
    main()
