"""Generates the elementwise-maths fixture of the general graph path (run from the repo root:
`python tests/golden/make_onnx_math_golden.py`): net_graph_math.onnx, net_math.npz (float64 value and draw) and the
float64 policy in two files, net_graph_math_policy_{0,1}.npz (positions 0-31 and 32-63, as for the other general-graph
fixtures).

net_graph_math is an 86-plane model of trunk width 32 that uses Exp, Log, Sqrt, Reciprocal and Pow on run-time tensors
and the three multi-node activations the planner recognises, each once on the way to its three outputs:

  * a 3x3 stem with BatchNorm and Mish, and a Mish residual block mish(x + bn(conv(mish(bn(conv(x))))));
  * a token FFN t + fc2(gelu_tanh(fc1(t)));
  * an RMS-style gate x * rsqrt(mean over the squares of x ** 2 + eps): Pow(x, 2) on a spatial tensor, the mean over
    the squares, Sqrt and Div(1, .) on the pooled flat tensor.  It is no RMSNorm: that one is over the last axis;
  * three branches of the gated tensor, log1p(|x|), (|x| + 0.5) ** 1.5 and x ** 2, mixed by a 1x1 conv, beside a
    softsign behind a 1x1 conv;
  * a 1x1 policy head scaled per (board, channel) by exp(clamp(fc(mean), -2, 2));
  * a value head on sqrt(|mean| + 0.25), the draw head on its reciprocal.

Every log, sqrt and fractional power gets an operand that is positive by construction (abs() + a constant); the
generator records the smallest operand of each in float64 and asserts it positive, and that every output is finite.  It
is exported with the siblings' recipe (make_onnx_golden.export: legacy TorchScript exporter, opset 17, dynamic batch
axis).  The positions are the 86-plane positions of net_graph.npz.  The generator asserts that float32 PyTorch agrees
with the float64 outputs it stores to better than 1e-5.

The module classes are importable: tests/test_onnx_math.py and tests/test_gpu_onnx_math.py export small models built
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

from make_onnx_attention_golden import tokens  # noqa: E402
from make_onnx_geometry_golden import MeanHeads, conv  # noqa: E402,F401
from make_onnx_norm_golden import export_model  # noqa: E402,F401  (make_onnx_golden.export at opset 17)


def gelu_tanh_pow(x):
    """tanh-GELU as hand-written code has it: Pow(x, 3) in place of the exporter's two Muls."""
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * torch.pow(x, 3.0))))


def back(x, t):
    return t.transpose(1, 2).reshape(x.size(0), -1, 9, 9)


class MishBlock(nn.Module):
    def __init__(self, F, act=Fn.mish):
        super().__init__()
        self.act = act
        self.c1, self.n1 = conv(F, F, 3, bias=False), nn.BatchNorm2d(F)
        self.c2, self.n2 = conv(F, F, 3, bias=False), nn.BatchNorm2d(F)

    def forward(self, x):
        return self.act(x + self.n2(self.c2(self.act(self.n1(self.c1(x))))))


class GeluFFN(nn.Module):
    def __init__(self, F, ffn):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(F, ffn), nn.Linear(ffn, F)

    def forward(self, t):
        return t + self.fc2(Fn.gelu(self.fc1(t), approximate="tanh"))


class MathFixtureNet(nn.Module):
    """The fixture.  With `record` set, forward notes the smallest operand of every log, sqrt and fractional power."""

    def __init__(self, C=86, F=32, VH=24):
        super().__init__()
        self.F, self.record, self.operands = F, False, {}
        self.stem, self.stem_n = conv(C, F, 3, bias=False), nn.BatchNorm2d(F)
        self.b1 = MishBlock(F)
        self.ffn = GeluFFN(F, 2 * F)
        self.cs, self.cm = conv(F, F, 1), conv(F, F, 1)
        self.p = conv(F, 27, 1)
        self.fc_l = nn.Linear(F, 27)
        self.fc1 = nn.Linear(F, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def positive(self, name, t):
        if self.record:
            self.operands[name] = float(t.min())
        return t

    def forward(self, x):
        x = Fn.mish(self.stem_n(self.stem(x)))
        x = self.b1(x)
        x = back(x, self.ffn(tokens(x)))
        ms = self.positive("rsqrt", x.pow(2).mean(dim=(2, 3)) + 1e-3)
        x = x * torch.rsqrt(ms)[:, :, None, None]
        a = torch.log(self.positive("log", x.abs() + 1.0))  # log1p(|x|) as the exporter writes it
        b = self.positive("pow", x.abs() + 0.5) ** 1.5
        x = Fn.softsign(self.cs(x)) + self.cm(a + 0.25 * b - 0.1 * x ** 2)
        m = x.mean(dim=(2, 3))
        scale = torch.exp(torch.clamp(self.fc_l(m), -2.0, 2.0))
        policy = torch.flatten(self.p(x) * scale[:, :, None, None], 1)
        h = torch.relu(self.fc1(m))
        h = torch.sqrt(self.positive("sqrt", h.abs() + 0.25))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(torch.reciprocal(h)))


class Front(nn.Module):
    """The smallest model around `f`: a k x k stem of C channels (with a BatchNorm when `bn`), x = f(stem), a 1x1 policy
    head and mean heads.  domain "token": f runs on the tokens [N,81,C] behind a Linear, then back to [N,C,9,9];
    "norm": f runs behind a GroupNorm of 3 groups.  split: the stem has 2 C channels, f runs on the second half (so no
    conv absorbs it) and the heads read the first.  f = None is the identity: the launch count the planner tests
    compare with."""

    def __init__(self, f, C=24, k=1, bn=False, domain="spatial", split=False, planes=86):
        super().__init__()
        self.f, self.C, self.domain, self.split = f, C, domain, split
        self.stem = conv(planes, 2 * C if split else C, k, bias=not bn)
        self.bn = nn.BatchNorm2d(C) if bn else None
        self.fc = nn.Linear(C, C) if domain == "token" else None
        self.gn = nn.GroupNorm(3, C) if domain == "norm" else None
        self.p = conv(C, 27, 1)
        self.heads = MeanHeads(C)

    def forward(self, x):
        x = self.stem(x)
        if self.split:
            a, x = torch.split(x, [self.C, self.C], dim=1)
        if self.bn is not None:
            x = self.bn(x)
        f = self.f if self.f is not None else (lambda t: t)
        if self.domain == "token":
            x = back(x, f(self.fc(tokens(x))))
        elif self.domain == "norm":
            x = f(self.gn(x))
        else:
            x = f(x)
        return (torch.flatten(self.p(x), 1),) + self.heads(a if self.split else x)


class MishSweepNet(nn.Module):
    """The width sweep's model: a cin-channel Mish stem, conv(cin, cout) -> BN -> Mish, and conv(cout, cout) -> BN with
    a residual and Mish behind it."""

    def __init__(self, cin, cout, planes=86):
        super().__init__()
        self.stem, self.stem_n = conv(planes, cin, 3, bias=False), nn.BatchNorm2d(cin)
        self.c1, self.n1 = conv(cin, cout, 3, bias=False), nn.BatchNorm2d(cout)
        self.c2, self.n2 = conv(cout, cout, 3, bias=False), nn.BatchNorm2d(cout)
        self.p = conv(cout, 27, 1)
        self.heads = MeanHeads(cout)

    def forward(self, x):
        x = Fn.mish(self.stem_n(self.stem(x)))
        x = Fn.mish(self.n1(self.c1(x)))
        x = Fn.mish(x + self.n2(self.c2(x)))
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


class MishBenchNet(nn.Module):
    """scripts/graph_bench.py's Mish row: the 20x256 residual net with Mish for every ReLU; with act = Fn.silu the same
    net with swish, the row it is timed beside."""

    def __init__(self, C=86, F=256, blocks=20, VH=256, act=Fn.mish):
        super().__init__()
        self.act = act
        self.stem, self.stem_n = conv(C, F, 3, bias=False), nn.BatchNorm2d(F)
        self.blocks = nn.ModuleList([MishBlock(F, act) for _ in range(blocks)])
        self.p = conv(F, 27, 1)
        self.fc1 = nn.Linear(F, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        x = self.act(self.stem_n(self.stem(x)))
        for b in self.blocks:
            x = b(x)
        h = self.act(self.fc1(x.mean(dim=(2, 3))))
        return torch.flatten(self.p(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


def randomize(net, seed):
    """BatchNorm and GroupNorm parameters and statistics, and every bias, away from their defaults."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
                if isinstance(m, nn.BatchNorm2d):
                    m.running_mean.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                    m.running_var.copy_(torch.rand(m.bias.shape, generator=g) + 0.5)
            elif isinstance(m, (nn.Linear, nn.Conv2d)) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return net


NAME = "net_graph_math"


def main():
    nsg = importlib.import_module("nshogi-engine_amd")
    bb = np.load(os.path.join(HERE, "net_graph.npz"))["bitboards86"]
    x32 = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float32))
    torch.manual_seed(362)
    net = randomize(MathFixtureNet(), 62).eval()
    data = export_model(net, os.path.join(HERE, NAME + ".onnx"))
    for op in (b"Exp", b"Log", b"Sqrt", b"Reciprocal", b"Pow", b"Softplus", b"Tanh", b"Abs", b"Clip"):
        assert op in data, op
    with torch.no_grad():
        o32 = [t.numpy().astype(np.float64) for t in net(x32)]
        net.record = True
        o64 = [t.numpy() for t in net.double()(x32.double())]
    assert sorted(net.operands) == ["log", "pow", "rsqrt", "sqrt"] and min(net.operands.values()) > 0, net.operands
    assert all(np.isfinite(o).all() for o in o64)
    err = max(float(np.abs(a.reshape(-1) - b.reshape(-1)).max()) for a, b in zip(o32, o64))
    assert err < 1e-5, err
    pol = o64[0].reshape(len(bb), -1)
    for half in range(2):
        np.savez_compressed(os.path.join(HERE, f"{NAME}_policy_{half}.npz"), policy=pol[32 * half:32 * (half + 1)])
    np.savez_compressed(os.path.join(HERE, "net_math.npz"),
                        **{NAME + "_value": o64[1].reshape(-1), NAME + "_draw": o64[2].reshape(-1)})
    print(NAME, "onnx bytes", len(data), "float32 vs float64", f"{err:.2e}", "policy range", float(pol.min()),
          float(pol.max()), "smallest operands", net.operands)


if __name__ == "__main__":
    main()
