"""Generates the normalisation fixture of the general graph path (run from the repo root:
`python tests/golden/make_onnx_norm_golden.py`): net_graph_norm.onnx, net_norm.npz (float64 value and draw) and the
float64 policy in two files, net_graph_norm_policy_{0,1}.npz (positions 0-31 and 32-63, as for the other general-graph
fixtures).

net_graph_norm is an 86-plane model of trunk width 32 without a single BatchNorm, which uses every normalisation that
needs no batch statistics once on the way to its three outputs:

  * a 3x3 stem with GroupNorm(4 groups) and ReLU;
  * a GN-ReLU residual block: relu(x + gn(conv(relu(gn(conv(x)))))) with 8 groups of 4 channels;
  * a 1x1 conv with an affine InstanceNorm2d and ReLU;
  * a ConvNeXt-style block: depthwise 3x3, LayerNorm over the channels in the channel-last view
    (permute(0, 2, 3, 1), LayerNorm, permute(0, 3, 1, 2)), 1x1 expand, GELU, 1x1 project, residual;
  * an RMSNorm pre-norm token block: t + fc2(relu(fc1(rmsnorm(t)))), the RMSNorm written by hand (nn.RMSNorm does
    not export at these opsets);
  * a LayerNorm over the tokens' channels written out in elementary ops (what the exporter makes of nn.LayerNorm below
    opset 17), then back to [N,32,9,9];
  * a 1x1 policy head, and a value head mean -> fc -> relu -> RMSNorm on the flat tensor -> sigmoid value and draw.

Every gamma, beta and bias is randomised away from its default.  It is exported with the siblings' recipe (legacy
TorchScript exporter, opset 17, dynamic batch axis); export_model here takes the opset as well, because the tests
export LayerNorm at opset 13 too.  The positions are the 86-plane positions of net_graph.npz.  The generator asserts that
float32 PyTorch agrees with the float64 outputs it stores to better than 1e-5: the reference alone stays far inside
the tests' bound, and a near-constant group blown up by 1 / sqrt(var + eps) would show here.

The module classes are importable: tests/test_onnx_norm.py and tests/test_gpu_onnx_norm.py export small models built
from them at test time.
"""
import importlib
import io
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

import make_onnx_golden  # noqa: E402
from make_onnx_attention_golden import tokens  # noqa: E402
from make_onnx_geometry_golden import MeanHeads, conv  # noqa: E402,F401


class ChanLastLN(nn.Module):
    """LayerNorm over the channels of a spatial tensor, the ConvNeXt way."""

    def __init__(self, C, eps=1e-6):
        super().__init__()
        self.ln = nn.LayerNorm(C, eps=eps)

    def forward(self, x):
        return self.ln(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class DecomposedLN(nn.Module):
    """LayerNorm over the last axis in elementary ops, the chain the exporter writes for nn.LayerNorm below opset 17.
    square: "pow" or "mul"; gamma / beta can be left out."""

    def __init__(self, C, eps=1e-5, square="pow", gamma=True, beta=True):
        super().__init__()
        self.eps, self.square = eps, square
        self.weight = nn.Parameter(torch.ones(C)) if gamma else None
        self.bias = nn.Parameter(torch.zeros(C)) if beta else None

    def forward(self, x):
        d = x - x.mean(-1, keepdim=True)
        v = (d.pow(2) if self.square == "pow" else d * d).mean(-1, keepdim=True)
        y = d / torch.sqrt(v + self.eps)
        if self.weight is not None:
            y = y * self.weight
        return y + self.bias if self.bias is not None else y


class RMSNorm(nn.Module):
    """RMSNorm over the last axis as people write it by hand.  form "rsqrt": x * rsqrt(mean(x^2) + eps) * w;
    form "div": w * (x / sqrt(mean(x * x) + eps))."""

    def __init__(self, C, eps=1e-6, form="rsqrt"):
        super().__init__()
        self.eps, self.form = eps, form
        self.weight = nn.Parameter(torch.ones(C))

    def forward(self, x):
        if self.form == "rsqrt":
            return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + self.eps) * self.weight
        return self.weight * (x / torch.sqrt((x * x).mean(-1, keepdim=True) + self.eps))


NORMS = (nn.GroupNorm, nn.InstanceNorm2d, nn.LayerNorm, DecomposedLN, RMSNorm)


def randomize(net, seed):
    """gamma and beta of every normalisation and every bias away from their defaults."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, NORMS):
                if getattr(m, "weight", None) is not None:
                    m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                if getattr(m, "bias", None) is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
            elif isinstance(m, (nn.Linear, nn.Conv2d)) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return net


class GNBlock(nn.Module):
    def __init__(self, F, G):
        super().__init__()
        self.c1, self.n1 = conv(F, F, 3), nn.GroupNorm(G, F)
        self.c2, self.n2 = conv(F, F, 3), nn.GroupNorm(G, F)

    def forward(self, x):
        return torch.relu(x + self.n2(self.c2(torch.relu(self.n1(self.c1(x))))))


class ConvNeXtBlock(nn.Module):
    def __init__(self, F, E):
        super().__init__()
        self.dw = conv(F, F, 3, groups=F)
        self.ln = ChanLastLN(F)
        self.pw1, self.pw2 = conv(F, E, 1), conv(E, F, 1)

    def forward(self, x):
        return x + self.pw2(Fn.gelu(self.pw1(self.ln(self.dw(x)))))


class RMSTokenBlock(nn.Module):
    def __init__(self, F, ffn, form="rsqrt"):
        super().__init__()
        self.norm = RMSNorm(F, form=form)
        self.fc1, self.fc2 = nn.Linear(F, ffn), nn.Linear(ffn, F)

    def forward(self, t):
        return t + self.fc2(torch.relu(self.fc1(self.norm(t))))


class NormFixtureNet(nn.Module):
    """The fixture."""

    def __init__(self, C=86, F=32, VH=24):
        super().__init__()
        self.F = F
        self.stem, self.stem_n = conv(C, F, 3), nn.GroupNorm(4, F)
        self.b1 = GNBlock(F, 8)
        self.ci, self.inorm = conv(F, F, 1), nn.InstanceNorm2d(F, affine=True)
        self.b2 = ConvNeXtBlock(F, 2 * F)
        self.b3 = RMSTokenBlock(F, 2 * F)
        self.dln = DecomposedLN(F)
        self.p = conv(F, 27, 1)
        self.fc1, self.vnorm = nn.Linear(F, VH), RMSNorm(VH, form="div")
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        N = x.size(0)
        x = torch.relu(self.stem_n(self.stem(x)))
        x = self.b1(x)
        x = torch.relu(self.inorm(self.ci(x)))
        x = self.b2(x)
        t = self.dln(self.b3(tokens(x)))
        x = t.transpose(1, 2).reshape(N, self.F, 9, 9)
        h = self.vnorm(torch.relu(self.fc1(x.mean(dim=(2, 3)))))
        return torch.flatten(self.p(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class NormNet(nn.Module):
    """The smallest model around one normalisation `mid`: a 3x3 stem to C channels with ReLU, `mid`, a 1x1 policy head
    and mean heads.  domain: "spatial" (mid on [N,C,9,9]), "token" (mid on the tokens [N,81,C], then back to
    [N,C,9,9]), "flat" (mid on the mean over the squares, in front of the value heads).  act: a ReLU behind mid.
    nn.Identity() as mid gives the launch count the planner tests compare with."""

    def __init__(self, C, mid, domain="spatial", act=False, planes=86):
        super().__init__()
        self.C, self.mid, self.domain, self.act = C, mid, domain, act
        self.stem = conv(planes, C, 3)
        self.p = conv(C, 27, 1)
        self.heads = MeanHeads(C)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        if self.domain == "spatial":
            x = self.mid(x)
        elif self.domain == "token":
            x = self.mid(tokens(x)).transpose(1, 2).reshape(x.size(0), self.C, 9, 9)
        if self.act:
            x = torch.relu(x)
        h = x.mean(dim=(2, 3))
        if self.domain == "flat":
            h = self.mid(h)
        return torch.flatten(self.p(x), 1), torch.sigmoid(self.heads.fc_v(h)), torch.sigmoid(self.heads.fc_d(h))


class GNSweepNet(nn.Module):
    """The GroupNorm sweep's model at (C, G).  full = False: the bare normalisation without gamma and beta behind the
    stem; full = True: relu(x + gn(conv(relu(gn(conv(x)))))), gamma and beta, a fused ReLU and a residual.  split > 0:
    the stem has C + split channels, torch.split gives [split, C], and the normalisation reads the second part where
    it lies, at channel offset `split`."""

    def __init__(self, C, G, full, split=0, planes=86):
        super().__init__()
        self.C, self.full, self.split = C, full, split
        self.stem = conv(planes, C + split, 3)
        self.block = GNBlock(C, G) if full else nn.GroupNorm(G, C, affine=False)
        self.p = conv(C + split, 27, 1)
        self.heads = MeanHeads(C + split)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        if self.split:
            a, b = torch.split(x, [self.split, self.C], dim=1)
            x = torch.cat([a, self.block(b)], dim=1)
        else:
            x = self.block(x)
        return (torch.flatten(self.p(x), 1),) + self.heads(x)


class NormBenchNet(nn.Module):
    """scripts/graph_bench.py's normalisation row: the 20x256 residual net with GroupNorm(32 groups)-ReLU in place of
    every BatchNorm-ReLU."""

    def __init__(self, C=86, F=256, blocks=20, G=32, VH=256):
        super().__init__()
        self.stem, self.stem_n = conv(C, F, 3), nn.GroupNorm(G, F)
        self.blocks = nn.ModuleList([GNBlock(F, G) for _ in range(blocks)])
        self.p = conv(F, 27, 1)
        self.fc1 = nn.Linear(F, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        x = torch.relu(self.stem_n(self.stem(x)))
        for b in self.blocks:
            x = b(x)
        h = torch.relu(self.fc1(x.mean(dim=(2, 3))))
        return torch.flatten(self.p(x), 1), torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


def export_model(net, path, planes=86, fold=True, opset=17):
    """The siblings' recipe (make_onnx_golden.export) at opset 17; the same call at another opset otherwise."""
    make_onnx_golden.C = planes  # the exporter's dummy input shape
    if opset == 17:
        return make_onnx_golden.export(net, path, fold)
    from torch.onnx._internal.torchscript_exporter import onnx_proto_utils
    onnx_proto_utils._add_onnxscript_fn = lambda proto, custom_opsets: proto  # see make_onnx_golden's docstring
    buf = io.BytesIO()
    torch.onnx.export(net, (torch.zeros(1, planes, 9, 9),), buf, input_names=["input"],
                      output_names=["policy", "value", "draw"], dynamo=False, opset_version=opset,
                      dynamic_axes={"input": {0: "N"}, "policy": {0: "N"}, "value": {0: "N"}, "draw": {0: "N"}},
                      do_constant_folding=fold,
                      training=torch.onnx.TrainingMode.EVAL if fold else torch.onnx.TrainingMode.PRESERVE)
    with open(path, "wb") as f:
        f.write(buf.getvalue())
    return buf.getvalue()


NAME = "net_graph_norm"


def main():
    nsg = importlib.import_module("nshogi-engine_amd")
    bb = np.load(os.path.join(HERE, "net_graph.npz"))["bitboards86"]
    x32 = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float32))
    torch.manual_seed(361)
    net = randomize(NormFixtureNet(), 61).eval()
    data = export_model(net, os.path.join(HERE, NAME + ".onnx"))
    for op in (b"InstanceNormalization", b"LayerNormalization", b"ReduceMean", b"Sqrt", b"Pow"):
        assert op in data, op
    with torch.no_grad():
        o32 = [t.numpy().astype(np.float64) for t in net(x32)]
        o64 = [t.numpy() for t in net.double()(x32.double())]
    err = max(float(np.abs(a.reshape(-1) - b.reshape(-1)).max()) for a, b in zip(o32, o64))
    assert err < 1e-5, err
    pol = o64[0].reshape(len(bb), -1)
    for half in range(2):
        np.savez_compressed(os.path.join(HERE, f"{NAME}_policy_{half}.npz"), policy=pol[32 * half:32 * (half + 1)])
    np.savez_compressed(os.path.join(HERE, "net_norm.npz"),
                        **{NAME + "_value": o64[1].reshape(-1), NAME + "_draw": o64[2].reshape(-1)})
    print(NAME, "onnx bytes", len(data), "float32 vs float64", f"{err:.2e}", "policy range", float(pol.min()),
          float(pol.max()))


if __name__ == "__main__":
    main()
