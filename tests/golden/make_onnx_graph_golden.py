"""Generates the general-graph fixtures (run from the repo root: `python tests/golden/make_onnx_graph_golden.py`):
net_graph_se.onnx, net_graph_gpool93.onnx, net_graph_softplus.onnx and net_graph.npz.

The three models lie outside the ResNet family the specialised path runs, and are built only from the op set of
DESIGN.md section 13.  They are exported with the same recipe as make_onnx_golden.py (legacy TorchScript exporter,
opset 17, dynamic batch axis):

  (a) net_graph_se       86 planes, 2 SE-ResNet blocks of width 32: swish activations, squeeze-and-excitation whose
                         FC output is `chunk`ed into a scale half and a bias half, BatchNorm folded by the exporter;
                         a two-layer policy head (1x1 + ReLU + 1x1); a value head reading the concat of a flattened
                         1x1 value conv and the globally pooled trunk; sigmoid value and sigmoid draw.
  (b) net_graph_gpool93  93 planes (CustomFeaturesV1), 1 block with a global-pooling bias, BatchNormalization nodes
                         kept with epsilon 1e-4, a BatchNorm after the residual add, a value head of MatMul + Add
                         and outputs squeezed to [N]; shape chains from `view(x.size(0), -1)` left unfolded.
  (c) net_graph_softplus 86 planes, Softplus and Tanh activations; `policy` written as [N, 27, 9, 9].
  (d) net_graph_views    86 planes, view ops right behind elementwise chains: a same-shape `view` of x * 0.5 read
                         by a conv, a KataGo-style value head fc(flatten(relu(v_conv(x) + gfc(mean(x)).view(N,-1,1,1)))),
                         and policy = flatten(p_conv(x) * 0.5) * 2.

net_graph.npz holds 64 positions per plane count (the 6 positions of net_torch.npz plus seeded synthetic ones for 86
planes, seeded synthetic ones for 93) and each model's float64 PyTorch value and draw outputs.  The float64 policy
outputs (64 x 2187 per model) would exceed the repository's 1 MiB file limit in one file, so they go into two files per
model, net_graph_<model>_policy_{0,1}.npz, for positions 0-31 and 32-63 (tests/test_gpu_onnx_graph.py joins them).
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
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_onnx_golden import export  # noqa: E402  (the shared exporter recipe)


def randomize_bn(net, seed, eps=None):
    g = torch.Generator().manual_seed(seed)
    for m in net.modules():
        if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
            n = m.num_features
            m.weight.data = torch.rand(n, generator=g) + 0.5
            m.bias.data = torch.randn(n, generator=g) * 0.1
            m.running_mean = torch.randn(n, generator=g) * 0.1
            m.running_var = torch.rand(n, generator=g) + 0.5
            if eps is not None:
                m.eps = eps
    return net


class SEBlock(nn.Module):
    def __init__(self, f, r=16):
        super().__init__()
        self.c1 = nn.Conv2d(f, f, 3, padding=1, bias=False)
        self.b1 = nn.BatchNorm2d(f)
        self.c2 = nn.Conv2d(f, f, 3, padding=1, bias=False)
        self.b2 = nn.BatchNorm2d(f)
        self.fc1 = nn.Linear(f, r)
        self.fc2 = nn.Linear(r, 2 * f)

    def forward(self, x):
        y = Fn.silu(self.b1(self.c1(x)))
        y = self.b2(self.c2(y))
        s = Fn.adaptive_avg_pool2d(y, 1).flatten(1)
        s = self.fc2(torch.relu(self.fc1(s)))
        w, b = torch.chunk(s, 2, dim=1)
        y = torch.sigmoid(w).view(x.size(0), -1, 1, 1) * y + b.view(x.size(0), -1, 1, 1)
        return Fn.silu(x + y)


class SENet(nn.Module):
    def __init__(self, C=86, F=32, blocks=2, VC=4, VH=32):
        super().__init__()
        self.stem = nn.Conv2d(C, F, 3, padding=1, bias=False)
        self.stem_bn = nn.BatchNorm2d(F)
        self.blocks = nn.ModuleList([SEBlock(F) for _ in range(blocks)])
        self.p1 = nn.Conv2d(F, F, 1)
        self.p2 = nn.Conv2d(F, 27, 1)
        self.v = nn.Conv2d(F, VC, 1, bias=False)
        self.v_bn = nn.BatchNorm2d(VC)
        self.fc1 = nn.Linear(VC * 81 + F, VH)
        self.fc_v = nn.Linear(VH, 1)
        self.fc_d = nn.Linear(VH, 1)

    def forward(self, x):
        x = Fn.silu(self.stem_bn(self.stem(x)))
        for b in self.blocks:
            x = b(x)
        policy = torch.flatten(self.p2(torch.relu(self.p1(x))), 1)
        v = torch.relu(self.v_bn(self.v(x)))
        h = torch.cat([torch.flatten(v, 1), x.mean(dim=(2, 3))], dim=1)
        h = torch.relu(self.fc1(h))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class GPoolNet(nn.Module):
    def __init__(self, C=93, F=24, VC=4, VH=16):
        super().__init__()
        self.stem = nn.Conv2d(C, F, 3, padding=1)
        self.stem_bn = nn.BatchNorm2d(F)
        self.c1 = nn.Conv2d(F, F, 3, padding=1, bias=False)
        self.b1 = nn.BatchNorm2d(F)
        self.gfc = nn.Linear(F, F)
        self.c2 = nn.Conv2d(F, F, 3, padding=1, bias=False)
        self.b2 = nn.BatchNorm2d(F)
        self.post = nn.BatchNorm2d(F)
        self.p = nn.Conv2d(F, 27, 1)
        self.v = nn.Conv2d(F, VC, 1)
        self.w1 = nn.Parameter(torch.randn(VC * 81, VH) / np.sqrt(VC * 81))
        self.bias1 = nn.Parameter(torch.randn(VH) * 0.1)
        self.wv = nn.Parameter(torch.randn(VH, 1) / np.sqrt(VH))
        self.bv = nn.Parameter(torch.randn(1) * 0.1)
        self.wd = nn.Parameter(torch.randn(VH, 1) / np.sqrt(VH))
        self.bd = nn.Parameter(torch.randn(1) * 0.1)

    def forward(self, x):
        x = torch.relu(self.stem_bn(self.stem(x)))
        y = torch.relu(self.b1(self.c1(x)))
        g = self.gfc(y.mean(dim=(2, 3), keepdim=True).view(x.size(0), -1))
        y = y + g.view(x.size(0), -1, 1, 1)
        y = self.b2(self.c2(y))
        x = torch.relu(self.post(x + y))
        policy = self.p(x).view(x.size(0), -1)
        v = torch.relu(self.v(x)).view(x.size(0), -1)
        h = torch.relu(torch.matmul(v, self.w1) + self.bias1)
        value = torch.sigmoid(torch.matmul(h, self.wv) + self.bv).squeeze(1)
        draw = torch.sigmoid(torch.matmul(h, self.wd) + self.bd).squeeze(1)
        return policy, value, draw


class SoftplusNet(nn.Module):
    def __init__(self, C=86, F=16, VH=16):
        super().__init__()
        self.stem = nn.Conv2d(C, F, 3, padding=1)
        self.c1 = nn.Conv2d(F, F, 3, padding=1)
        self.c2 = nn.Conv2d(F, F, 1)
        self.p = nn.Conv2d(F, 27, 1)
        self.fc1 = nn.Linear(F, VH)
        self.fc_v = nn.Linear(VH, 1)
        self.fc_d = nn.Linear(VH, 1)

    def forward(self, x):
        x = torch.tanh(self.stem(x))
        y = Fn.softplus(self.c1(x))
        x = torch.tanh(x + self.c2(y))
        policy = self.p(x)
        h = torch.tanh(self.fc1(Fn.adaptive_avg_pool2d(x, 1).flatten(1)))
        value = (torch.tanh(self.fc_v(h)) + 1.0) / 2.0
        return policy, value, torch.sigmoid(self.fc_d(h))


class ViewsNet(nn.Module):
    def __init__(self, C=86, F=16, VC=4, VH=16):
        super().__init__()
        self.stem = nn.Conv2d(C, F, 3, padding=1)
        self.c1 = nn.Conv2d(F, F, 3, padding=1)
        self.p = nn.Conv2d(F, 27, 1)
        self.v = nn.Conv2d(F, VC, 1)
        self.gfc = nn.Linear(F, VC)
        self.fc1 = nn.Linear(VC * 81, VH)
        self.fc_v = nn.Linear(VH, 1)
        self.fc_d = nn.Linear(VH, 1)

    def forward(self, x):
        x = torch.relu(self.stem(x))
        x = torch.relu(self.c1((x * 0.5).view(x.size(0), 16, 9, 9))) + x
        policy = torch.flatten(self.p(x) * 0.5, 1) * 2.0
        g = self.gfc(x.mean(dim=(2, 3))).view(x.size(0), -1, 1, 1)
        h = torch.relu(self.fc1(torch.flatten(torch.relu(self.v(x) + g), 1)))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


MODELS = (
    # name, module factory, planes, constant folding (BatchNorm folded by the exporter)
    ("net_graph_se", lambda: randomize_bn(SENet(), 11), 86, True),
    ("net_graph_gpool93", lambda: randomize_bn(GPoolNet(), 12, eps=1e-4), 93, False),
    ("net_graph_softplus", lambda: SoftplusNet(), 86, True),
    ("net_graph_views", lambda: ViewsNet(), 86, False),
)


def export_model(net, path, planes, fold):
    import make_onnx_golden
    make_onnx_golden.C = planes  # the exporter's dummy input shape
    return export(net, path, fold)


def positions():
    nsg = importlib.import_module("nshogi-engine_amd")
    old = np.load(os.path.join(HERE, "net_torch.npz"))["bitboards"]
    bb86 = np.concatenate([old, nsg.synth.random_batch(64 - len(old), 86, seed=20261016)])
    bb93 = nsg.synth.random_batch(64, 93, seed=20261017)
    return nsg, bb86, bb93


def main():
    nsg, bb86, bb93 = positions()
    out = {"bitboards86": bb86, "bitboards93": bb93}
    for seed, (name, make, planes, fold) in enumerate(MODELS):
        torch.manual_seed(100 + seed)
        net = make().eval()
        data = export_model(net, os.path.join(HERE, name + ".onnx"), planes, fold)
        bb = bb86 if planes == 86 else bb93
        x = nsg.synth.expand_reference(bb, True).reshape(-1, planes, 9, 9)
        with torch.no_grad():
            p, v, d = net.double()(torch.from_numpy(x).double())
        pol = p.numpy().reshape(len(bb), -1)
        for half in range(2):
            np.savez_compressed(os.path.join(HERE, f"{name}_policy_{half}.npz"), policy=pol[32 * half:32 * (half + 1)])
        out[name + "_value"] = v.numpy().reshape(-1)
        out[name + "_draw"] = d.numpy().reshape(-1)
        print(name, "onnx bytes", len(data), "positions", len(bb))
    np.savez_compressed(os.path.join(HERE, "net_graph.npz"), **out)


if __name__ == "__main__":
    main()
