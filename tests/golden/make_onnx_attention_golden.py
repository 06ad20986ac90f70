"""Generates the attention fixtures of the general graph path (run from the repo root:
`python tests/golden/make_onnx_attention_golden.py`): net_att_pre.onnx, net_att_hybrid.onnx, net_att.npz and each
model's float64 policy in two files, net_att_<model>_policy_{0,1}.npz (positions 0-31 and 32-63, as for the other
general-graph fixtures: one file would exceed the repository's 1 MiB limit).

Both models treat the 81 squares as tokens [N,81,C] and are exported with the recipe of make_onnx_golden.py (legacy
TorchScript exporter, opset 17, dynamic batch axis).  The positions are the 86-plane positions of net_graph.npz.

  (a) net_att_pre     86 planes, 3x3 stem to F = 32 + ReLU, tokens, a learned positional embedding [1,81,32]; two
                      pre-LN blocks with H = 4 heads (d = 8), a fused QKV Linear that is `chunk`ed, the scale on the
                      scores, a relative bias [4,81,81] in block 1 and none in block 2, an exact-GELU FFN of width 64; a
                      final LayerNorm; policy = Linear(32,27) transposed back to [N,2187]; value and draw heads from
                      the token mean.
  (b) net_att_hybrid  F = 48, H = 3 (d = 16), separate q / k / v Linears with the scale applied to q before the
                      matmul and k permuted straight to [N,H,d,81]; one post-LN block (LayerNorm after the residual)
                      with a ReLU FFN; the tokens turned back into [N,48,9,9] and followed by one 3x3 residual conv
                      block; a 1x1 conv policy head and a value head over a flattened 1x1 conv.

LayerNorm gamma / beta and every bias are randomised.  Wq and Wk are scaled until the pre-softmax scores have a
standard deviation between 1 and 4 (asserted): near-uniform attention would hide a broken softmax.  The generator
also asserts that float32 PyTorch agrees with the float64 outputs it stores to better than 1e-5.

The module classes are importable: tests/test_gpu_onnx_attention.py exports small variants of them at test time.
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


class Attention(nn.Module):
    """Multi-head self-attention over the 81 squares.  fused: one QKV Linear, chunked; scale_on: 'scores', 'q' or
    'k'; k_perm: k goes to [N,H,d,81] in one permute (True) or by transpose(1,2) then transpose(-2,-1) (False).
    tweak: "size_scale" takes d from q.size(-1), which the exporter writes as Shape / Gather / Cast / Pow nodes;
    "softmax_axis1" and "relu_scores" are forms outside the supported pattern, for the refusal tests."""

    def __init__(self, F, H, bias=False, fused=True, scale_on="scores", k_perm=False, proj=True, tweak=None):
        super().__init__()
        self.tweak = tweak
        self.F, self.H, self.d = F, H, F // H
        self.fused, self.scale_on, self.k_perm = fused, scale_on, k_perm
        if fused:
            self.qkv = nn.Linear(F, 3 * F)
        else:
            self.q, self.k, self.v = nn.Linear(F, F), nn.Linear(F, F), nn.Linear(F, F)
        self.rel = nn.Parameter(torch.randn(H, 81, 81) * 0.5) if bias else None
        self.proj = nn.Linear(F, F) if proj else None
        self.uniform = False  # checks only: replace the softmax weights by 1/81
        self.scores = None    # checks only: the last pre-softmax scores

    def scale_qk(self, s):
        with torch.no_grad():
            if self.fused:
                self.qkv.weight[:2 * self.F] *= s
                self.qkv.bias[:2 * self.F] *= s
            else:
                for m in (self.q, self.k):
                    m.weight *= s
                    m.bias *= s

    def forward(self, x):
        N = x.size(0)
        if self.fused:
            q, k, v = self.qkv(x).chunk(3, dim=-1)
        else:
            q, k, v = self.q(x), self.k(x), self.v(x)
        scale = self.d ** -0.5
        if self.scale_on == "q":
            q = q * scale
        if self.scale_on == "k":
            k = k * scale
        q = q.view(N, 81, self.H, self.d).transpose(1, 2)
        v = v.view(N, 81, self.H, self.d).transpose(1, 2)
        k = k.view(N, 81, self.H, self.d)
        k = k.permute(0, 2, 3, 1) if self.k_perm else k.transpose(1, 2).transpose(-2, -1)
        a = q @ k
        if self.scale_on == "scores":
            a = a * (q.size(-1) ** -0.5 if self.tweak == "size_scale" else scale)
        if self.rel is not None:
            a = a + self.rel
        self.scores = a
        if self.tweak == "relu_scores":
            a = torch.relu(a)
        a = torch.softmax(a, dim=1 if self.tweak == "softmax_axis1" else -1)
        if self.uniform:
            a = torch.full_like(a, 1.0 / 81.0)
        o = (a @ v).transpose(1, 2).reshape(N, 81, self.F)
        return self.proj(o) if self.proj is not None else o


def tokens(x):
    return x.flatten(2).transpose(1, 2)


class PreBlock(nn.Module):
    def __init__(self, F, H, ffn, bias):
        super().__init__()
        self.ln1, self.ln2 = nn.LayerNorm(F), nn.LayerNorm(F)
        self.att = Attention(F, H, bias=bias, fused=True, scale_on="scores")
        self.fc1, self.fc2 = nn.Linear(F, ffn), nn.Linear(ffn, F)

    def forward(self, x):
        x = x + self.att(self.ln1(x))
        return x + self.fc2(Fn.gelu(self.fc1(self.ln2(x))))


class PreNet(nn.Module):
    def __init__(self, C=86, F=32, H=4, ffn=64, VH=32, blocks=2):
        super().__init__()
        self.stem = nn.Conv2d(C, F, 3, padding=1)
        self.pos = nn.Parameter(torch.randn(1, 81, F) * 0.3)
        self.blocks = nn.ModuleList([PreBlock(F, H, ffn, i == 0) for i in range(blocks)])  # a relative bias in block 1 only
        self.ln = nn.LayerNorm(F)
        self.p = nn.Linear(F, 27)
        self.fc1 = nn.Linear(F, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        N = x.size(0)
        x = tokens(torch.relu(self.stem(x))) + self.pos
        for b in self.blocks:
            x = b(x)
        x = self.ln(x)
        policy = self.p(x).transpose(1, 2).reshape(N, 2187)
        h = torch.relu(self.fc1(x.mean(dim=1)))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class PostBlock(nn.Module):
    def __init__(self, F, H, ffn):
        super().__init__()
        self.ln1, self.ln2 = nn.LayerNorm(F), nn.LayerNorm(F)
        self.att = Attention(F, H, bias=False, fused=False, scale_on="q", k_perm=True)
        self.fc1, self.fc2 = nn.Linear(F, ffn), nn.Linear(ffn, F)

    def forward(self, x):
        x = self.ln1(x + self.att(x))
        return self.ln2(x + self.fc2(torch.relu(self.fc1(x))))


class HybridNet(nn.Module):
    def __init__(self, C=86, F=48, H=3, ffn=96, VC=4, VH=32):
        super().__init__()
        self.F = F
        self.stem = nn.Conv2d(C, F, 3, padding=1)
        self.block = PostBlock(F, H, ffn)
        self.c1 = nn.Conv2d(F, F, 3, padding=1)
        self.c2 = nn.Conv2d(F, F, 3, padding=1)
        self.p = nn.Conv2d(F, 27, 1)
        self.v = nn.Conv2d(F, VC, 1)
        self.fc1 = nn.Linear(VC * 81, VH)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        N = x.size(0)
        x = self.block(tokens(torch.relu(self.stem(x))))
        x = x.transpose(1, 2).reshape(N, self.F, 9, 9)
        x = torch.relu(x + self.c2(torch.relu(self.c1(x))))
        policy = torch.flatten(self.p(x), 1)
        h = torch.relu(self.fc1(torch.flatten(torch.relu(self.v(x)), 1)))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class AttNet(nn.Module):
    """The smallest model around one attention module: stem, tokens, x + att(x), token heads.  flat_softmax: a Softmax
    on the flat value-head tensor (outside the pattern, for the refusal tests)."""

    def __init__(self, F, H, C=86, flat_softmax=False, **kw):
        super().__init__()
        self.flat_softmax = flat_softmax
        self.stem = nn.Conv2d(C, F, 3, padding=1)
        self.att = Attention(F, H, **kw)
        self.p = nn.Linear(F, 27)
        self.fc_v, self.fc_d = nn.Linear(F, 1), nn.Linear(F, 1)

    def forward(self, x):
        x = tokens(torch.tanh(self.stem(x)))
        x = x + self.att(x)
        policy = self.p(x).transpose(1, 2).reshape(x.size(0), 2187)
        h = x.mean(dim=1)
        if self.flat_softmax:
            h = torch.softmax(h, dim=-1)
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class LNNet(nn.Module):
    """LayerNorm alone: stem, tokens, LayerNorm over C = 24 channels (the row stride is 32: pad channels in play),
    token heads; the value head runs a LayerNorm over a flat [N,VH] tensor."""

    def __init__(self, F=24, C=86, VH=20, eps=1e-3):
        super().__init__()
        self.stem = nn.Conv2d(C, F, 3, padding=1)
        self.ln = nn.LayerNorm(F, eps=eps)
        self.p = nn.Linear(F, 27)
        self.fc1 = nn.Linear(F, VH)
        self.ln_flat = nn.LayerNorm(VH, eps=eps)
        self.fc_v, self.fc_d = nn.Linear(VH, 1), nn.Linear(VH, 1)

    def forward(self, x):
        x = self.ln(tokens(torch.tanh(self.stem(x))))
        policy = self.p(x).transpose(1, 2).reshape(x.size(0), 2187)
        h = torch.relu(self.ln_flat(self.fc1(x.mean(dim=1))))
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


def randomize(net, seed):
    """LayerNorm gamma / beta and every bias away from their defaults."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.LayerNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.2)
            elif isinstance(m, (nn.Linear, nn.Conv2d)) and m.bias is not None:
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
    return net


def sharpen(net, x, target=2.0):
    """Scales Wq and Wk of every attention module, in order, until its pre-softmax scores have a standard deviation
    near `target`; returns the final standard deviations."""
    atts = [m for m in net.modules() if isinstance(m, Attention)]
    for a in atts:
        for _ in range(4):
            with torch.no_grad():
                net(x)
            sd = float(a.scores.std())
            a.scale_qk(float(np.sqrt(min(max(target / max(sd, 1e-6), 0.25), 16.0))))
    with torch.no_grad():
        net(x)
    sds = [float(a.scores.std()) for a in atts]
    for a in atts:
        a.scores = None
    return sds


def export_model(net, path, planes=86, fold=True):
    make_onnx_golden.C = planes  # the exporter's dummy input shape
    return make_onnx_golden.export(net, path, fold)


MODELS = (("net_att_pre", PreNet, 31), ("net_att_hybrid", HybridNet, 32))


def main():
    nsg = importlib.import_module("nshogi-engine_amd")
    bb = np.load(os.path.join(HERE, "net_graph.npz"))["bitboards86"]
    x32 = torch.from_numpy(nsg.synth.expand_reference(bb, True).reshape(-1, 86, 9, 9).astype(np.float32))
    out = {}
    for name, make, seed in MODELS:
        torch.manual_seed(200 + seed)
        net = randomize(make(), seed).eval()
        sds = sharpen(net, x32)
        assert all(1.0 < s < 4.0 for s in sds), (name, sds)
        data = export_model(net, os.path.join(HERE, name + ".onnx"))
        with torch.no_grad():
            o32 = [t.numpy().astype(np.float64) for t in net(x32)]
            o64 = [t.numpy() for t in net.double()(x32.double())]
        err = max(float(np.abs(a.reshape(-1) - b.reshape(-1)).max()) for a, b in zip(o32, o64))
        assert err < 1e-5, (name, err)
        pol = o64[0].reshape(len(bb), -1)
        for half in range(2):
            np.savez_compressed(os.path.join(HERE, f"{name}_policy_{half}.npz"), policy=pol[32 * half:32 * (half + 1)])
        out[name + "_value"] = o64[1].reshape(-1)
        out[name + "_draw"] = o64[2].reshape(-1)
        print(name, "onnx bytes", len(data), "score std", [round(s, 2) for s in sds], "float32 vs float64", f"{err:.2e}",
              "policy range", float(pol.min()), float(pol.max()))
    np.savez_compressed(os.path.join(HERE, "net_att.npz"), **out)


if __name__ == "__main__":
    main()
