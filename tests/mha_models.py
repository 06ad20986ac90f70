"""Small nets around PyTorch's stock transformer modules, and for each a hand-written twin with the same weights: the
shared half of tests/test_onnx_mha.py (host) and tests/test_gpu_onnx_mha.py (device).

Every net is built like make_onnx_attention_golden.AttNet: 86 planes, a 3x3 stem with tanh, tokens(), the module, a
token policy Linear(E,27) transposed to 2187, the mean over the squares, sigmoid value and draw heads.

  MhaNet      x + nn.MultiheadAttention(E, H)(x, x, x)[0]: batch_first or behind the caller's own transpose(0, 1), with or
              without biases, need_weights False (the module goes through scaled-dot-product attention on [N,H,81,d]) or
              True with the weights dropped (the exporter writes the 3-D form on [N*H,81,d])
  EncNet      nn.TransformerEncoder of nn.TransformerEncoderLayer(E, H, ffn, dropout=0, batch_first=True): pre- or
              post-norm, relu or gelu, one layer or more, an optional final norm

twin(net) is the same function written out by hand around make_onnx_attention_golden.Attention (fused QKV,
scale_on="q", proj=True): in_proj_weight / in_proj_bias go into `qkv`, out_proj into `proj`, the layer norms and the FFN
into a block of the encoder layer's own order.  A module without biases gets zero biases in its twin: the launches are
the same, the bias vector of a launch is always there.

Everything is exported at test time in .eval() with the exporter recipe shared by the other generators."""
import os
import sys

import torch
import torch.nn as nn
import torch.nn.functional as Fn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import make_onnx_attention_golden as gen  # noqa: E402

tokens = gen.tokens


class Mha(nn.Module):
    """Self-attention over the squares through nn.MultiheadAttention.  call: further keyword arguments of the module's
    forward (masks), for the refusal tests; other: "kv" takes key and value from a second tensor."""

    def __init__(self, E, H, bias=True, batch_first=True, need_weights=False, use_weights=False, call=None, **kw):
        super().__init__()
        self.batch_first, self.need_weights, self.use_weights = batch_first, need_weights, use_weights
        self.call = call or {}
        self.m = nn.MultiheadAttention(E, H, bias=bias, batch_first=batch_first, **kw)

    def forward(self, x, kv=None):
        if not self.batch_first:
            x, kv = x.transpose(0, 1), None if kv is None else kv.transpose(0, 1)
        kv = x if kv is None else kv  # (self-attention hands the module one tensor three times: it packs the projection)
        y, w = self.m(x, kv, kv, need_weights=self.need_weights, **self.call)
        if self.use_weights:  # [N,81,81] averaged over the heads, applied once more
            y = y + (w @ y if self.batch_first else (w @ y.transpose(0, 1)).transpose(0, 1))
        return y if self.batch_first else y.transpose(0, 1)


class Heads(nn.Module):
    def __init__(self, E):
        super().__init__()
        self.p = nn.Linear(E, 27)
        self.fc_v, self.fc_d = nn.Linear(E, 1), nn.Linear(E, 1)

    def forward(self, x):
        policy = self.p(x).transpose(1, 2).reshape(x.size(0), 2187)
        h = x.mean(dim=1)
        return policy, torch.sigmoid(self.fc_v(h)), torch.sigmoid(self.fc_d(h))


class MhaNet(nn.Module):
    """cross: key and value come from a second stem (cross-attention); squares: attend over the first `squares` tokens
    only (a sequence that is not the 81 squares), the rest pass through."""

    def __init__(self, E, H, C=86, cross=False, squares=81, **kw):
        super().__init__()
        self.E, self.H, self.squares = E, H, squares
        self.stem = nn.Conv2d(C, E, 3, padding=1)
        self.stem2 = nn.Conv2d(C, kw.get("kdim", E), 3, padding=1) if cross else None  # (kdim = vdim where given)
        self.att = Mha(E, H, **kw)
        self.heads = Heads(E)

    def forward(self, x0):
        x = tokens(torch.tanh(self.stem(x0)))
        if self.squares != 81:
            a = self.att(x[:, :self.squares])
            return self.heads(torch.cat([x[:, :self.squares] + a, x[:, self.squares:]], dim=1))
        kv = tokens(torch.tanh(self.stem2(x0))) if self.stem2 is not None else None
        return self.heads(x + self.att(x, kv))


class EncNet(nn.Module):
    def __init__(self, E, H, ffn, C=86, layers=1, norm_first=True, activation="relu", final_norm=False):
        super().__init__()
        self.E, self.H = E, H
        self.stem = nn.Conv2d(C, E, 3, padding=1)
        layer = nn.TransformerEncoderLayer(E, H, ffn, dropout=0.0, activation=activation, batch_first=True, norm_first=norm_first)
        self.enc = nn.TransformerEncoder(layer, layers, norm=nn.LayerNorm(E) if final_norm else None, enable_nested_tensor=False)
        self.heads = Heads(E)

    def forward(self, x):
        return self.heads(self.enc(tokens(torch.tanh(self.stem(x)))))


# ---- the hand-written twins ---------------------------------------------------------------------------------------------
def twin_attention(m):
    """make_onnx_attention_golden.Attention with the weights of the nn.MultiheadAttention m."""
    E, H = m.embed_dim, m.num_heads
    a = gen.Attention(E, H, bias=False, fused=True, scale_on="q", proj=True)
    with torch.no_grad():
        a.qkv.weight.copy_(m.in_proj_weight)
        a.qkv.bias.copy_(m.in_proj_bias if m.in_proj_bias is not None else torch.zeros(3 * E))
        a.proj.weight.copy_(m.out_proj.weight)
        a.proj.bias.copy_(m.out_proj.bias if m.out_proj.bias is not None else torch.zeros(E))
    return a


class TwinMhaNet(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.stem, self.heads = net.stem, net.heads
        self.att = twin_attention(net.att.m)

    def forward(self, x):
        x = tokens(torch.tanh(self.stem(x)))
        return self.heads(x + self.att(x))


class TwinLayer(nn.Module):
    """An encoder layer in its own order around the hand-written attention (PreBlock / PostBlock of the generator)."""

    def __init__(self, layer):
        super().__init__()
        self.norm_first = layer.norm_first
        self.gelu = layer.activation is Fn.gelu
        assert self.gelu or layer.activation is Fn.relu
        self.att = twin_attention(layer.self_attn)
        self.ln1, self.ln2, self.fc1, self.fc2 = layer.norm1, layer.norm2, layer.linear1, layer.linear2

    def ffn(self, x):
        h = self.fc1(x)
        return self.fc2(Fn.gelu(h) if self.gelu else torch.relu(h))

    def forward(self, x):
        if self.norm_first:
            x = x + self.att(self.ln1(x))
            return x + self.ffn(self.ln2(x))
        x = self.ln1(x + self.att(x))
        return self.ln2(x + self.ffn(x))


class TwinEncNet(nn.Module):
    def __init__(self, net):
        super().__init__()
        self.stem, self.heads, self.norm = net.stem, net.heads, net.enc.norm
        self.layers = nn.ModuleList([TwinLayer(l) for l in net.enc.layers])

    def forward(self, x):
        x = tokens(torch.tanh(self.stem(x)))
        for l in self.layers:
            x = l(x)
        return self.heads(x if self.norm is None else self.norm(x))


def twin(net):
    return (TwinMhaNet if isinstance(net, MhaNet) else TwinEncNet)(net).eval()


def make(kind, E, H, seed=0, **kw):
    """A seeded net of `kind` ("mha" or "enc") with every bias and LayerNorm away from its default, in eval mode."""
    torch.manual_seed(1000 + seed)
    net = MhaNet(E, H, **kw) if kind == "mha" else EncNet(E, H, **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.MultiheadAttention):
                # (torch starts in_proj_bias and out_proj.bias at zero)
                for b in (m.in_proj_bias, m.out_proj.bias):
                    if b is not None:
                        b.copy_(torch.randn(b.shape, generator=g) * 0.1)
                if m.in_proj_weight is not None:
                    m.in_proj_weight[:2 * E] *= 3.0  # q and k: scores of a spread that a uniform softmax would not give
    return gen.randomize(net, seed).eval()


def export(net, path):
    return gen.export_model(net.eval(), str(path))
