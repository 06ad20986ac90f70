"""A plain float64 interpreter of ONNX models from the general graph path's op set: the reference of the buffer-history
and topology tests (tests/test_gpu_graph_history.py, tests/topology_models.py).

It reads the file with nsg.onnx_io.read_onnx and evaluates node after node with torch on the CPU in float64, from the
operators' definitions; it shares nothing with the planner or the kernels, knows no fusion and no layout.  Float
constants are the file's float32 values widened, float attributes likewise.  tests/test_plan_lifetimes.py holds it
against the float64 outputs stored beside the golden models, so it is itself checked.

run(nsg, model_bytes, planes, hook=None) -> {tensor name: numpy array}; `hook(node, inputs, output)` sees every node."""
import numpy as np
import torch
import torch.nn.functional as F


def _is_int(t):
    return not torch.is_floating_point(t)


def _ints(t):
    return [int(v) for v in np.asarray(t).reshape(-1)]


def _pool_pad(x, pads, value):
    return F.pad(x, (pads[1], pads[3], pads[0], pads[2]), value=value)


def _windows(x, kh, kw, dh, dw):
    """[taps, N, C, H, W] of a padded x, stride 1."""
    H, W = x.shape[2] - dh * (kh - 1), x.shape[3] - dw * (kw - 1)
    return torch.stack([x[:, :, ky * dh:ky * dh + H, kx * dw:kx * dw + W] for ky in range(kh) for kx in range(kw)])


def _node(nd, a, at):
    op = nd.op
    x = a[0] if a else None
    if op == "Conv":
        pads = at.get("pads", [0, 0, 0, 0])
        xp = F.pad(x, (pads[1], pads[3], pads[0], pads[2]))
        return F.conv2d(xp, a[1], a[2] if len(a) > 2 else None, dilation=tuple(at.get("dilations", [1, 1])), groups=int(at.get("group", 1)))
    if op == "Gemm":
        A = x.T if at.get("transA", 0) else x
        B = a[1].T if at.get("transB", 0) else a[1]
        y = float(at.get("alpha", 1.0)) * (A @ B)
        return y + float(at.get("beta", 1.0)) * a[2] if len(a) > 2 and a[2] is not None else y
    if op == "MatMul":
        return x @ a[1]
    if op == "BatchNormalization":
        shape = [1, -1] + [1] * (x.dim() - 2)
        eps = float(at.get("epsilon", np.float32(1e-5)))
        return (x - a[3].reshape(shape)) / torch.sqrt(a[4].reshape(shape) + eps) * a[1].reshape(shape) + a[2].reshape(shape)
    if op == "InstanceNormalization":
        shape = [1, -1] + [1] * (x.dim() - 2)
        dims = tuple(range(2, x.dim()))
        d = x - x.mean(dim=dims, keepdim=True)
        return d / torch.sqrt((d * d).mean(dim=dims, keepdim=True) + float(at.get("epsilon", np.float32(1e-5)))) * a[1].reshape(shape) + a[2].reshape(shape)
    if op == "LayerNormalization":
        dims = tuple(range(int(at.get("axis", -1)) % x.dim(), x.dim()))
        d = x - x.mean(dim=dims, keepdim=True)
        y = d / torch.sqrt((d * d).mean(dim=dims, keepdim=True) + float(at.get("epsilon", np.float32(1e-5)))) * a[1]
        return y + a[2] if len(a) > 2 and a[2] is not None else y
    if op in ("Add", "Sub", "Mul"):
        return {"Add": torch.add, "Sub": torch.sub, "Mul": torch.mul}[op](x, a[1])
    if op == "Div":
        return torch.div(x, a[1], rounding_mode="trunc") if _is_int(x) and _is_int(a[1]) else x / a[1]
    if op in ("Max", "Min"):
        return (torch.maximum if op == "Max" else torch.minimum)(x, a[1].expand_as(x) if a[1].dim() <= x.dim() else a[1])
    if op == "Pow":
        return torch.pow(x, a[1])
    unary = {"Relu": torch.relu, "Sigmoid": torch.sigmoid, "Tanh": torch.tanh, "Erf": torch.erf, "Exp": torch.exp, "Log": torch.log,
             "Sqrt": torch.sqrt, "Abs": torch.abs, "Neg": torch.neg, "Reciprocal": torch.reciprocal, "Identity": lambda t: t,
             "Softplus": lambda t: torch.where(t > 30.0, t, torch.log1p(torch.exp(torch.clamp(t, max=30.0)))),
             "HardSwish": lambda t: t * torch.clamp(t / 6.0 + 0.5, 0.0, 1.0),
             "Softsign": lambda t: t / (1.0 + torch.abs(t))}
    if op in unary:
        return unary[op](x)
    if op == "HardSigmoid":
        return torch.clamp(x * float(at.get("alpha", np.float32(0.2))) + float(at.get("beta", np.float32(0.5))), 0.0, 1.0)
    if op == "LeakyRelu":
        return torch.where(x > 0, x, x * float(at.get("alpha", np.float32(0.01))))
    if op == "PRelu":
        s = a[1].reshape(1, -1, 1, 1) if a[1].dim() == 1 and a[1].numel() > 1 and x.dim() == 4 else a[1]
        return torch.where(x > 0, x, x * s)
    if op == "Clip":
        y = x
        if len(a) > 1 and a[1] is not None:
            y = torch.maximum(y, a[1])
        if len(a) > 2 and a[2] is not None:
            y = torch.minimum(y, a[2])
        return y
    if op == "Softmax":
        return torch.softmax(x, dim=int(at.get("axis", -1)))
    if op in ("GlobalAveragePool", "GlobalMaxPool"):
        return x.mean(dim=(2, 3), keepdim=True) if op == "GlobalAveragePool" else x.amax(dim=(2, 3), keepdim=True)
    if op in ("ReduceMean", "ReduceMax", "ReduceSum"):
        axes = at.get("axes") if "axes" in at else (_ints(a[1]) if len(a) > 1 and a[1] is not None else list(range(x.dim())))
        keep = bool(at.get("keepdims", 1))
        fn = {"ReduceMean": torch.mean, "ReduceMax": torch.amax, "ReduceSum": torch.sum}[op]
        return fn(x, dim=tuple(int(v) for v in axes), keepdim=keep)
    if op in ("MaxPool", "AveragePool"):
        kh, kw = at["kernel_shape"]
        dh, dw = at.get("dilations", [1, 1])
        pads = at.get("pads", [0, 0, 0, 0])
        assert at.get("strides", [1, 1]) == [1, 1] and not at.get("ceil_mode", 0)
        if op == "MaxPool":
            return _windows(_pool_pad(x, pads, -np.inf), kh, kw, dh, dw).amax(dim=0)
        total = _windows(_pool_pad(x, pads, 0.0), kh, kw, dh, dw).sum(dim=0)
        if at.get("count_include_pad", 0):
            return total / (kh * kw)
        return total / _windows(_pool_pad(torch.ones_like(x), pads, 0.0), kh, kw, dh, dw).sum(dim=0)
    if op == "Flatten":
        ax = int(at.get("axis", 1))
        return x.reshape(int(np.prod(x.shape[:ax], dtype=np.int64)), -1)
    if op == "Reshape":
        to = _ints(a[1])
        to = [x.shape[k] if d == 0 and not at.get("allowzero", 0) else d for k, d in enumerate(to)]
        return x.reshape(to)
    if op == "Transpose":
        return x.permute(*at["perm"]) if "perm" in at else x.permute(*reversed(range(x.dim())))
    if op in ("Squeeze", "Unsqueeze"):
        axes = at.get("axes") if "axes" in at else (_ints(a[1]) if len(a) > 1 else None)
        if op == "Squeeze":
            if axes is None:
                return x.squeeze()
            for ax in sorted((v % x.dim() for v in axes), reverse=True):
                x = x.squeeze(ax)
            return x
        rank = x.dim() + len(axes)
        for ax in sorted(v % rank for v in axes):
            x = x.unsqueeze(ax)
        return x
    if op == "Concat":
        return torch.cat(a, dim=int(at["axis"]))
    if op == "Shape":
        return torch.tensor(list(x.shape), dtype=torch.int64)
    if op == "Cast":
        return x.to(torch.float64) if int(at["to"]) in (1, 10, 11) else x.to(torch.int64)
    if op == "Gather":
        ax = int(at.get("axis", 0)) % max(x.dim(), 1)
        idx = a[1].to(torch.int64)
        idx = torch.where(idx < 0, idx + x.shape[ax], idx)
        y = torch.index_select(x, ax, idx.reshape(-1))
        return y.reshape(list(x.shape[:ax]) + list(idx.shape) + list(x.shape[ax + 1:]))
    if op == "Slice":
        starts, ends = _ints(a[1]), _ints(a[2])
        axes = _ints(a[3]) if len(a) > 3 and a[3] is not None else list(range(len(starts)))
        steps = _ints(a[4]) if len(a) > 4 and a[4] is not None else [1] * len(starts)
        for s, e, ax, st in zip(starts, ends, axes, steps):
            idx = list(range(x.shape[ax]))[s:e:st]  # Python clamps and counts from the end as ONNX does
            x = torch.index_select(x, ax % x.dim(), torch.tensor(idx, dtype=torch.int64))
        return x
    raise NotImplementedError(f"{op} (node {nd.name})")


def run(nsg, data, planes, hook=None):
    """Every tensor of the model on planes [N, C, 9, 9], as float64 (or int64) numpy arrays by name."""
    nodes, inits, ins, outs = nsg.onnx_io.read_onnx(data)
    env = {k: torch.from_numpy(np.array(v, np.float64 if v.dtype.kind == "f" else np.int64)) for k, v in inits.items()}
    env["input"] = torch.from_numpy(np.array(planes, np.float64))
    with torch.no_grad():
        for nd in nodes:
            if nd.op == "Constant":
                continue
            a = [env[i] if i else None for i in nd.inputs]
            if nd.op == "Split":
                ax = int(nd.attrs.get("axis", 0))
                sizes = _ints(a[1]) if len(a) > 1 and a[1] is not None else nd.attrs.get("split") or [a[0].shape[ax] // len(nd.outputs)] * len(nd.outputs)
                for o, part in zip(nd.outputs, torch.split(a[0], [int(s) for s in sizes], dim=ax)):
                    env[o] = part
                continue
            y = _node(nd, a, nd.attrs)
            if hook is not None:
                hook(nd, a, y)
            env[nd.outputs[0]] = y
    return {k: v.numpy() for k, v in env.items()}


def outputs(nsg, data, planes, hook=None):
    """(policy [N,2187], value [N], draw [N]) in float64."""
    env = run(nsg, data, planes, hook)
    return [env["policy"].reshape(len(planes), -1), env["value"].reshape(-1), env["draw"].reshape(-1)]
