"""Hand-built ONNX models around the general graph path's fused elementwise launch, and a plain numpy interpreter of the
same node lists: the reference of tests/test_onnx_elementwise.py and tests/test_gpu_onnx_elementwise.py.

A `Net` records its nodes as Python tuples and serialises them with nsg.onnx_io's helpers.  `Net.run` evaluates the
recorded nodes in float64, op by op, with numpy indexing of its own: with `rounded` every result is rounded to float32
once, which is what the kernel's registers do (+ - * / of two f32 values computed in f64 and rounded once are the
correctly rounded f32 results; max, min, abs, neg and a select are exact)."""
import math

import numpy as np

F = 27  # 27 channels: policy = Flatten(result) is the [N, 2187] policy, and rows of stride 32 have 5 pad channels


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _erf(a):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, np.float64))).numpy()


def _relu6(a):
    return np.minimum(np.maximum(a, 0.0), 6.0)


def _softplus(a):
    with np.errstate(over="ignore"):
        return np.where(a > 20.0, a, np.log1p(np.exp(np.minimum(a, 30.0))))  # torch's threshold


def _sigmoid(a):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-a))


# float64 definitions (torch's) of the activations the kernels know as one Act code
ACT64 = {
    "relu": lambda a: np.maximum(a, 0.0),
    "sigmoid": _sigmoid,
    "tanh": np.tanh,
    "swish": lambda a: a * _sigmoid(a),
    "softplus": _softplus,
    "erf": _erf,
    "gelu": lambda a: 0.5 * a * (1.0 + _erf(a / math.sqrt(2.0))),
    "relu6": _relu6,
    "hardswish": lambda a: a * _relu6(a + 3.0) / 6.0,
    "hardsigmoid": lambda a: _relu6(a + 3.0) / 6.0,
}


ACT_OPS = {"Relu": "relu", "Sigmoid": "sigmoid", "Tanh": "tanh", "Softplus": "softplus", "Erf": "erf", "HardSwish": "hardswish"}


class Net:
    def __init__(self, nsg, planes=86):
        self.io, self.planes = nsg.onnx_io, planes
        self.nodes, self.consts = [], {}

    def const(self, name, arr, dtype=np.float32):
        assert name not in self.consts, name
        self.consts[name] = np.asarray(arr, dtype)
        return name

    def node(self, op, ins, outs, name=None, **attrs):
        outs = [outs] if isinstance(outs, str) else list(outs)
        self.nodes.append((op, list(ins), outs, attrs, name or outs[0]))
        return outs[0] if len(outs) == 1 else outs

    # ---- the pieces every model shares -------------------------------------------------------------------------
    def stem(self, width=F, seed=0, exp=-3, span=1, out="s"):
        """A 3x3 conv of the planes with weights from {-span..span} * 2^exp (most of them zero) and a bias of the same
        grid; zero on the last four planes, which hold fractions.  Every partial sum is a small multiple of 2^exp, so
        the conv's float32 result is exact in any order of summation."""
        rng = np.random.default_rng(seed)
        w = rng.integers(-span, span + 1, size=(width, self.planes, 3, 3)) * (rng.random((width, self.planes, 3, 3)) < 0.2)
        w[:, self.planes - 4:] = 0
        b = rng.integers(-8, 9, size=width)
        self.const(out + "_w", w * 2.0 ** exp)
        self.const(out + "_b", b * 2.0 ** exp)
        return self.node("Conv", ["input", out + "_w", out + "_b"], out, kernel_shape=[3, 3], pads=[1, 1, 1, 1])

    def split_stem(self, seed=0, exp=-3):
        """The 54-channel stem split at channel 27: the second half is a view at an offset that 4 does not divide."""
        self.stem(2 * F, seed, exp)
        self.const("halves", [F, F], np.int64)
        return self.node("Split", ["s", "halves"], ["a", "b"], name="split", axis=1)

    def heads(self, x, seed=1):
        rng = np.random.default_rng(seed)
        self.node("GlobalAveragePool", [x], "gp", name="gap")
        self.node("Flatten", ["gp"], "gpf", name="gflat", axis=1)
        for out in ("value", "draw"):
            self.const(out + "_w", rng.normal(size=(1, F)) * 0.2)
            self.const(out + "_b", [0.1])
            self.node("Gemm", ["gpf", out + "_w", out + "_b"], out + "_z", name=out + "_fc", transB=1)
            self.node("Sigmoid", [out + "_z"], out, name=out + "_sig")

    def finish(self, result, heads_from, flatten=True):
        """policy = Flatten(result), value and draw from the mean of `heads_from`; returns the model's bytes."""
        if flatten:
            self.node("Flatten", [result], "policy", name="pflat", axis=1)
        self.heads(heads_from)
        return self.data()

    def data(self):
        io = self.io
        nodes = []
        for op, ins, outs, attrs, name in self.nodes:
            at = []
            for k, v in attrs.items():
                at.append(io._attr_ints(k, v) if isinstance(v, (list, tuple)) else io._attr_f(k, v) if isinstance(v, float) else io._attr_i(k, v))
            nodes.append(io._node(op, ins, outs, at, name=name))
        graph = b"".join(io._f_bytes(1, n) for n in nodes) + io._f_bytes(2, "elementwise")
        graph += b"".join(io._f_bytes(5, io._tensor(k, v)) for k, v in self.consts.items())
        graph += io._f_bytes(11, io._value_info("input", ["N", self.planes, 9, 9]))
        for name, dims in (("policy", ["N", 2187]), ("value", ["N", 1]), ("draw", ["N", 1])):
            graph += io._f_bytes(12, io._value_info(name, dims))
        return io._f_varint(1, 7) + io._f_bytes(7, graph) + io._f_bytes(8, io._f_bytes(1, "") + io._f_varint(2, 17))

    # ---- the reference -----------------------------------------------------------------------------------------
    def run(self, x, rounded=True):
        """Evaluates the nodes on planes x [N, planes, 9, 9] (float64).  Returns every tensor by name."""
        r = f32 if rounded else (lambda a: np.asarray(a, np.float64))
        env = {k: v.astype(np.float64) if v.dtype == np.float32 else v for k, v in self.consts.items()}
        env["input"] = np.asarray(x, np.float64)
        for op, ins, outs, at, _ in self.nodes:
            a = [env[i] if i else None for i in ins]
            if op == "Conv":
                k = at["kernel_shape"][0]
                h = k // 2
                xp = np.pad(a[0], ((0, 0), (0, 0), (h, h), (h, h)))
                y = np.zeros((a[0].shape[0], a[1].shape[0], 9, 9))
                for dy in range(k):
                    for dx in range(k):
                        y += np.einsum("oc,ncyx->noyx", a[1][:, :, dy, dx], xp[:, :, dy:dy + 9, dx:dx + 9])
                y = y + a[2].reshape(1, -1, 1, 1) if len(a) > 2 else y
            elif op == "Split":
                cut = np.cumsum(a[1])[:-1]
                for o, part in zip(outs, np.split(a[0], cut, axis=at["axis"])):
                    env[o] = part
                continue
            elif op == "MaxPool":
                kh, kw = at["kernel_shape"]
                xp = np.pad(a[0], ((0, 0), (0, 0), (kh // 2, kh // 2), (kw // 2, kw // 2)), constant_values=-np.inf)
                y = np.max([xp[:, :, dy:dy + 9, dx:dx + 9] for dy in range(kh) for dx in range(kw)], axis=0)
            elif op in ("Add", "Sub", "Mul", "Div"):
                y = {"Add": np.add, "Sub": np.subtract, "Mul": np.multiply, "Div": np.divide}[op](a[0], a[1])
            elif op in ("Max", "Min"):
                y = (np.maximum if op == "Max" else np.minimum)(a[0], a[1])
            elif op == "Neg":
                y = -a[0]
            elif op == "Abs":
                y = np.abs(a[0])
            elif op == "Clip":
                y = a[0]
                if len(a) > 1 and a[1] is not None:
                    y = np.maximum(y, a[1])
                if len(a) > 2 and a[2] is not None:
                    y = np.minimum(y, a[2])
            elif op == "LeakyRelu":
                y = np.where(a[0] > 0, a[0], r(a[0] * f32(at.get("alpha", 0.01))))
            elif op == "PRelu":
                slope = a[1].reshape(1, -1, 1, 1) if a[1].ndim == 1 and a[1].size > 1 else a[1]
                y = np.where(a[0] > 0, a[0], r(a[0] * slope))
            elif op in ACT_OPS or (op == "HardSigmoid" and abs(at.get("alpha", 0.2) - 1.0 / 6.0) < 1e-6):
                env[outs[0]] = ACT64[ACT_OPS.get(op, "hardsigmoid")](a[0])  # one Act code: float64, not rounded
                continue
            elif op == "HardSigmoid":  # at another alpha than 1/6: four instructions
                y = r(a[0] * f32(at.get("alpha", 0.2)))
                y = np.minimum(np.maximum(r(y + f32(at.get("beta", 0.5))), 0.0), 1.0)
            elif op == "BatchNormalization":  # x * s + t with s and t computed in double and rounded once, as the planner does
                s = a[1] / np.sqrt(a[4] + np.float64(np.float32(at.get("epsilon", 1e-5))))
                t = a[2] - a[3] * s
                shape = (1, -1, 1, 1)
                y = r(r(a[0] * r(s).reshape(shape)) + r(t).reshape(shape))
            elif op == "GlobalAveragePool":
                y = r(r(a[0].sum(axis=(2, 3), keepdims=True)) / 81.0)
            elif op == "Flatten":
                y = a[0].reshape(a[0].shape[0], -1)
            elif op == "Reshape":
                y = a[0].reshape([a[0].shape[0] if d == -1 else d for d in a[1]])
            elif op == "Unsqueeze":
                y = a[0]
                for ax in sorted(a[1]):
                    y = np.expand_dims(y, int(ax))
            elif op == "Transpose":
                y = np.transpose(a[0], at["perm"])
            elif op == "Gemm":
                y = a[0] @ a[1].T + (a[2] if len(a) > 2 else 0.0)
            else:
                raise NotImplementedError(op)
            env[outs[0]] = r(y)
        return env


# ---- the three families of chains that reach the launch's limits ------------------------------------------------------
def scalar_mul_chain(net, x, k):
    """x * c0 * c1 * ... : one source and two registers per node."""
    for i in range(k):
        x = net.node("Mul", [x, net.const(f"c{i}", [1.0 + (i % 5 - 2) * 0.125])], f"m{i}", name=f"mul{i}")
    return x


WINDOWS = [(kh, kw) for kh in (3, 1, 5, 7) for kw in (3, 1, 5, 7) if (kh, kw) != (1, 1)]  # 15 distinct windows


def pooled_sum(net, x, n):
    """((p0 + p1) + p2) + ... of n distinct non-conv tensors, each a MaxPool of x over another window (one launch
    each): one source per term."""
    ps = []
    for i, (kh, kw) in enumerate(WINDOWS[:n]):
        ps.append(net.node("MaxPool", [x], f"p{i}", name=f"pool{i}", kernel_shape=[kh, kw], pads=[kh // 2, kw // 2] * 2, strides=[1, 1]))
    y = ps[0]
    for i in range(1, n):
        y = net.node("Add", [y, ps[i]], f"sum{i}", name=f"add{i}")
    return y


def unary_then_binary(net, x, u):
    """u alternating Abs / Neg (one register each), then one Mul by a scalar."""
    for i in range(u):
        x = net.node("Abs" if i % 2 == 0 else "Neg", [x], f"u{i}", name=f"un{i}")
    return net.node("Mul", [x, net.const("cu", [0.75])], "ub", name="umul")


FAMILIES = {"scalar_mul": scalar_mul_chain, "pooled_sum": pooled_sum, "unary_binary": unary_then_binary}


def family_model(nsg, family, length, seed=0):
    """An exact stem that also feeds the heads (so nothing joins its epilogue), the chain, policy = Flatten(chain)."""
    net = Net(nsg)
    s = net.stem(seed=seed)
    y = FAMILIES[family](net, s, length)
    return net, net.finish(y, s)
