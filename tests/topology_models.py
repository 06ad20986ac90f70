"""Small hand-built graphs whose shape, not whose arithmetic, is the test: tensors that stay alive across many unrelated
launches, read late through every view field a launch has (rules R1-R5).  The shared half of
tests/test_plan_lifetimes.py (host) and tests/test_gpu_graph_history.py (device).

Every model starts from elt_models.Net's exact integer stem on the 0/1 planes (exp = 0: integers) with its weights and
bias made positive, so that the Relu fused into the stem's launch passes the whole output.  Its 1x1 convs and dense
layers have weights in {-1, 0, 1} and small integer biases and a Relu behind them, the only activation: nothing
saturates, so a board of large planes (the poison of the history test) leaves large values in every buffer.  The chains
of unrelated launches between a tensor's writer and its late reader hold, besides the convs, a 3x3 max pooling, a Gather
of the channels (kLaunchGather) and a two-stage token-mixing MLP with 20 hidden units, 12 pad units behind them
(kLaunchTokenMix), all with integer constants.  Every tensor of the real boards is therefore an integer and the float64
reference (tests/onnx_ref64.py) is exact in float32 in any order of summation: `reference` asserts that every tensor of
an exact case is integer-valued and that sum |w x| of every Conv, Gemm and MatMul stays below 2^24.  The device must
give those values bit for bit.  Value and draw are integers too (a dense layer on the global max), so all three outputs
are exact.  No tensor is wider than 64 channels.

  long_skip       s -> six 1x1 convs of widths 16, 40, 24, 64, 16, 40; the last adds s (the field `res`)
  fan_out         four branches from s of widths 16, 24, 40, 64, two launches each, joined by Concat (`seg`) and read
                  through a Split view at channel 20; the heads come last, so the policy waits for them (`policy`)
  early_heads     value and draw are finished by launches 2 and 3, fourteen more launches of every width follow
  token_and_flat  one token tensor read by a token dense layer and, launches later, through Flatten -> Gemm
  kv, rtbias, bmm, srcs, lines18   the second operand of a kernel is produced right after the stem and read at least
                  three unrelated launches later: attention's K and V, its run-time bias, a run-time MatMul's second
                  operand, an elementwise launch's spatial, flat (kSrcBoard) and line sources, an 18-line block

Attention cannot be exact: `kv` and `rtbias` are held to 1e-4 (their convs carry a gain of 1/4, which keeps the
operands of the real boards of order 1 to 100), and `swaps` gives, for each early operand, the models
in which the reader takes another tensor that is live at that point instead; the float64 policy must move by more than
1e-2, so a wrong buffer cannot hide inside the tolerance."""
import numpy as np

import onnx_ref64
import reduction_models as rm

WIDTHS = (16, 40, 24, 64)


class TNet(rm.RNet):
    def __init__(self, nsg, width, seed=0, gain=1.0):
        """gain: a power of two on the weights of every conv and token-mixing stage (the attention cases keep their
        operands of order 1 with it; the exact cases leave it at 1)."""
        super().__init__(nsg)
        self.rng = np.random.default_rng(1000 + seed)
        self.gain = gain
        self.stem(width, seed, exp=0)
        # every stem weight and bias at or above zero: the stem output is positive on every board, so the Relu that rides
        # in the stem's launch passes it whole and a board of large planes gives a large value in every channel
        self.consts["s_w"], self.consts["s_b"] = np.abs(self.consts["s_w"]), np.abs(self.consts["s_b"]) + np.float32(1.0)
        self.act("s", "sr")
        self.width = width

    def act(self, x, out):
        return self.node("Relu", [x], out, name=out)

    def weights(self, cout, cin):
        """{-1, 0, 1}, about six taps per output and at least one; biases 0..3."""
        w = self.rng.integers(-1, 2, size=(cout, cin)) * (self.rng.random((cout, cin)) < min(1.0, 6.0 / cin))
        w[np.arange(cout), self.rng.integers(0, cin, size=cout)] = 1
        return w.astype(np.float64), self.rng.integers(0, 4, size=cout).astype(np.float64)

    def conv(self, x, cin, cout, out, res=None):
        w, b = self.weights(cout, cin)
        w = w * self.gain
        y = self.node("Conv", [x, self.const(out + "_w", w.reshape(cout, cin, 1, 1)), self.const(out + "_b", b)], out + "_c", name=out + "_conv",
                      kernel_shape=[1, 1], pads=[0, 0, 0, 0])
        if res is not None:
            y = self.node("Add", [y, res], out + "_r", name=out + "_add")
        return self.act(y, out)

    def gather(self, x, cin, out):
        """The channels of x in reverse order: one kLaunchGather."""
        return self.node("Gather", [x, self.const(out + "_idx", np.arange(cin)[::-1].copy(), np.int64)], out, name=out, axis=1)

    def token_mix(self, x, cin, out, hidden=20):
        """A two-stage Linear over the 81 squares of every channel, 20 hidden units (12 pad units behind them) and a
        Relu between the stages: one kLaunchTokenMix.  Two taps per hidden unit and per square keep the sums small."""
        def taps(k, d):
            w = np.zeros((k, d))
            for j in range(d):
                w[self.rng.choice(k, 2, replace=False), j] = (1.0, -1.0) if j % 3 == 0 else (1.0, 1.0)
            return w * min(1.0, 2.0 * self.gain)
        y = self.node("Reshape", [x, self.const(out + "_to3", [-1, cin, 81], np.int64)], out + "_c3", name=out + "_c3")
        y = self.node("MatMul", [y, self.const(out + "_w1", taps(81, hidden))], out + "_mm1", name=out + "_mm1")
        y = self.node("Add", [y, self.const(out + "_b1", self.rng.integers(0, 3, size=hidden).astype(np.float64))], out + "_h", name=out + "_bias1")
        y = self.node("Relu", [y], out + "_hr", name=out + "_relu")
        y = self.node("MatMul", [y, self.const(out + "_w2", taps(hidden, 81))], out + "_mm2", name=out + "_mm2")
        y = self.node("Add", [y, self.const(out + "_b2", self.rng.integers(0, 3, size=81).astype(np.float64))], out + "_o", name=out + "_bias2")
        return self.node("Reshape", [y, self.const(out + "_to4", [-1, cin, 9, 9], np.int64)], out, name=out)

    def chain(self, x, cin, widths, tag):
        """Unrelated launches: 1x1 convs, with a 3x3 max pooling behind the first, a Gather of the channels behind the
        second and a token-mixing MLP behind the third (chains of three or more)."""
        for i, w in enumerate(widths):
            x = self.conv(x, cin, w, f"{tag}{i}")
            if len(widths) > 2:
                if i == 0:
                    x = self.node("MaxPool", [x], f"{tag}{i}_mp", name=f"{tag}{i}_pool", kernel_shape=[3, 3], pads=[1, 1, 1, 1], strides=[1, 1])
                if i == 1:
                    x = self.gather(x, w, f"{tag}{i}_g")
                if i == 2:
                    x = self.token_mix(x, w, f"{tag}{i}_mix")
            cin = w
        return x

    def dense(self, x, cin, cout, out):
        w, b = self.weights(cout, cin)
        return self.node("Gemm", [x, self.const(out + "_w", w), self.const(out + "_b", b)], out, name=out + "_fc", transB=1)

    def int_heads(self, x, width):
        """value and draw: dense layers on the global max of x, integers."""
        self.node("GlobalMaxPool", [x], "gm4", name="gmax")
        g = self.node("Flatten", ["gm4"], "gm", name="gmflat", axis=1)
        self.dense(g, width, 1, "value")
        self.dense(g, width, 1, "draw")
        return g

    def token_dense(self, tok, cin, cout, out):
        w, b = self.weights(cout, cin)
        self.node("MatMul", [tok, self.const(out + "_w", w.T.copy())], out + "_mm", name=out + "_mm")
        return self.node("Add", [out + "_mm", self.const(out + "_b", b)], out, name=out + "_bias")

    def policy_of_tokens(self, tok27):
        """[N,81,27] -> [N,2187] in the policy's order (channel major)."""
        self.node("Transpose", [tok27], "pt", perm=[0, 2, 1])
        return self.node("Reshape", ["pt", self.const("to2", [-1, 2187], np.int64)], "policy", name="pflat")

    def policy_conv(self, x, cin):
        p = self.conv(x, cin, 27, "pol")
        return self.node("Flatten", [p], "policy", name="pflat", axis=1)

    def attention(self, q, k, v, F, out, bias=None):
        """One head of F channels over token tensors q, k, v; the scores are 2^-3 q.k (+ bias [N,1,81,81])."""
        self.const(out + "_to4", [-1, 81, 1, F], np.int64)
        q4, k4, v4 = (self.node("Reshape", [t, out + "_to4"], f"{out}_{nm}4") for nm, t in zip("qkv", (q, k, v)))
        qh = self.node("Transpose", [q4], out + "_qh", perm=[0, 2, 1, 3])
        kt = self.node("Transpose", [k4], out + "_kt", perm=[0, 2, 3, 1])
        vh = self.node("Transpose", [v4], out + "_vh", perm=[0, 2, 1, 3])
        a = self.node("MatMul", [qh, kt], out + "_qk")
        a = self.node("Mul", [a, self.const(out + "_scale", [0.125])], out + "_scaled")
        if bias is not None:
            a = self.node("Add", [a, bias], out + "_biased")
        p = self.node("Softmax", [a], out + "_probs", axis=-1)
        o = self.node("MatMul", [p, vh], out + "_oh")
        o = self.node("Transpose", [o], out + "_ot", perm=[0, 2, 1, 3])
        return self.node("Reshape", [o, self.const(out + "_to3", [-1, 81, F], np.int64)], out)


class Topo:
    def __init__(self, name, net, exact=True, fields=(), swaps=None):
        self.name, self.net, self.data, self.exact, self.fields = name, net, net.data(), exact, tuple(fields)
        self.swaps = swaps or {}  # {operand: [model bytes with another live tensor in its place]}


# ---- the topologies ---------------------------------------------------------------------------------------------------
def long_skip(nsg):
    n = TNet(nsg, 40, 1)
    n.int_heads("sr", 40)
    x, cin = "sr", 40
    for i, w in enumerate((16, 40, 24, 64, 16)):
        x, cin = n.conv(x, cin, w, f"c{i}"), w
    x = n.conv(x, cin, 40, "c5", res="sr")
    n.policy_conv(x, 40)
    return Topo("long_skip", n, fields=("res", "value", "draw"))


def fan_out(nsg):
    n = TNet(nsg, 64, 2)
    outs = []
    for i, (w, w2) in enumerate(zip((16, 24, 40, 64), (8, 12, 20, 24))):
        a = n.conv("sr", 64, w, f"b{i}a")
        outs.append(n.conv(a, w, w2, f"b{i}b"))
    n.node("Concat", outs, "joined", name="join", axis=1)
    n.const("cuts", [20, 27, 17], np.int64)
    n.node("Split", ["joined", "cuts"], ["left", "mid", "right"], name="cut", axis=1)
    n.node("Flatten", ["mid"], "policy", name="pflat", axis=1)
    n.int_heads("right", 17)  # the heads come after the policy
    return Topo("fan_out", n, fields=("seg", "policy"))


def early_heads(nsg):
    n = TNet(nsg, 64, 3)
    n.int_heads("sr", 64)
    x = n.chain("sr", 64, (16, 40, 24), "p")
    x = n.conv(x, 24, 64, "p3", res="sr")  # s stays alive, so the chain needs every free buffer
    x = n.chain(x, 64, (16, 40, 24), "q")
    n.policy_conv(x, 24)
    return Topo("early_heads", n, fields=("value", "draw"))


def token_and_flat(nsg):
    n = TNet(nsg, 64, 4)
    n.int_heads("sr", 64)
    t4 = n.conv("sr", 64, 16, "t4")
    tok = n.tokens(t4, 16, "tok")
    a = n.token_dense(tok, 16, 27, "first")          # the first reader: token rows
    u = n.chain("sr", 64, (40, 24, 27), "u")          # unrelated launches
    fl = n.node("Flatten", [tok], "tokflat", name="tokflat", axis=1)
    g = n.dense(fl, 81 * 16, 27, "second")            # the second reader: flat rows of 81 * 16
    back = n.node("Transpose", [a], "a_t", perm=[0, 2, 1])
    a4 = n.node("Reshape", [back, n.const("to4d", [-1, 27, 9, 9], np.int64)], "a4", name="a4")
    y = n.node("Max", [u, a4], "ua", name="ua")
    g4 = n.node("Unsqueeze", [g, n.const("ax23", [2, 3], np.int64)], "g4", name="g4")
    y = n.node("Add", [y, g4], "uag", name="uag")
    n.node("Flatten", [y], "policy", name="pflat", axis=1)
    return Topo("token_and_flat", n, fields=("in",))


def kv(nsg, swap=None):
    n = TNet(nsg, 64, 5, gain=0.25)
    n.int_heads("sr", 64)
    ops = {"k": n.tokens(n.conv("sr", 64, 16, "k4"), 16, "ktok"), "v": n.tokens(n.conv("sr", 64, 16, "v4"), 16, "vtok")}
    q = n.tokens(n.chain("sr", 64, (40, 24, 16), "u"), 16, "qtok")
    ops["q"] = q
    if swap:
        ops[swap[0]] = ops[swap[1]]
    att = n.attention(q, ops["k"], ops["v"], 16, "att")
    n.policy_of_tokens(n.token_dense(att, 16, 27, "ptok"))
    if swap:
        return n.data()
    swaps = {"attK": [kv(nsg, ("k", o)) for o in "vq"], "attV": [kv(nsg, ("v", o)) for o in "kq"]}
    return Topo("kv", n, exact=False, fields=("attK", "attV"), swaps=swaps)


def rtbias(nsg, swap=False):
    n = TNet(nsg, 64, 6, gain=0.25)
    g = n.int_heads("sr", 64)
    rts = []
    for nm in ("ra", "rb"):  # two early biases [N,6561] on the grid of 1/4, one per attention launch below
        w = n.rng.integers(-1, 2, size=(64, 6561)) * (n.rng.random((64, 6561)) < 0.1) * 0.25
        n.node("MatMul", [g, n.const(nm + "_w", w)], nm, name=nm + "_dense")
        rts.append(n.node("Reshape", [nm, n.const(nm + "_to", [-1, 1, 81, 81], np.int64)], nm + "4", name=nm + "_view"))
    if swap:
        rts.reverse()
    x = n.chain("sr", 64, (40, 24, 16), "u")
    t = n.tokens(x, 16, "xtok")
    a1 = n.attention(t, t, t, 16, "att1", bias=rts[0])
    a2 = n.attention(a1, t, t, 16, "att2", bias=rts[1])
    n.policy_of_tokens(n.token_dense(a2, 16, 27, "ptok"))
    if swap:
        return n.data()
    return Topo("rtbias", n, exact=False, fields=("rtBias",), swaps={"rtBias": [rtbias(nsg, True)]})


def bmm(nsg):
    n = TNet(nsg, 64, 7)
    n.int_heads("sr", 64)
    b = n.tokens(n.conv("sr", 64, 16, "b4"), 16, "btok")
    a = n.tokens(n.chain("sr", 64, (40, 24, 16), "u"), 16, "atok")
    bt = n.node("Transpose", [b], "bt", name="b_t", perm=[0, 2, 1])
    prod = n.node("MatMul", [a, bt], "prod", name="product")  # [N,81,81]
    for nm, val in (("st", [27]), ("en", [54]), ("ax", [2])):
        n.const("show_" + nm, val, np.int64)
    n.policy_of_tokens(n.node("Slice", [prod, "show_st", "show_en", "show_ax"], "shown", name="show"))
    return Topo("bmm", n, fields=("bmmB",))


def srcs(nsg):
    n = TNet(nsg, 64, 8)
    g = n.int_heads("sr", 64)
    e = n.conv("sr", 64, 27, "e")                                   # an early spatial tensor
    f = n.dense(g, 64, 27, "f")                                     # an early flat tensor
    ln = n.node("ReduceMax", [e], "ln", name="rank_max", axes=[3], keepdims=1)  # an early line tensor [N,27,9,1]
    ln = n.node("Add", [ln, n.const("one", [1.0])], "ln1", name="line_add")
    y = n.chain("sr", 64, (40, 24, 27), "u")
    y = n.node("Max", [y, e], "ye", name="ye")
    f4 = n.node("Unsqueeze", [f, n.const("ax23", [2, 3], np.int64)], "f4", name="f4")
    y = n.node("Add", [y, f4], "yef", name="yef")
    y = n.node("Add", [y, ln], "yefl", name="yefl")
    n.node("Flatten", [y], "policy", name="pflat", axis=1)
    return Topo("srcs", n, fields=("srcSame", "srcBoard", "srcRankLine"))


def lines18(nsg):
    n = TNet(nsg, 64, 9)
    n.int_heads("sr", 64)
    e = n.conv("sr", 64, 27, "e")
    xh = n.node("ReduceMax", [e], "xh", name="rank_max", axes=[3], keepdims=1)
    xw = n.node("ReduceMax", [e], "xw", name="file_max", axes=[2], keepdims=1)
    xwt = n.node("Transpose", [xw], "xwt", name="xw_t", perm=[0, 1, 3, 2])
    blk = n.node("Concat", [xh, xwt], "blk", name="block", axis=2)
    y = n.chain("sr", 64, (40, 24, 27), "u")
    n.const("nine", [9, 9], np.int64)
    n.node("Split", [blk, "nine"], ["yh", "ywt"], name="halves", axis=2)
    yw = n.node("Transpose", ["ywt"], "yw", name="yw_t", perm=[0, 1, 3, 2])
    # the rank half goes through a 1x1 conv over its lines (a copy of the half, kSrcLine, then the dense launch, whose
    # output is a line tensor that would fit the block's buffer): the file half alone keeps the block alive meanwhile
    yh2 = n.conv("yh", 27, 27, "late")
    y = n.node("Add", [y, yh2], "y_h", name="y_h")
    y = n.node("Mul", [y, yw], "y_hw", name="y_hw")
    n.node("Flatten", [y], "policy", name="pflat", axis=1)
    return Topo("lines18", n, fields=("srcFileLine",))


BUILDERS = {f.__name__: f for f in (long_skip, fan_out, early_heads, token_and_flat, kv, rtbias, bmm, srcs, lines18)}
NAMES = list(BUILDERS)
_BUILT = {}


def build(nsg, name):
    if name not in _BUILT:
        _BUILT[name] = BUILDERS[name](nsg)
    return _BUILT[name]


# ---- the reference ----------------------------------------------------------------------------------------------------
def reference(nsg, topo, x, data=None):
    """(policy, value, draw) in float64 on planes x.  An exact case: every tensor an integer (a multiple of 1/4 behind
    the fractional weights), every |w| |x| sum of a Conv, Gemm or MatMul below 2^24 -- float32 holds all of it."""
    worst = [0.0]

    def hook(nd, a, y):
        if not topo.exact:
            return
        assert np.array_equal(np.asarray(y), np.round(np.asarray(y))), nd.name
        if nd.op in ("Conv", "Gemm", "MatMul"):
            worst[0] = max(worst[0], float(onnx_ref64._node(nd, [None if t is None else abs(t) for t in a], nd.attrs).max()))

    out = onnx_ref64.outputs(nsg, data or topo.data, x, hook if data is None else None)
    assert worst[0] < 2 ** 24, worst[0]
    if topo.exact and data is None:
        for o in out:
            assert np.array_equal(o, o.astype(np.float32).astype(np.float64))
    return out
