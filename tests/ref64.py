"""A batched float64 restatement of the network, and the localisation check the plan sweep applies with it.

The reference shares no code with the kernels or with the C oracle: torch on the CPU, float64 throughout, BatchNorm
left unfolded and computed from (gamma, beta, mean, var, eps) of the weight dict, each 3x3 convolution as nine shifted
matrix products over the whole batch.  Input: the weight dict of nsg.weights.make_random / from_blob and the feature
planes of oracle.extract_bits ([B, C, 81] float32).  The heads follow oracle/oracle.c: the 1x1 policy convolution
with bias; value convolution -> BN -> ReLU -> fc1 -> ReLU -> fc2; value = (tanh + 1) / 2, draw = sigmoid.

It never touches the GPU and runs on at most 16 host threads.
"""
import numpy as np
import torch

MAX_THREADS = 16
_CACHE = {}


class _Threads:
    def __enter__(self):
        self.prev = torch.get_num_threads()
        torch.set_num_threads(max(1, min(MAX_THREADS, self.prev)))

    def __exit__(self, *exc):
        torch.set_num_threads(self.prev)


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64).copy())


def _bn(acc, p, eps):
    """acc [..., F] float64; p [4, F] = (gamma, beta, mean, var)."""
    g, b, mu, var = (_t(p[i]) for i in range(4))
    return (acc - mu) * (g / torch.sqrt(var + eps)) + b


def _conv3x3(x, w, layer, hook):
    """x [B, 9, 9, Cin] float64, w [F, Cin, 3, 3] -> pre-BN accumulator [B, 9, 9, F]."""
    B, _, _, cin = x.shape
    xp = torch.zeros((B, 11, 11, cin), dtype=torch.float64)
    xp[:, 1:10, 1:10, :] = x
    wt = _t(w).permute(2, 3, 1, 0).contiguous()  # [3, 3, Cin, F]
    acc = torch.zeros((B * 81, wt.shape[-1]), dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            acc += xp[:, ky:ky + 9, kx:kx + 9, :].reshape(B * 81, cin) @ wt[ky, kx]
    acc = acc.view(B, 9, 9, -1)
    if hook is not None:
        hook(layer, xp, wt, acc)
    return acc


def forward(w, planes, round_to=None, hook=None):
    """Returns {"trunk": [B, F, 81], "policy": [B, 2187], "value": [B], "draw": [B]} as float64 numpy arrays.

    round_to (torch.float16 / torch.bfloat16): every layer's output activation is rounded to that type (a model of
    the rounding noise of a reduced-precision trunk).  hook(layer, padded_input [B, 11, 11, Cin], taps [3, 3, Cin, F],
    acc [B, 9, 9, F]) may change a 3x3 layer's accumulator in place before its BatchNorm (layer 0 = the stem)."""
    m = w["_meta"]
    eps = float(np.float32(m["bn_eps"]))  # the value the weight file stores
    F, cin = m["channels"], m["in_channels"]
    planes = np.asarray(planes, dtype=np.float32)
    B = planes.shape[0]

    def rnd(a):
        return a if round_to is None else a.to(round_to).to(torch.float64)

    with _Threads(), torch.no_grad():
        x = _t(planes).view(B, cin, 9, 9).permute(0, 2, 3, 1).contiguous()  # NHWC
        x = rnd(torch.relu(_bn(_conv3x3(x, w["stem_w"], 0, hook), w["stem_bn"], eps)))
        for k in range(m["blocks"]):
            y = rnd(torch.relu(_bn(_conv3x3(x, w[f"b{k}_w1"], 2 * k + 1, hook), w[f"b{k}_bn1"], eps)))
            z = _bn(_conv3x3(y, w[f"b{k}_w2"], 2 * k + 2, hook), w[f"b{k}_bn2"], eps)
            x = rnd(torch.relu(z + x))
        xs = x.reshape(B, 81, F)
        pol = xs @ _t(w["policy_w"]).T + _t(w["policy_b"])  # [B, 81, 27]
        pol = pol.permute(0, 2, 1).reshape(B, -1)
        v = torch.relu(_bn(xs @ _t(w["value_w"]).T, w["value_bn"], eps))  # [B, 81, VC]
        v = v.permute(0, 2, 1).reshape(B, -1)
        h = torch.relu(v @ _t(w["fc1_w"]).T + _t(w["fc1_b"]))
        o = h @ _t(w["fc2_w"]).T + _t(w["fc2_b"])
        value = 0.5 * (torch.tanh(o[:, 0]) + 1.0)
        draw = torch.sigmoid(o[:, 1])
        trunk = xs.permute(0, 2, 1).contiguous()
    return {"trunk": trunk.numpy(), "policy": pol.numpy(), "value": value.numpy(), "draw": draw.numpy()}


def cached(key, w, planes):
    """forward(w, planes) computed once per key for the session.  Boards are independent, so a caller computes the
    largest batch of a (net, input set) once and slices it (take())."""
    if key not in _CACHE:
        _CACHE[key] = forward(w, planes)
    return _CACHE[key]


def take(ref, idx):
    """The reference of the boards idx (a slice or an index array) of a cached batch."""
    return {k: v[idx] for k, v in ref.items()}


# ---------------------------------------------------------------------------------------------------------------
# Localisation.  An absolute tolerance wide enough for fp16 or bf16 rounding also passes a kernel that drops a tap
# of one square, mishandles one workgroup slot or one 16-channel fragment: such a mistake is small next to the
# tolerance but it is CONCENTRATED.  The trunk error |gpu - ref|, normalised per board by that board's reference
# RMS, is reduced to its RMS along three axes -- per square (81), per board slot (B), per 16-channel fragment
# (F / 16) -- and on each axis the largest entry must stay within bound x median + floor.  Rounding noise spreads
# evenly over all three axes; a localised mistake raises one entry of at least one of them.

AXES = ("square", "slot", "fragment")

# (bound on max / median, floor) per trunk precision.  The bounds are twice the largest clean ratio measured on an
# MI355X over the whole plan sweep (tests/test_gpu_plan_sweep.py) or more; the floor (normalised error) keeps the
# exact precisions, whose error is at the level of float32 rounding, from failing on ratios of tiny numbers.
LOCALISATION_BOUNDS = {
    "fp32": (4.0, 1e-6),   # largest clean ratio 1.85 (64 channels, square axis)
    "f16x3": (3.0, 1e-6),  # 1.40
    "f16m8": (3.0, 1e-6),  # 1.44
    "f16m6": (3.0, 1e-6),  # 1.48
    "fp16": (3.0, 1e-6),   # 1.32
    "bf16": (3.0, 1e-6),   # 1.37
}


def localisation(trunk, ref_trunk):
    """{axis: (max, median)} of the per-board-normalised trunk error's RMS along each axis."""
    ref_trunk = np.asarray(ref_trunk, dtype=np.float64)
    B, F, _ = ref_trunk.shape
    scale = np.sqrt(np.mean(ref_trunk ** 2, axis=(1, 2)))
    e2 = ((np.asarray(trunk, dtype=np.float64) - ref_trunk) / np.maximum(scale, 1e-30)[:, None, None]) ** 2
    per = {
        "square": np.sqrt(e2.mean(axis=(0, 1))),
        "slot": np.sqrt(e2.mean(axis=(1, 2))),
        "fragment": np.sqrt(e2.reshape(B, F // 16, 16, 81).mean(axis=(0, 2, 3))),
    }
    return {a: (float(v.max()), float(np.median(v))) for a, v in per.items()}


def localisation_failures(loc, precision):
    """Axes of localisation() whose largest entry exceeds bound x median + floor, with their ratios."""
    bound, floor = LOCALISATION_BOUNDS[precision]
    return {a: mx / max(med, 1e-300) for a, (mx, med) in loc.items() if mx > bound * med + floor}


def localisation_ratios(loc):
    return {a: mx / max(med, 1e-300) for a, (mx, med) in loc.items()}
