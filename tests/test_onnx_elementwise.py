"""The planner's fused elementwise launches at their limits (kMaxEltSrcs = 8 sources, kMaxEltRegs = 16 registers): a
chain of supported elementwise nodes is never refused for its length or its number of inputs, it is cut into launches.
No device needed.

Each family is swept across the limits; every length must plan on the graph path, and one more node costs no launch or
exactly one.  Before the cut was added the planner refused the scalar-Mul chain at 8 nodes, the sum of pooled tensors
at 9 terms and 14 unary nodes followed by a binary one (13 and 15 planned)."""
import numpy as np
import pytest

import elt_models as em

# family -> the lengths swept
SWEEPS = {
    "scalar_mul": range(1, 21),
    "pooled_sum": range(2, 14),
    "unary_binary": range(10, 21),
    "clip": range(1, 12),
    "hardsigmoid": range(1, 8),
    "channel_mul": range(1, 13),
    "prelu": range(1, 13),
}


def clip_chain(net, x, k):
    """Clip with both bounds: two sources and four registers per node."""
    for i in range(k):
        lo, hi = net.const(f"lo{i}", [-4.0 + 0.25 * i]), net.const(f"hi{i}", [4.0 - 0.25 * i])
        x = net.node("Clip", [x, lo, hi], f"cl{i}", name=f"clip{i}")
    return x


def hardsigmoid_chain(net, x, k):
    """HardSigmoid at an alpha that is no Act code: four sources and eight registers per node."""
    for i in range(k):
        x = net.node("HardSigmoid", [x], f"hs{i}", name=f"hsig{i}", alpha=0.25, beta=0.5)
    return x


def channel_mul_chain(net, x, k):
    for i in range(k):
        x = net.node("Mul", [x, net.const(f"g{i}", np.linspace(0.5, 1.5, em.F).reshape(em.F, 1, 1))], f"cm{i}", name=f"cmul{i}")
    return x


def prelu_chain(net, x, k):
    for i in range(k):
        x = net.node("PRelu", [x, net.const(f"sl{i}", np.linspace(-0.5, 1.5, em.F).reshape(em.F, 1, 1))], f"pr{i}", name=f"prelu{i}")
    return x


CHAINS = dict(em.FAMILIES, clip=clip_chain, hardsigmoid=hardsigmoid_chain, channel_mul=channel_mul_chain, prelu=prelu_chain)


def launches(nsg, family, length):
    net = em.Net(nsg)
    s = net.stem()
    info = nsg.inspect_onnx(net.finish(CHAINS[family](net, s, length), s), 86)
    assert info["path"] == "graph", (family, length)
    # the pooled sum's terms are one MaxPool launch each: what is counted is the elementwise launches
    return info["launches"] - (length if family == "pooled_sum" else 0)


@pytest.fixture(scope="module")
def counts(nsg):
    """family -> {length: launches (without the pooled sum's MaxPool launches)}, planned once; a refusal is kept as the
    error it raised."""
    out = {}
    for family, lengths in SWEEPS.items():
        out[family] = {}
        for n in lengths:
            try:
                out[family][n] = launches(nsg, family, n)
            except nsg.NsgError as e:
                out[family][n] = e
    return out


@pytest.mark.parametrize("family", list(SWEEPS))
def test_every_length_plans_and_a_node_costs_at_most_one_launch(counts, family):
    got = counts[family]
    for n, c in got.items():
        assert isinstance(c, int), f"{family} of length {n} is refused: {c}"
    lengths = list(got)
    for a, b in zip(lengths, lengths[1:]):
        assert got[b] in (got[a], got[a] + 1), (family, a, got[a], b, got[b])


def test_the_cuts_fall_at_the_limits(counts):
    """Seven scalar Mul nodes are 8 sources and 15 registers, one launch; the eighth starts a second launch, which
    again holds seven (it reads the first launch's result as its one runtime source).  Eight pooled tensors are one
    launch of 8 sources, the ninth is added by a second.  One source and u unary nodes are u + 1 registers: the Mul
    with its constant needs two more, so it joins up to u = 13 and is a launch of its own behind 14 or 15; the
    sixteenth unary node starts the second launch itself."""
    m = counts["scalar_mul"]
    assert [m[k] - m[1] for k in (7, 8, 14, 15, 20)] == [0, 1, 1, 2, 2]
    p = counts["pooled_sum"]
    assert [p[n] - p[2] for n in (8, 9, 13)] == [0, 1, 1]
    u = counts["unary_binary"]
    assert [u[k] - u[10] for k in (13, 14, 15, 16, 20)] == [0, 1, 1, 1, 1]


@pytest.mark.parametrize("order", ["big_first", "small_first"])
def test_two_open_groups_that_do_not_fit_together(nsg, order):
    """abs(a * c0 .. c5) is an open group of 7 sources and 14 registers, b * c one of 2 and 3: together 9 sources.
    The first operand is inlined, the other is launched and read as one source, in either operand order."""
    net = em.Net(nsg)
    a, b = net.split_stem()
    big = net.node("Abs", [em.scalar_mul_chain(net, a, 6)], "big")
    small = net.node("Mul", [b, net.const("cs", [0.5])], "small")
    y = net.node("Sub", [big, small] if order == "big_first" else [small, big], "y")
    info = nsg.inspect_onnx(net.finish(y, a), 86)
    assert info["path"] == "graph"
    # stem, two elementwise launches, mean, two dense, outputs and the planes' expansion: the same count both ways
    single = em.Net(nsg)
    a1, _ = single.split_stem()
    base = nsg.inspect_onnx(single.finish(single.node("Abs", [a1], "y"), a1), 86)["launches"]
    assert info["launches"] == base + 1


def test_a_runtime_batchnorm_behind_a_full_group_plans(nsg):
    """BatchNormalization on a runtime tensor is 3 sources and 5 registers: behind a group of 7 sources it is cut."""
    for k in range(4, 9):
        net = em.Net(nsg)
        s = net.stem()
        x = em.scalar_mul_chain(net, s, k)
        for nm, v in (("g", 1.0), ("bt", 0.5), ("mn", 0.25), ("vr", 4.0)):
            net.const(nm, np.full(em.F, v))
        y = net.node("BatchNormalization", [x, "g", "bt", "mn", "vr"], "y", name="bn")
        assert nsg.inspect_onnx(net.finish(y, s), 86)["path"] == "graph", k


# launches per forward of the shipped fixtures, measured before the cut was added: it moves no launch of theirs
FIXTURE_LAUNCHES = {"net_graph_se": 24, "net_graph_pool": 32, "net_graph_norm": 25, "net_att_pre": 24}


@pytest.mark.parametrize("name", list(FIXTURE_LAUNCHES))
def test_fixture_launch_counts_are_unchanged(nsg, golden_dir, name):
    with open(f"{golden_dir}/{name}.onnx", "rb") as f:
        info = nsg.inspect_onnx(f.read(), 86)
    assert info["launches"] == FIXTURE_LAUNCHES[name]
