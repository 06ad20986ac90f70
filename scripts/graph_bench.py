"""Throughput of the general graph path against the specialised path, on the same network.

    python scripts/graph_bench.py [--out profiles/graph/graph_bench.json] [--batches 1,64,512]
    python scripts/graph_bench.py --trace      # one shape of two nets for `rocprofv3 --kernel-trace --stats`
    python scripts/graph_bench.py --summarize DIR/run_results.db   # per-kernel times and each conv kernel's share of peak
    python scripts/graph_bench.py --attention [--out profiles/graph/attention_bench.json]   # the transformer row
    python scripts/graph_bench.py --trace-attention      # one shape of it for `rocprofv3 --kernel-trace --stats`
    python scripts/graph_bench.py --summarize-attention DIR/run_results.db   # each kernel's share of that forward
    python scripts/graph_bench.py --pool [--out profiles/graph/pool_bench.json]   # the pooling row
    python scripts/graph_bench.py --trace-pool      # it, a depthwise 3x3 and the family net for `rocprofv3 --kernel-trace`
    python scripts/graph_bench.py --summarize-pool DIR/run_results.db   # graphPool against graphDepthwise and 8 TB/s
    python scripts/graph_bench.py --norm [--out profiles/graph/norm_bench.json]   # the GroupNorm row
    python scripts/graph_bench.py --trace-norm      # GroupNorm at three group counts, a max pool and a depthwise 3x3
    python scripts/graph_bench.py --summarize-norm DIR/run_results.db [--out profiles/graph/norm_bench.json]
    python scripts/graph_bench.py --mish [--out profiles/graph/mish_bench.json] [--repeats 3]   # the Mish row
    python scripts/graph_bench.py --smolgen [--out profiles/graph/smolgen_bench.json] [--repeats 3]   # the run-time bias row
    python scripts/graph_bench.py --trace-smolgen      # both transformers at B = 512 for `rocprofv3 --kernel-trace`
    python scripts/graph_bench.py --summarize-smolgen DIR/run_results.db   # graphAttention with and without the bias
    python scripts/graph_bench.py --group [--out profiles/graph/group_bench.json] [--repeats 3]   # the grouped-conv row
    python scripts/graph_bench.py --trace-group      # the ResNeXt net and its dense twin at B = 1, 32, 128, 512 for `rocprofv3 --kernel-trace`
    python scripts/graph_bench.py --summarize-group DIR/run_results.db [--out profiles/graph/group_bench.json]
    python scripts/graph_bench.py --gate [--out profiles/graph/gate_bench.json] [--repeats 3]   # the scSE row

Rows: the 20x256 family net forced onto the general path; the same net on the specialised fp32 and f16m6 paths; an
SE-swish 20x256 net (squeeze-and-excitation, swish; tests/golden/make_onnx_graph_golden.py's SENet) exported at run
time with PyTorch's exporter; a geometry 20x256 net (tests/golden/make_onnx_geometry_golden.py's GeomBenchNet: a 5x5
stem, four blocks of two 5x5 convs, sixteen depthwise 7x7 + pointwise blocks), exported the same way.  evals/s =
positions / wall time of `iters` computeBlocking calls after a warm-up.
Also the SE net's load time (nsg_load on the .onnx file, planning and upload included).

--pool: a pooling 20x256 net (tests/golden/make_onnx_pool_golden.py's PoolBenchNet: blocks that alternate the
KataGo-style pooled bias and the inception-style 3x3 max / average pooling branch), exported at run time.  --trace-pool
runs it at B = 512 beside a bare depthwise 3x3 of 256 channels (graphDepthwise: the yardstick of graphPool, same bytes,
more work) and the forced family net (graphConv<9>, which must not move), all in one process.

--norm: the 20x256 residual net with GroupNorm(32 groups)-ReLU in place of every BatchNorm-ReLU
(tests/golden/make_onnx_norm_golden.py's NormBenchNet), exported at run time.  --trace-norm runs, in one process at
B = 512 and C = 256, a bare GroupNorm of 32 groups, of 256 groups (instance norm) and of one group (graphGroupNorm), a
3x3 max pool (graphPool) and a bare depthwise 3x3 (graphDepthwise): five kernels that each read and write the same
84.9 MB.  --summarize-norm prints their medians and ranges and adds them to the --norm file.

--mish: the 20x256 residual net with Mish for every ReLU (tests/golden/make_onnx_math_golden.py's MishBenchNet: every
Mish rides in a conv's launch), the same net with swish, and the 20x256 family net forced onto the general path, each
timed `--repeats` times in turn; the file holds every repeat, so the run's spread is in it.

--attention: a pre-LN transformer over the 81 squares (tests/golden/make_onnx_attention_golden.py's PreNet with 8
blocks, F = 256, H = 8 heads of d = 32, FFN width 1024), exported at run time, on the general path.

--smolgen: the --attention transformer with a bias generator in every block (tests/attention_bias_models.py's
SmolgenPreNet: token Linear(256,32), flatten, Linear(2592,256) + swish, Linear(256,8x64), LayerNorm, head rows, one shared
Linear(64,6561), the Add into the scores), beside the plain --attention net, each timed `--repeats` times in turn.
--trace-smolgen runs both at B = 512 in one process; --summarize-smolgen prints the median and range of every
graphAttention instantiation (`<2, false>`: no run-time bias, `<2, true>`: with one) and of the head-row dense launch.

--group: a ResNeXt-style 20x256 net (tests/group_models.py's ResNeXtNet: blocks of 1x1 -> 3x3 grouped, G = 8, 32 per
group, with BatchNorm and ReLU -> 1x1, plus the residual), its twin with groups = 1 in the 3x3, and the forced family
net, each timed `--repeats` times in turn at B = 1, 32, 128, 512.  --trace-group runs the two ResNeXt nets at those
batches in one process (GROUP_FORWARDS forwards each); --summarize-group prints, per batch, the median and range of the
grouped launch (graphConvGrouped) and of the twin's dense 3x3 256 -> 256 launch (graphConv<9>, the stem left out) and
adds them to the --group file.

--gate: the 20x256 residual net with an scSE gate in every block (tests/gate_models.py's gate_bench_net: per block one
one-channel 1x1 conv and one elementwise launch that reads it through kSrcRowOne) beside the SE-swish net, each timed
`--repeats` times in turn at the --batches.
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def family_onnx(nsg, path):
    w = nsg.weights.make_random(20, 256, seed=1, bn="random")
    nsg.onnx_io.export_onnx(w, path)


def se_onnx(path):
    import torch
    import make_onnx_graph_golden as mk
    torch.manual_seed(5)
    net = mk.randomize_bn(mk.SENet(C=86, F=256, blocks=20, VC=32, VH=256), 13).eval()
    mk.export_model(net, path, 86, True)


def geometry_onnx(path):
    import torch
    import make_onnx_geometry_golden as mk
    torch.manual_seed(7)
    net = mk.randomize(mk.GeomBenchNet(C=86, F=256, blocks=20, VC=32, VH=256), 15).eval()
    mk.export_model(net, path)


def pool_onnx(path):
    import torch
    import make_onnx_pool_golden as mk
    torch.manual_seed(8)
    net = mk.randomize(mk.PoolBenchNet(C=86, F=256, blocks=20), 16).eval()
    mk.export_model(net, path)


def norm_onnx(path):
    import torch
    import make_onnx_norm_golden as mk
    torch.manual_seed(10)
    mk.export_model(mk.randomize(mk.NormBenchNet(C=86, F=256, blocks=20, G=32), 18).eval(), path)


def groupnorm_onnx(path, groups):
    """A 3x3 stem of 256 channels and one bare GroupNorm behind it."""
    import torch
    import make_onnx_norm_golden as mk
    torch.manual_seed(11)
    mk.export_model(mk.randomize(mk.NormNet(256, torch.nn.GroupNorm(groups, 256)), 19).eval(), path)


def maxpool3_onnx(path):
    import torch
    import make_onnx_norm_golden as mk
    torch.manual_seed(12)
    mk.export_model(mk.randomize(mk.NormNet(256, torch.nn.MaxPool2d(3, 1, 1)), 20).eval(), path)


def depthwise3_onnx(path):
    import torch
    import make_onnx_geometry_golden as mk
    torch.manual_seed(9)
    mk.export_model(mk.randomize(mk.DwNet(256, 3, full=False), 17).eval(), path)


def mish_onnx(path, swish=False):
    import torch
    import torch.nn.functional as Fn
    import make_onnx_math_golden as mk
    torch.manual_seed(13)
    mk.export_model(mk.randomize(mk.MishBenchNet(C=86, F=256, blocks=20, act=Fn.silu if swish else Fn.mish), 21).eval(), path)


def gate_onnx(path):
    import torch
    import gate_models as gm
    import make_onnx_norm_golden as mk
    torch.manual_seed(14)
    mk.export_model(gm.randomize(gm.gate_bench_net(C=86, Fw=256, blocks=20), 22).eval(), path)


def attention_onnx(path):
    import torch
    import make_onnx_attention_golden as mk
    torch.manual_seed(6)
    net = mk.randomize(mk.PreNet(C=86, F=256, H=8, ffn=1024, VH=256, blocks=8), 14).eval()
    mk.export_model(net, path)


def smolgen_onnx(path):
    import torch
    import attention_bias_models as abm
    import make_onnx_attention_golden as mk
    torch.manual_seed(16)
    mk.export_model(mk.randomize(abm.SmolgenPreNet(), 24).eval(), path)


GROUP_BATCHES = (1, 32, 128, 512)
GROUP_FORWARDS = 8  # --trace-group: 3 warm-up + 5 timed forwards per (net, batch)
GROUP_BLOCKS = 20


def group_onnx(path, groups):
    """The ResNeXt-style 20x256 net; groups = 1 is the dense twin (the same seeds: every other layer is identical)."""
    import torch
    import group_models as gm
    torch.manual_seed(14)
    net = gm.randomize(gm.ResNeXtNet(F=256, groups=groups, blocks=GROUP_BLOCKS, swish=False, VC=32, VH=256), 22).eval()
    gm.export(net, path)


def summarize_group(db, out):
    """A --trace-group run: the grouped net first, then the twin, each at GROUP_BATCHES in order, GROUP_FORWARDS forwards
    of GROUP_BLOCKS 3x3 launches per batch (the twin's graphConv<9> launches one more per forward: the stem, left out)."""
    import sqlite3
    import statistics
    c = sqlite3.connect(db)
    print(f"{'kernel':60s} {'calls':>6s} {'total ms':>10s} {'avg us':>9s}")
    for n, k, t, a in c.execute("select name, count(*), sum(end-start), avg(end-start) from kernels group by name "
                                "order by sum(end-start) desc"):
        short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{short:60s} {k:6d} {t / 1e6:10.2f} {a / 1e3:9.1f}")
    print()
    g = [r[0] for r in c.execute("select end-start from kernels where name like '%graphConvGrouped%' order by start")]
    d = [r[0] for r in c.execute("select end-start from kernels where name like '%graphConv<9>%' order by start")]
    per_g, per_d = GROUP_FORWARDS * GROUP_BLOCKS, GROUP_FORWARDS * (GROUP_BLOCKS + 1)
    # graphConv<9>: the grouped net's own stems come first (one launch per forward), then the twin's stem + 20 per forward
    d = d[GROUP_FORWARDS * len(GROUP_BATCHES):]
    res = {}
    for i, b in enumerate(GROUP_BATCHES):
        gs = g[i * per_g:(i + 1) * per_g]
        ds = [t for j, t in enumerate(d[i * per_d:(i + 1) * per_d]) if j % (GROUP_BLOCKS + 1) != 0]
        # the warm-up forwards are left out of both
        gs, ds = gs[3 * GROUP_BLOCKS:], ds[3 * GROUP_BLOCKS:]
        if not gs or not ds:
            continue
        row = {}
        for label, ts in (("grouped_3x3_g8", gs), ("dense_3x3", ds)):
            row[label] = {"median_us": round(statistics.median(ts) / 1e3, 1), "min_us": round(min(ts) / 1e3, 1),
                          "max_us": round(max(ts) / 1e3, 1), "launches": len(ts)}
        row["dense_over_grouped"] = round(statistics.median(ds) / statistics.median(gs), 2)
        res[str(b)] = row
        print(f"B={b}: graphConvGrouped 3x3 256->256 G=8 median {row['grouped_3x3_g8']['median_us']} us (min "
              f"{row['grouped_3x3_g8']['min_us']}, max {row['grouped_3x3_g8']['max_us']}, {len(gs)} launches); graphConv<9> dense "
              f"3x3 256->256 median {row['dense_3x3']['median_us']} us (min {row['dense_3x3']['min_us']}, max "
              f"{row['dense_3x3']['max_us']}, {len(ds)} launches); dense / grouped = {row['dense_over_grouped']}")
    if out:
        doc = {}
        if os.path.exists(out):
            with open(out) as f:
                doc = json.load(f)
        doc["trace_3x3_256_launch"] = res
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)


def summarize_smolgen(db):
    """graphAttention per instantiation (a --trace-attention or --trace-smolgen run): launches, median, range in us."""
    import sqlite3
    import statistics
    c = sqlite3.connect(db)
    by = {}
    for n, t in c.execute("select name, end-start from kernels"):
        if "graphAttention" in n or "graphConv<1>" in n:
            short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            by.setdefault(short, []).append(t / 1e3)
    for n, ts in sorted(by.items()):
        print(f"{n:50s} n={len(ts):5d} median {statistics.median(ts):9.1f} us  min {min(ts):9.1f}  max {max(ts):9.1f}")


def rate(nsg, path, batch, prec="fp32", force=False, iters=50, warmup=5):
    ev = nsg.Evaluator(0, batch, 86, precision=prec)
    if force:
        ev.set_graph_mode("force")
    ev.load(path)
    bb = nsg.synth.random_batch(batch, 86, seed=3)
    for _ in range(warmup):
        ev.compute_blocking(bb)
    t0 = time.perf_counter()
    for _ in range(iters):
        ev.compute_blocking(bb)
    dt = time.perf_counter() - t0
    info = ev.graph_info()
    ev.close()
    return batch * iters / dt, info


TRACE_BATCH, TRACE_FORWARDS = 512, 23  # --trace: 3 warm-up + 20 timed forwards of the 20x256 net at B = 512 ...
GEOM_FORWARDS = 8                      # ... then 3 + 5 of the geometry net
POOL_FAMILY_FORWARDS = 8               # --trace-pool: 3 + 5 forwards of each of its three nets
HBM_PEAK = 8.0e12  # bytes/s
F32_MFMA_PEAK = 157.3e12  # FLOP/s at the 2.4 GHz peak clock (MI355X_MICROARCH): the run's clock is not sampled


def summarize(db):
    """The kernel table of a --trace run (rocprofv3's SQLite output) and the 3x3 conv's share of the f32 MFMA peak:
    algorithmic FLOPs (2 * 81 * 9 * Cin * Cout per board, real channel counts) over measured kernel time."""
    import sqlite3
    import statistics
    c = sqlite3.connect(db)
    print(f"{'kernel':60s} {'calls':>6s} {'total ms':>10s} {'avg us':>9s}")
    for n, k, t, a in c.execute("select name, count(*), sum(end-start), avg(end-start) from kernels group by name "
                                "order by sum(end-start) desc"):
        short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{short:60s} {k:6d} {t / 1e6:10.2f} {a / 1e3:9.1f}")
    d = [r[0] for r in c.execute("select end-start from kernels where name like '%graphConv<9>%' order by start")]
    per_fwd = 41  # the stem + 40 residual-block convs
    fl_main = 2.0 * TRACE_BATCH * 81 * 9 * 256 * 256
    fl_stem = 2.0 * TRACE_BATCH * 81 * 9 * 86 * 256
    main_ns = [d[i] for i in range(len(d)) if i % per_fwd != 0]
    m = statistics.median(main_ns) * 1e-9
    print()
    print(f"3x3 256->256 conv, B={TRACE_BATCH}: {fl_main / 1e9:.2f} GFLOP per launch, median {m * 1e6:.1f} us over "
          f"{len(main_ns)} launches = {fl_main / m / 1e12:.1f} TFLOP/s = {fl_main / m / F32_MFMA_PEAK:.3f} of the f32 MFMA "
          f"peak at the peak clock (the run's clock was not sampled)")
    tot = sum(d) * 1e-9 / (len(d) / per_fwd)
    print(f"all 3x3 launches of a forward: {tot * 1e3:.2f} ms for {(40 * fl_main + fl_stem) / 1e9:.1f} GFLOP = "
          f"{(40 * fl_main + fl_stem) / tot / F32_MFMA_PEAK:.3f} of peak")
    one = [r[0] for r in c.execute("select end-start from kernels where name like '%graphConv<1>%' order by start")]
    one = one[:5 * (len(d) // per_fwd)]  # the family net's: two head convs and three dense layers per forward, run first
    if one:
        print(f"1x1 / dense launches of the family net (graphConv<1>): {len(one)} launches, avg {statistics.mean(one) / 1e3:.1f} us, "
              f"total {sum(one) / 1e6:.2f} ms")
    # the geometry net (GeomBenchNet): per forward a 5x5 stem and eight 5x5 256->256 convs on graphConvGeo, sixteen
    # depthwise 7x7 convs of 256 channels on graphDepthwise
    geo = [r[0] for r in c.execute("select end-start from kernels where name like '%graphConvGeo%' order by start")]
    if geo:
        main_geo = [geo[i] for i in range(len(geo)) if i % 9 != 0]
        fl5 = 2.0 * TRACE_BATCH * 81 * 25 * 256 * 256
        m5 = statistics.median(main_geo) * 1e-9
        print(f"5x5 256->256 conv (graphConvGeo), B={TRACE_BATCH}: {fl5 / 1e9:.2f} GFLOP per launch, median {m5 * 1e6:.1f} us "
              f"over {len(main_geo)} launches = {fl5 / m5 / 1e12:.1f} TFLOP/s = {fl5 / m5 / F32_MFMA_PEAK:.3f} of the f32 MFMA "
              f"peak (3x3 on graphConv<9> in this run: {fl_main / m / F32_MFMA_PEAK:.3f})")
    dwt = [r[0] for r in c.execute("select end-start from kernels where name like '%graphDepthwise%' order by start")]
    if dwt:
        by = 2.0 * TRACE_BATCH * 81 * 256 * 4  # one read and one write of the activation (no residual on this launch)
        md = statistics.median(dwt) * 1e-9
        print(f"depthwise 7x7, C=256, B={TRACE_BATCH}: {by / 1e6:.1f} MB per launch, median {md * 1e6:.1f} us over {len(dwt)} "
              f"launches = {by / md / 1e12:.2f} TB/s = {by / md / HBM_PEAK:.3f} of {HBM_PEAK / 1e12:.0f} TB/s")


def summarize_pool(db):
    """graphPool (3x3, C = 256, B = 512; PoolBenchNet launches the max pool of a block before its average pool) as bytes
    moved over time, beside graphDepthwise 3x3 at the same C and B and graphConv<9> of the forced family net, all from
    one --trace-pool run."""
    import sqlite3
    import statistics
    c = sqlite3.connect(db)
    print(f"{'kernel':60s} {'calls':>6s} {'total ms':>10s} {'avg us':>9s}")
    for n, k, t, a in c.execute("select name, count(*), sum(end-start), avg(end-start) from kernels group by name "
                                "order by sum(end-start) desc"):
        short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{short:60s} {k:6d} {t / 1e6:10.2f} {a / 1e3:9.1f}")
    by = 2.0 * TRACE_BATCH * 81 * 256 * 4  # one read and one write of the activation
    print()
    pl = [r[0] for r in c.execute("select end-start from kernels where name like '%graphPool%' order by start")]
    dwt = [r[0] for r in c.execute("select end-start from kernels where name like '%graphDepthwise%' order by start")]
    for label, d in (("graphPool 3x3 max", pl[0::2]), ("graphPool 3x3 avg (exclude pad)", pl[1::2]), ("graphDepthwise 3x3", dwt)):
        if not d:
            continue
        m = statistics.median(d) * 1e-9
        print(f"{label}, C=256, B={TRACE_BATCH}: {by / 1e6:.1f} MB per launch, median {m * 1e6:.1f} us (min {min(d) / 1e3:.1f}, max "
              f"{max(d) / 1e3:.1f}) over {len(d)} launches = {by / m / 1e12:.2f} TB/s = {by / m / HBM_PEAK:.3f} of "
              f"{HBM_PEAK / 1e12:.0f} TB/s")
    d = [r[0] for r in c.execute("select end-start from kernels where name like '%graphConv<9>%' order by start")]
    # the family net runs last: 41 launches per forward, the stem first
    fam = d[-41 * POOL_FAMILY_FORWARDS:]
    main_ns = [fam[i] for i in range(len(fam)) if i % 41 != 0]
    if main_ns:
        print(f"family net, 3x3 256->256 on graphConv<9>, B={TRACE_BATCH}: median {statistics.median(main_ns) / 1e3:.1f} us (min "
              f"{min(main_ns) / 1e3:.1f}, max {max(main_ns) / 1e3:.1f}) over {len(main_ns)} launches")


NORM_TRACE = (("graphGroupNorm G=32", 32), ("graphGroupNorm G=256", 256), ("graphGroupNorm G=1", 1))


def summarize_norm(db, out):
    """graphGroupNorm at C = 256, B = 512 with 32, 256 and 1 groups (run in that order, POOL_FAMILY_FORWARDS launches
    each) beside graphPool 3x3 max and graphDepthwise 3x3 from the same --trace-norm run: the same bytes each."""
    import sqlite3
    import statistics
    c = sqlite3.connect(db)
    print(f"{'kernel':60s} {'calls':>6s} {'total ms':>10s} {'avg us':>9s}")
    for n, k, t, a in c.execute("select name, count(*), sum(end-start), avg(end-start) from kernels group by name "
                                "order by sum(end-start) desc"):
        short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{short:60s} {k:6d} {t / 1e6:10.2f} {a / 1e3:9.1f}")
    by = 2.0 * TRACE_BATCH * 81 * 256 * 4  # one read and one write of the activation
    print()
    gn = [r[0] for r in c.execute("select end-start from kernels where name like '%graphGroupNorm%' order by start")]
    rows = [(label, gn[i * POOL_FAMILY_FORWARDS:(i + 1) * POOL_FAMILY_FORWARDS]) for i, (label, _) in enumerate(NORM_TRACE)]
    rows.append(("graphPool 3x3 max", [r[0] for r in c.execute("select end-start from kernels where name like '%graphPool%' order by start")]))
    rows.append(("graphDepthwise 3x3", [r[0] for r in c.execute("select end-start from kernels where name like '%graphDepthwise%' order by start")]))
    res = {}
    for label, d in rows:
        if not d:
            continue
        m = statistics.median(d) * 1e-9
        res[label] = {"median_us": round(m * 1e6, 1), "min_us": round(min(d) / 1e3, 1), "max_us": round(max(d) / 1e3, 1),
                      "launches": len(d), "TB_per_s": round(by / m / 1e12, 2)}
        print(f"{label}, C=256, B={TRACE_BATCH}: {by / 1e6:.1f} MB per launch, median {m * 1e6:.1f} us (min {min(d) / 1e3:.1f}, max "
              f"{max(d) / 1e3:.1f}) over {len(d)} launches = {by / m / 1e12:.2f} TB/s = {by / m / HBM_PEAK:.3f} of "
              f"{HBM_PEAK / 1e12:.0f} TB/s")
    if out:
        doc = {}
        if os.path.exists(out):
            with open(out) as f:
                doc = json.load(f)
        doc["trace_b512_c256"] = res
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)


def summarize_attention(db):
    """Each kernel's share of the transformer's forward (a --trace-attention run), and the attention + LayerNorm time
    against the dense launches' (graphConv<1>)."""
    import sqlite3
    c = sqlite3.connect(db)
    rows = list(c.execute("select name, count(*), sum(end-start), avg(end-start) from kernels group by name "
                          "order by sum(end-start) desc"))
    total = sum(r[2] for r in rows)
    print(f"{'kernel':60s} {'calls':>6s} {'total ms':>10s} {'avg us':>9s} {'share':>7s}")
    group = {"dense": 0, "attention": 0, "layernorm": 0}
    for n, k, t, a in rows:
        short = n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        print(f"{short:60s} {k:6d} {t / 1e6:10.2f} {a / 1e3:9.1f} {t / total:7.3f}")
        for key, pat in (("dense", "graphConv<1>"), ("attention", "graphAttention"), ("layernorm", "graphLayerNorm")):
            if pat in n:
                group[key] += t
    print()
    print("share of all kernel time: " + ", ".join(f"{k} {v / total:.3f}" for k, v in group.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph", "graph_bench.json"))
    ap.add_argument("--batches", default="1,64,512")
    ap.add_argument("--trace", action="store_true",
                    help="only the forced 20x256 general path at B=512, 20 forwards, then the geometry net, 5 forwards")
    ap.add_argument("--summarize", metavar="DB", help="summarise the rocprofv3 database of a --trace run")
    ap.add_argument("--attention", action="store_true", help="the 8-block F=256 H=8 transformer on the general path")
    ap.add_argument("--trace-attention", action="store_true", help="only that transformer at B=512, 13 forwards")
    ap.add_argument("--summarize-attention", metavar="DB", help="summarise the rocprofv3 database of a --trace-attention run")
    ap.add_argument("--pool", action="store_true", help="the pooling 20x256 net on the general path")
    ap.add_argument("--trace-pool", action="store_true", help="it, a depthwise 3x3 and the forced family net at B=512, 8 forwards each")
    ap.add_argument("--summarize-pool", metavar="DB", help="summarise the rocprofv3 database of a --trace-pool run")
    ap.add_argument("--norm", action="store_true", help="the 20x256 net with GroupNorm(32)-ReLU on the general path")
    ap.add_argument("--trace-norm", action="store_true", help="GroupNorm of 32, 256 and 1 groups, a 3x3 max pool and a depthwise 3x3 at B=512, C=256")
    ap.add_argument("--summarize-norm", metavar="DB", help="summarise the rocprofv3 database of a --trace-norm run")
    ap.add_argument("--mish", action="store_true", help="the 20x256 net with Mish, the same net with swish, and the forced family net")
    ap.add_argument("--gate", action="store_true", help="the 20x256 residual net with an scSE gate per block, beside the SE-swish net")
    ap.add_argument("--repeats", type=int, default=3, help="--mish, --smolgen: times each (net, batch) is timed")
    ap.add_argument("--smolgen", action="store_true", help="the transformer with a run-time attention bias per block, and without")
    ap.add_argument("--trace-smolgen", action="store_true", help="both at B=512, 13 forwards each")
    ap.add_argument("--summarize-smolgen", metavar="DB", help="graphAttention medians of a --trace-smolgen / --trace-attention run")
    ap.add_argument("--group", action="store_true", help="the ResNeXt-style 20x256 net (G = 8), its dense twin and the forced family net")
    ap.add_argument("--trace-group", action="store_true", help="the ResNeXt net and its twin at B = 1, 32, 128, 512, 8 forwards each")
    ap.add_argument("--summarize-group", metavar="DB", help="grouped against dense 3x3 launch medians of a --trace-group run")
    a = ap.parse_args()
    if a.summarize_group:
        summarize_group(a.summarize_group, a.out.replace("graph_bench.json", "group_bench.json"))
        return
    if a.summarize_smolgen:
        summarize_smolgen(a.summarize_smolgen)
        return
    if a.summarize_norm:
        summarize_norm(a.summarize_norm, a.out.replace("graph_bench.json", "norm_bench.json"))
        return
    if a.summarize_pool:
        summarize_pool(a.summarize_pool)
        return
    if a.summarize:
        summarize(a.summarize)
        return
    if a.summarize_attention:
        summarize_attention(a.summarize_attention)
        return
    nsg = importlib.import_module("nshogi-engine_amd")
    tmp = tempfile.mkdtemp()
    if a.trace_norm:
        jobs = [(label, (lambda p, g=g: groupnorm_onnx(p, g))) for label, g in NORM_TRACE]
        jobs += [("graphPool 3x3 max", maxpool3_onnx), ("graphDepthwise 3x3", depthwise3_onnx)]
        for i, (label, make) in enumerate(jobs):
            path = os.path.join(tmp, f"norm_trace_{i}.onnx")
            make(path)
            r, info = rate(nsg, path, TRACE_BATCH, iters=POOL_FAMILY_FORWARDS - 3, warmup=3)
            print(json.dumps({label: r, "launches": info["launches"]}), flush=True)
        return
    if a.group or a.trace_group:
        paths = {"resnext_20x256_g8_general": os.path.join(tmp, "resnext_g8.onnx"), "resnext_20x256_g1_general": os.path.join(tmp, "resnext_g1.onnx")}
        group_onnx(paths["resnext_20x256_g8_general"], 8)
        group_onnx(paths["resnext_20x256_g1_general"], 1)
        if a.trace_group:
            for k, path in paths.items():
                for b in GROUP_BATCHES:
                    r, info = rate(nsg, path, b, iters=GROUP_FORWARDS - 3, warmup=3)
                    print(json.dumps({k: r, "batch": b, "launches": info["launches"]}), flush=True)
            return
        paths["family_20x256_general"] = os.path.join(tmp, "family.onnx")
        family_onnx(nsg, paths["family_20x256_general"])
        rows = {k: {} for k in paths}
        batches = GROUP_BATCHES if a.batches == "1,64,512" else [int(b) for b in a.batches.split(",")]
        for b in batches:
            for rep in range(a.repeats):  # the nets in turn, so that drift of the clock falls on all of them
                for k, path in paths.items():
                    r, info = rate(nsg, path, b, force=k.startswith("family"), iters=20 if b >= 128 else 50)
                    rows[k].setdefault(str(b), []).append(round(r, 1))
                    rows[k].update(path=info["path"], launches=info["launches"], conv_launches=info["conv_launches"],
                                   flops_per_position=info["flops_per_position"])
        for k, row in rows.items():
            print(k, json.dumps(row), flush=True)
        out = a.out.replace("graph_bench.json", "group_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        doc = {}
        if os.path.exists(out):
            with open(out) as f:
                doc = json.load(f)
        doc.update(repeats=a.repeats, rows=rows)
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
        return
    if a.smolgen or a.trace_smolgen:
        paths = {"smolgen_8x256_general": os.path.join(tmp, "smolgen.onnx"), "attention_8x256_general": os.path.join(tmp, "att.onnx")}
        smolgen_onnx(paths["smolgen_8x256_general"])
        attention_onnx(paths["attention_8x256_general"])
        if a.trace_smolgen:
            for k, path in paths.items():
                r, info = rate(nsg, path, TRACE_BATCH, iters=10, warmup=3)
                print(json.dumps({k: r, "launches": info["launches"]}), flush=True)
            return
        rows = {k: {} for k in paths}
        for b in [int(b) for b in a.batches.split(",")]:
            for rep in range(a.repeats):
                for k, path in paths.items():
                    r, info = rate(nsg, path, b, iters=20 if b >= 256 else 50)
                    rows[k].setdefault(str(b), []).append(round(r, 1))
                    rows[k].update(path=info["path"], launches=info["launches"], attention_launches=info["attention_launches"],
                                   flops_per_position=info["flops_per_position"])
        for k, row in rows.items():
            print(k, json.dumps(row), flush=True)
        out = a.out.replace("graph_bench.json", "smolgen_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump({"repeats": a.repeats, "rows": rows}, f, indent=1)
        return
    if a.gate:
        paths = {k: os.path.join(tmp, k + ".onnx") for k in ("scse_20x256_general", "se_swish_20x256_general")}
        gate_onnx(paths["scse_20x256_general"])
        se_onnx(paths["se_swish_20x256_general"])
        rows = {k: {} for k in paths}
        for b in [int(b) for b in a.batches.split(",")]:
            for rep in range(a.repeats):  # the nets in turn, so that drift of the clock falls on both
                for k, path in paths.items():
                    r, info = rate(nsg, path, b, iters=20 if b >= 256 else 50)
                    rows[k].setdefault(str(b), []).append(round(r, 1))
                    rows[k].update(path=info["path"], launches=info["launches"], conv_launches=info["conv_launches"],
                                   flops_per_position=info["flops_per_position"])
        for k, row in rows.items():
            print(k, json.dumps(row), flush=True)
        out = a.out.replace("graph_bench.json", "gate_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump({"repeats": a.repeats, "rows": rows}, f, indent=1)
        return
    if a.mish:
        paths = {k: os.path.join(tmp, k + ".onnx") for k in ("mish_20x256_general", "swish_20x256_general", "family_20x256_general")}
        mish_onnx(paths["mish_20x256_general"])
        mish_onnx(paths["swish_20x256_general"], swish=True)
        family_onnx(nsg, paths["family_20x256_general"])
        rows = {k: {} for k in paths}
        for b in [int(b) for b in a.batches.split(",")]:
            for rep in range(a.repeats):  # the nets in turn, so that drift of the clock falls on all of them
                for k, path in paths.items():
                    r, info = rate(nsg, path, b, force=k.startswith("family"), iters=20 if b >= 256 else 50)
                    rows[k].setdefault(str(b), []).append(round(r, 1))
                    rows[k].update(path=info["path"], launches=info["launches"], conv_launches=info["conv_launches"])
        for k, row in rows.items():
            print(k, json.dumps(row), flush=True)
        out = a.out.replace("graph_bench.json", "mish_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump({"repeats": a.repeats, "rows": rows}, f, indent=1)
        return
    if a.norm:
        nm = os.path.join(tmp, "norm_20x256.onnx")
        norm_onnx(nm)
        row = {}
        for b in [int(b) for b in a.batches.split(",")]:
            r, info = rate(nsg, nm, b, iters=20 if b >= 256 else 50)
            row[str(b)] = round(r, 1)
            row.update(path=info["path"], launches=info["launches"], flops_per_position=info["flops_per_position"])
        print("groupnorm_20x256_general", json.dumps(row), flush=True)
        out = a.out.replace("graph_bench.json", "norm_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        doc = {}
        if os.path.exists(out):
            with open(out) as f:
                doc = json.load(f)
        doc["rows"] = {"groupnorm_20x256_general": row}
        with open(out, "w") as f:
            json.dump(doc, f, indent=1)
        return
    if a.pool or a.trace_pool:
        pl = os.path.join(tmp, "pool_20x256.onnx")
        pool_onnx(pl)
        if a.trace_pool:
            dw3, fam = os.path.join(tmp, "depthwise3_256.onnx"), os.path.join(tmp, "family_20x256.onnx")
            depthwise3_onnx(dw3)
            family_onnx(nsg, fam)
            for label, path, force in (("pool", pl, False), ("depthwise3", dw3, False), ("family", fam, True)):
                r, info = rate(nsg, path, TRACE_BATCH, force=force, iters=POOL_FAMILY_FORWARDS - 3, warmup=3)
                print(json.dumps({label + "_trace_evals_per_s": r, "launches": info["launches"]}), flush=True)
            return
        row = {}
        for b in [int(b) for b in a.batches.split(",")]:
            r, info = rate(nsg, pl, b, iters=20 if b >= 256 else 50)
            row[str(b)] = round(r, 1)
            row.update(path=info["path"], launches=info["launches"], flops_per_position=info["flops_per_position"])
        print("pool_20x256_general", json.dumps(row), flush=True)
        out = a.out.replace("graph_bench.json", "pool_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump({"rows": {"pool_20x256_general": row}}, f, indent=1)
        return
    if a.attention or a.trace_attention:
        att = os.path.join(tmp, "attention_8x256.onnx")
        attention_onnx(att)
        if a.trace_attention:
            r, info = rate(nsg, att, TRACE_BATCH, iters=10, warmup=3)
            print(json.dumps({"trace_evals_per_s": r, "flops_per_position": info["flops_per_position"]}))
            return
        row = {}
        for b in [int(b) for b in a.batches.split(",")]:
            r, info = rate(nsg, att, b, iters=20 if b >= 256 else 50)
            row[str(b)] = round(r, 1)
            row.update(path=info["path"], launches=info["launches"], attention_launches=info["attention_launches"],
                       flops_per_position=info["flops_per_position"])
        print("attention_8x256_general", json.dumps(row), flush=True)
        out = a.out.replace("graph_bench.json", "attention_bench.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump({"rows": {"attention_8x256_general": row}}, f, indent=1)
        return
    fam = os.path.join(tmp, "family_20x256.onnx")
    family_onnx(nsg, fam)
    if a.trace:
        r, info = rate(nsg, fam, TRACE_BATCH, force=True, iters=TRACE_FORWARDS - 3, warmup=3)
        print(json.dumps({"trace_evals_per_s": r, "conv_flops_per_position": info["flops_per_position"]}))
        geo = os.path.join(tmp, "geometry_20x256.onnx")
        geometry_onnx(geo)
        r, info = rate(nsg, geo, TRACE_BATCH, iters=GEOM_FORWARDS - 3, warmup=3)
        print(json.dumps({"geometry_trace_evals_per_s": r, "flops_per_position": info["flops_per_position"]}))
        return
    se = os.path.join(tmp, "se_20x256.onnx")
    se_onnx(se)
    geo = os.path.join(tmp, "geometry_20x256.onnx")
    geometry_onnx(geo)
    res = {"batches": [int(b) for b in a.batches.split(",")], "rows": {}}
    for label, path, prec, force in (("family_20x256_general", fam, "fp32", True),
                                     ("family_20x256_specialised_fp32", fam, "fp32", False),
                                     ("family_20x256_specialised_f16m6", fam, "f16m6", False),
                                     ("se_swish_20x256_general", se, "fp32", False),
                                     ("geometry_20x256_general", geo, "fp32", False)):
        row = {}
        for b in res["batches"]:
            r, info = rate(nsg, path, b, prec, force, iters=20 if b >= 256 else 50)
            row[str(b)] = round(r, 1)
            row["path"] = info["path"]
            row["launches"] = info["launches"]
            row["flops_per_position"] = info["flops_per_position"]
        res["rows"][label] = row
        print(label, json.dumps(row), flush=True)
    ev = nsg.Evaluator(0, 512, 86)
    t0 = time.perf_counter()
    ev.load(se)
    res["se_load_seconds"] = round(time.perf_counter() - t0, 3)
    ev.close()
    print("se load seconds", res["se_load_seconds"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
