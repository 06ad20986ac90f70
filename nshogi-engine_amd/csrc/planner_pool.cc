// planner_pool.cc -- the planner: pooling and the reductions over the board.
#include "planner.h"

namespace nsg::graph {

// ---- MaxPool / AveragePool that keep the board: one kLaunchPool.  A MaxPool whose window is the whole board (what the
// exporter writes for adaptive_max_pool2d(x, 1)) is the global max: one kLaunchMax.
void Planner::pool(const Node& N) {
    const Val& X = get(N, 0);
    const bool Max = N.Op == "MaxPool";
    if (X.form != kFormPlain || X.flatOfSpatial || !isSpatialDims(X.dims))
        fail(N, "input " + dimsStr(X.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)X.v.C * 81} : X.dims) +
                    " is not [N,C,9,9]: pooling runs on a spatial tensor only");
    const int C = (int)X.dims[1];
    const std::vector<int64_t> Ks = N.attrInts("kernel_shape", {});
    if (Ks.size() != 2) fail(N, "a kernel_shape of two sizes expected");
    const std::string KStr = std::to_string(Ks[0]) + "x" + std::to_string(Ks[1]);
    if (N.Out.size() > 1 && !N.Out[1].empty() && Uses.count(N.Out[1]))
        fail(N, "the Indices output '" + N.Out[1] + "' is used: only the pooled values are computed");
    const std::vector<int64_t> Dil = N.attrInts("dilations", {1, 1});
    if (Dil.size() != 2 || Dil[0] < 1 || Dil[1] < 1) fail(N, "two dilations of at least 1 expected");
    const std::vector<int64_t> Pads = N.attrInts("pads", {0, 0, 0, 0});
    const bool Ceil = N.attrI("ceil_mode", 0) != 0, AutoPad = N.Attrs.count("auto_pad") != 0;
    Launch L;
    L.name = N.Name;
    if (Max && Ks == std::vector<int64_t>{9, 9} && Pads == std::vector<int64_t>{0, 0, 0, 0} && Dil == std::vector<int64_t>{1, 1} &&
        !Ceil && !AutoPad) { // one window: the strides do not matter
        L.args = SquareReduceArgs{ready(N.In[0]).v, true};
        L.out = freshView(C, false);
        Val V = runtimeVal(N, {kBatch, C, 1, 1});
        V.v = L.out;
        emit(L);
        Vals[N.Out[0]] = V;
        return;
    }
    // a window that is exactly one rank or one file, unpadded (what the exporter writes for adaptive_*_pool2d(x, (9, 1))
    // and (1, 9)): the output is [N,C,9,1] or [N,C,1,9], a line tensor.  The stride along the window does not matter.
    {
        const bool Rank = Ks == std::vector<int64_t>{1, 9}, File = Ks == std::vector<int64_t>{9, 1};
        const std::vector<int64_t> St = N.attrInts("strides", {1, 1});
        if ((Rank || File) && Pads == std::vector<int64_t>{0, 0, 0, 0} && Dil == std::vector<int64_t>{1, 1} && !Ceil && !AutoPad &&
            St.size() == 2 && St[Rank ? 0 : 1] == 1 && St[Rank ? 1 : 0] >= 1)
            return linePool(N, File, Max);
    }
    for (int64_t S : N.attrInts("strides", {1, 1}))
        if (S != 1) fail(N, "stride " + std::to_string(S) + ": only stride 1 (the output stays 9x9)");
    if (Ks[0] < 1 || Ks[1] < 1 || Ks[0] > 9 || Ks[1] > 9 || Ks[0] % 2 == 0 || Ks[1] % 2 == 0)
        fail(N, "a " + KStr + " kernel: only odd kernel sizes from 1 to 9 each way");
    if (Ceil) fail(N, "ceil_mode 1: only ceil_mode 0");
    const int KH = (int)Ks[0], KW = (int)Ks[1];
    const int DH = KH == 1 ? 1 : (int)std::min<int64_t>(Dil[0], 64), DW = KW == 1 ? 1 : (int)std::min<int64_t>(Dil[1], 64);
    const int Hy = DH * (KH - 1) / 2, Hx = DW * (KW - 1) / 2;
    if (Hy > kMaxConvHalo || Hx > kMaxConvHalo)
        fail(N, "a " + KStr + " kernel at dilation " + std::to_string(Dil[0]) + "x" + std::to_string(Dil[1]) + " reaches " +
                    std::to_string(std::max(Hy, Hx)) + " squares past the edge: the halo is at most " + std::to_string(kMaxConvHalo));
    if (AutoPad) fail(N, "auto_pad: only explicit pads");
    if (Pads != std::vector<int64_t>{Hy, Hx, Hy, Hx}) {
        std::string Ps;
        for (int64_t P1 : Pads) Ps += (Ps.empty() ? "" : ",") + std::to_string(P1);
        fail(N, "pads [" + Ps + "] do not keep the 9x9 board: a " + KStr + " kernel at dilation " + std::to_string(DH) + "x" +
                    std::to_string(DW) + " needs [" + std::to_string(Hy) + "," + std::to_string(Hx) + "," + std::to_string(Hy) + "," + std::to_string(Hx) + "]");
    }
    const int Mode = Max ? kPoolMax : N.attrI("count_include_pad", 0) != 0 ? kPoolAvgInclude : kPoolAvgExclude;
    // a view at any channel offset: the kernel reads an unaligned one with scalar loads
    L.args = PoolArgs{ready(N.In[0]).v, KH, KW, DH, DW, Mode};
    L.out = freshView(C, true);
    Val V = runtimeVal(N, X.dims);
    V.v = L.out;
    emit(L);
    Vals[N.Out[0]] = V;
}

// ---- GlobalAveragePool / ReduceMean / GlobalMaxPool / ReduceMax over the squares: one kLaunchMean or kLaunchMax
void Planner::reduceSquares(const Node& N) {
    const std::string& Op = N.Op;
    const Val& X = get(N, 0);
    const bool Reduce = Op == "ReduceMean" || Op == "ReduceMax";
    const bool Tok = X.form == kFormToken && Reduce;
    if (!Tok && (X.flatOfSpatial || !isSpatialDims(X.dims))) fail(N, "input " + dimsStr(X.dims) + " is not [N,C,9,9]");
    bool Keep = true;
    if (Reduce) {
        std::vector<int64_t> Axes = axes(N, Tok ? 3 : 4);
        std::sort(Axes.begin(), Axes.end());
        // along one board axis: over the files (axis 3) one value per rank, over the ranks (axis 2) one per file
        if (!Tok && (Axes == std::vector<int64_t>{2} || Axes == std::vector<int64_t>{3})) {
            if (N.attrI("keepdims", 1) == 0)
                fail(N, Op + " over axis " + std::to_string(Axes[0]) + " of " + dimsStr(X.dims) + " with keepdims = 0: [N,C,9] is ambiguous with the other 3-D shapes; rank and file pooling keeps the axis (keepdims = 1)");
            return linePool(N, Axes[0] == 2, Op == "ReduceMax");
        }
        if (Tok ? Axes != std::vector<int64_t>{1} : Axes != std::vector<int64_t>{2, 3})
            fail(N, Op + " over the squares only: axes {2,3} of [N,C,9,9], axis 1 of a token tensor");
        Keep = N.attrI("keepdims", 1) != 0;
        if (Tok && Keep) fail(N, Op + " of a token tensor with keepdims = 0 only");
    }
    const int C = Tok ? (int)X.dims[2] : (int)X.dims[1];
    Launch L;
    L.name = N.Name;
    L.args = SquareReduceArgs{ready(N.In[0]).v, Op == "GlobalMaxPool" || Op == "ReduceMax"};
    L.out = freshView(C, false);
    Val V = runtimeVal(N, Keep ? std::vector<int64_t>{kBatch, C, 1, 1} : std::vector<int64_t>{kBatch, C});
    V.v = L.out;
    emit(L);
    Vals[N.Out[0]] = V;
}

// ---- ReduceMax / ReduceMin / ReduceSum / ReduceL1 / ReduceL2 / ReduceSumSquare / ReduceLogSumExp (and ReduceMean on token
// and flat rows) over the channels: one kLaunchChanReduce
// Which kind of tensor X is when the node's axes are exactly its channel axis: 1 spatial (axis 1 of [N,C,9,9]), 2 token
// (axis 2 of [N,81,C]), 3 flat (axis 1 of [N,C] / [N,C,1,1]); 0 otherwise.
int Planner::channelAxis(const Node& N, const Val& X) {
    if (!X.runtime || X.flatOfSpatial || (X.form != kFormPlain && X.form != kFormToken)) return 0;
    if (has(N, 1) && Vals.count(N.In[1]) && Vals.at(N.In[1]).runtime) return 0;
    const std::vector<int64_t> Axes = axes(N, X.dims.size());
    if (Axes.size() != 1) return 0;
    if (X.form == kFormToken) return Axes[0] == 2 ? 2 : 0;
    if (isSpatialDims(X.dims)) return Axes[0] == 1 ? 1 : 0;
    return flatC(X.dims) > 0 && X.dims.size() >= 2 && Axes[0] == 1 ? 3 : 0;
}

void Planner::reduceChannels(const Node& N) {
    const std::string& Op = N.Op;
    const Val& X = get(N, 0);
    const std::vector<int64_t> XD = X.runtime && X.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)X.v.C * 81} : X.dims;
    const int Kind = channelAxis(N, X);
    if (!Kind)
        fail(N, Op + " of " + dimsStr(XD) + ": a " + Op + " runs over the channels only, with keepdims = 1: axis 1 of [N,C,9,9] -> [N,1,9,9], "
                "the last axis of a token tensor [N,81,C] -> [N,81,1], axis 1 of a flat [N,C] -> [N,1]");
    const bool Keep = N.attrI("keepdims", 1) != 0;
    if (!Keep)
        fail(N, Op + " over axis " + std::to_string(Kind == 2 ? 2 : 1) + " of " + dimsStr(XD) + " with keepdims = 0: " +
                    (Kind == 1 ? "[N,9,9] is ambiguous with the other 3-D shapes" : Kind == 2 ? "[N,81] is ambiguous with the other 2-D shapes"
                                                                                               : "the result is the one-channel tensor [N,1]") +
                    "; a reduction over the channels keeps the axis (keepdims = 1)");
    const int C = Kind == 2 ? (int)XD[2] : (int)XD[1];
    Launch L;
    L.name = N.Name;
    ChanReduceArgs& A = L.args.emplace<ChanReduceArgs>();
    A.redMode = Op == "ReduceMax" ? kRedMax : Op == "ReduceMin" ? kRedMin : Op == "ReduceL1" ? kRedL1 : Op == "ReduceL2" ? kRedL2
                : Op == "ReduceSumSquare" ? kRedSumSq : Op == "ReduceLogSumExp" ? kRedLogSumExp : kRedSum;
    A.scale = Op == "ReduceMean" ? (float)(1.0 / C) : 1.f; // the mean: the sum times the f32 constant 1/C, applied after the last add
    A.in = ready(N.In[0]).v; // a view at any channel offset: the kernel reads the ragged ends with scalar loads
    L.out = freshView(1, Kind != 3);
    if (A.redMode == kRedSum) P.flopsPerPosition += (double)C * (Kind == 3 ? 1 : 81);
    std::vector<int64_t> OD = XD;
    OD[Kind == 2 ? 2 : 1] = 1;
    Val V = runtimeVal(N, OD, Kind == 2 ? kFormToken : kFormPlain);
    V.v = L.out;
    emit(L);
    Vals[N.Out[0]] = V;
}

} // namespace nsg::graph
