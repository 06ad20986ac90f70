// planner_lines.cc -- the planner: rank and file pooling and the line tensors behind it (DESIGN.md sections 13.3, 13.7).
// A line tensor ([N,C,9,1] rank lines, [N,C,1,9] file lines, [N,C,18,1]) exists only between the pooling that makes it
// and the broadcast back onto the board; what reads it is listed in lineOp, everything else is refused there.
#include "planner.h"

namespace nsg::graph {

// ---- ReduceMean / ReduceMax over one board axis, AveragePool / MaxPool of a 1x9 or 9x1 window: one kLaunchLinePool
void Planner::linePool(const Node& N, bool Files, bool Max) {
    const Val& X = get(N, 0);
    const int C = (int)X.dims[1];
    Launch L;
    L.name = N.Name;
    const View In = ready(N.In[0]).v; // a view at any channel offset, read where it lies
    L.args = LinePoolArgs{In, Files, Max ? kPoolMax : kPoolAvgInclude};
    L.out = freshLines(C, 9);
    Val V;
    V.runtime = true;
    V.dims = Files ? std::vector<int64_t>{kBatch, C, 1, 9} : std::vector<int64_t>{kBatch, C, 9, 1};
    V.form = kFormLine;
    V.producer = N.Name;
    V.v = L.out;
    V.lineLaunch = (int)P.launches.size();
    emit(L);
    Vals[N.Out[0]] = V;
}

// a line view as contiguous rows at offset 0 of a buffer of its own (the input of a conv): itself, or a copy
View Planner::linePlain(const std::string& Name, const std::string& Why) {
    const View V0 = ready(Name).v;
    if (V0.offset == 0 && V0.stride == roundUp(V0.C, kChunk) && V0.line0 == 0 && V0.bufLines == V0.lines) return V0;
    const View Out = freshLines(V0.C, V0.lines);
    EltSrc S;
    S.v = V0;
    S.mode = V0.line0 != 0 || V0.bufLines != V0.lines ? kSrcLine : kSrcSame;
    emit(Launch{Why, Out, EltProgram{{S}, {EltInstr{(uint8_t)kEltLoad, 0, 0, 0}}, 0}});
    Val& V = Vals[Name];
    V.v = Out;
    V.lineLaunch = -1;
    return Out;
}

// ---- a 1x1 Conv on a line tensor: the dense form of graphConv<1> over N * L rows, as headRowsDense runs it
void Planner::lineConv(const Node& N, size_t Index) {
    const Val X = get(N, 0);
    const int Ln = X.v.lines;
    const Val& Wt = host(N, 1, "the weight");
    if (Wt.isInt || Wt.dims.size() != 4) fail(N, "expected a 4-D float weight [Cout,Cin/group,kh,kw]");
    if (Wt.dims[2] != 1 || Wt.dims[3] != 1)
        fail(N, "a " + std::to_string(Wt.dims[2]) + "x" + std::to_string(Wt.dims[3]) + " kernel on the line tensor " + dimsStr(X.dims) +
                    ": only a 1x1 conv reads a line tensor (its rows are lines, not squares with neighbours)");
    if (N.attrI("group", 1) != 1) fail(N, "group " + std::to_string(N.attrI("group", 1)) + " on the line tensor " + dimsStr(X.dims) + ": only group 1");
    for (int64_t S : N.attrInts("strides", {1, 1}))
        if (S != 1) fail(N, "stride " + std::to_string(S) + " on the line tensor " + dimsStr(X.dims) + ": only stride 1");
    for (int64_t Pd : N.attrInts("pads", {0, 0, 0, 0}))
        if (Pd != 0) fail(N, "pads on the line tensor " + dimsStr(X.dims) + ": a 1x1 conv takes none");
    if (N.Attrs.count("auto_pad")) fail(N, "auto_pad: only explicit pads");
    LinearW Lw;
    Lw.Cout = (int)Wt.dims[0];
    Lw.Cin = Lw.CinW = (int)Wt.dims[1];
    if ((int)X.dims[1] != Lw.Cin)
        fail(N, "the weight expects " + std::to_string(Lw.Cin) + " input channels, '" + N.In[0] + "' has " + std::to_string(X.dims[1]));
    if (Wt.f.size() != (size_t)Lw.Cout * Lw.Cin) fail(N, "the weight's data does not match its shape");
    Lw.W.assign(Wt.f.begin(), Wt.f.end());
    Lw.Bias.assign((size_t)Lw.Cout, 0.0);
    if (has(N, 2)) {
        const Val& B = host(N, 2, "the bias");
        if ((int)B.count() != Lw.Cout) fail(N, "bias length does not match the output channels");
        for (int C = 0; C < Lw.Cout; ++C) Lw.Bias[(size_t)C] = B.at((size_t)C);
    }
    const int Cout = Lw.Cout;
    std::vector<int64_t> Dims = X.dims;
    Dims[1] = Cout;
    // BatchNorm, constant per-channel Adds and one activation; a residual is not absorbed (it stays an elementwise Add)
    const Epilogue E = foldEpilogue(N, Index, Dims, 1, -1, &Lw);
    Launch L;
    L.name = E.name;
    ConvArgs& A = L.args.emplace<ConvArgs>();
    A.dense = true;
    A.rowsPerBoard = Ln;
    A.taps = A.kh = A.kw = 1;
    A.in = linePlain(N.In[0], N.Name + " (input copy)");
    A.cinPad = roundUp(Lw.Cin, kChunk);
    A.coutTiles = (Cout + kCoutTile - 1) / kCoutTile;
    A.act = E.act;
    // packed [tile][chunk][1][16][64], bias [tiles * 64]
    const int Chunks = A.cinPad / kChunk;
    std::vector<float> Pk((size_t)A.coutTiles * Chunks * kChunk * kCoutTile, 0.f), Bf((size_t)A.coutTiles * kCoutTile, 0.f);
    for (int O = 0; O < Cout; ++O) {
        for (int I = 0; I < Lw.Cin; ++I)
            Pk[(((size_t)(O / kCoutTile) * Chunks + I / kChunk) * kChunk + I % kChunk) * kCoutTile + O % kCoutTile] = (float)Lw.W[(size_t)O * Lw.Cin + I];
        Bf[(size_t)O] = (float)Lw.Bias[(size_t)O];
    }
    A.wOff = addConst(Pk);
    A.biasOff = addConst(Bf);
    L.out = freshLines(Cout, Ln);
    P.flopsPerPosition += 2.0 * Ln * (double)Lw.Cin * Cout;
    Val V;
    V.runtime = true;
    V.dims = Dims;
    V.form = kFormLine;
    V.v = L.out;
    V.producer = N.Name;
    emit(L);
    Vals[E.out] = V;
}

// ---- every node that reads a line tensor -----------------------------------------------------------------------------
void Planner::lineOp(const Node& N, size_t Index) {
    const std::string& Op = N.Op;
    const Val& X = get(N, 0);
    const bool XLine = X.runtime && X.form == kFormLine;
    if (Op == "Conv" && XLine) return lineConv(N, Index);
    if (isAct(Op) || isBinary(Op) || isEltExtra(Op) || Op == "BatchNormalization" || Op == "Pow") return elementwise(N);
    if (Op == "Transpose" && XLine) { // [0,1,3,2] flips rank lines and file lines: the same rows
        const std::vector<int64_t> Perm = N.attrInts("perm", {});
        if (Perm != std::vector<int64_t>{0, 1, 3, 2} || X.v.lines != 9)
            fail(N, "Transpose of the line tensor " + dimsStr(X.dims) + " with perm " + dimsStr(Perm) + ": only [0,1,3,2] of nine lines, rank lines to file lines and back");
        const bool Move = X.group >= 0 && absorbable(N.In[0]);
        Val V = Move ? X : ready(N.In[0]);
        if (!absorbable(N.In[0])) V.lineLaunch = -1;
        V.dims = {kBatch, X.dims[1], X.dims[3], X.dims[2]};
        V.producer = N.Name;
        if (Move) Groups[(size_t)V.group].out = N.Out[0];
        Vals[N.Out[0]] = V;
        return;
    }
    if (Op == "Concat") {
        // 9 + 9 rank lines along axis 2: the two poolings write the halves of one 18-line block, no launch of its own
        int64_t Ax = N.attrI("axis", 1);
        if (Ax < 0) Ax += 4;
        std::string Shapes;
        bool Nine = N.In.size() == 2;
        for (size_t J = 0; J < N.In.size(); ++J) {
            const Val& V = get(N, J);
            const std::vector<int64_t> D = V.runtime && V.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)V.v.C * 81} : V.dims;
            Shapes += (J ? " and " : "") + dimsStr(D);
            Nine = Nine && V.runtime && V.form == kFormLine && D[2] == 9 && D[3] == 1 && D[1] == get(N, 0).dims[1];
        }
        if (Ax != 2 || !Nine)
            fail(N, "Concat of " + Shapes + " along axis " + std::to_string(N.attrI("axis", 1)) +
                        ": line tensors are joined as 9 + 9 rank lines [N,C,9,1] of the same channels along axis 2 only");
        int Lp[2];
        for (size_t J = 0; J < 2; ++J) {
            const Val& V = get(N, J);
            Lp[J] = V.lineLaunch;
            if (Lp[J] < 0 || !absorbable(N.In[J]) || (J == 1 && Lp[1] == Lp[0]))
                fail(N, "'" + N.In[J] + "' " + dimsStr(V.dims) + ": Concat joins the results of two rank / file poolings (ReduceMean, ReduceMax, a 1x9 or 9x1 pool, through Transpose [0,1,3,2]) that nothing else reads; they write the halves of the 18-line block themselves");
        }
        const int C = (int)X.dims[1];
        const View Block = freshLines(C, 18);
        for (int J = 0; J < 2; ++J) {
            Launch& Pl = P.launches[(size_t)Lp[J]];
            Pl.out.buf = Block.buf;
            Pl.out.bufLines = 18;
            Pl.out.line0 = 9 * J;
        }
        P.launches[(size_t)Lp[1]].name += "+" + N.Name;
        Val V;
        V.runtime = true;
        V.dims = {kBatch, C, 18, 1};
        V.form = kFormLine;
        V.producer = N.Name;
        V.v = Block;
        Vals[N.Out[0]] = V;
        return;
    }
    if ((Op == "Split" || Op == "Slice") && XLine) {
        // along axis 2 of an 18-line tensor, back into two 9-line views: no launch
        const Val Src = ready(N.In[0]);
        auto part = [&](const std::string& Out, int First) {
            Val V = Src;
            V.producer = N.Name;
            V.lineLaunch = -1;
            V.dims = {kBatch, Src.dims[1], 9, 1};
            V.v.lines = 9;
            V.v.line0 += First;
            Vals[Out] = V;
        };
        const std::string Only = Op + " of the line tensor " + dimsStr(Src.dims) + ": only 18 lines along axis 2, into 9 + 9";
        if (Src.v.lines != 18) fail(N, Only);
        if (Op == "Split") {
            int64_t Axis = N.attrI("axis", 0);
            if (Axis < 0) Axis += 4;
            std::vector<int64_t> Sizes = has(N, 1) ? ints(N, 1, "the split sizes") : N.attrInts("split", {});
            if (Sizes.empty() && N.Out.size() == 2) Sizes = {9, 9};
            if (Axis != 2 || Sizes != std::vector<int64_t>{9, 9} || N.Out.size() != 2) fail(N, Only);
            for (size_t J = 0; J < 2; ++J)
                if (!N.Out[J].empty()) part(N.Out[J], 9 * (int)J);
            return;
        }
        const std::vector<int64_t> St = ints(N, 1, "starts"), En = ints(N, 2, "ends");
        const std::vector<int64_t> Axes = has(N, 3) ? ints(N, 3, "axes") : std::vector<int64_t>();
        const std::vector<int64_t> Sp = has(N, 4) ? ints(N, 4, "steps") : std::vector<int64_t>{1};
        if (St.size() != 1 || En.size() != 1 || Axes.size() != 1 || (Axes[0] != 2 && Axes[0] != -2) || Sp != std::vector<int64_t>{1} ||
            !((St[0] == 0 && En[0] == 9) || (St[0] == 9 && En[0] >= 18)))
            fail(N, Only);
        part(N.Out[0], (int)St[0]);
        return;
    }
    for (size_t J = 0; J < N.In.size(); ++J) {
        if (N.In[J].empty()) continue;
        const Val& I = Vals.at(N.In[J]);
        if (I.runtime && I.form == kFormLine)
            fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " is a line tensor: only elementwise ops, a 1x1 Conv, Transpose [0,1,3,2], Concat and Split of 9 + 9 lines along axis 2 and the broadcast onto [N,C,9,9] read it (DESIGN.md section 13.3)");
    }
    fail(N, "internal planner error: no line tensor among the inputs");
}

} // namespace nsg::graph
