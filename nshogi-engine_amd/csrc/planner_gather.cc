// planner_gather.cc -- the planner: Gather of a run-time tensor with constant indices, and board flips (a Slice with
// step -1 over a whole board axis), as one kLaunchGather ("indexing").
#include "planner.h"

#include <cstring>

namespace nsg::graph {

// One kLaunchGather: output element (r, c) of a board is src[board * Block + RowTab[r] + ColTab[c]].  Every entry is
// checked here, which is what keeps the kernel's reads inside the source board's own block: the device checks nothing.
View Planner::gatherLaunch(const Node& N, const View& In, long Block, const std::vector<int>& RowTab,
                           const std::vector<int>& ColTab, bool Spatial) {
    Launch L;
    L.name = N.Name;
    GatherArgs& A = L.args.emplace<GatherArgs>();
    A.in = In;
    L.out = freshView((int)ColTab.size(), Spatial);
    A.gatherRows = (int)RowTab.size();
    A.gatherBlock = Block;
    const int RowMin = *std::min_element(RowTab.begin(), RowTab.end()), RowMax = *std::max_element(RowTab.begin(), RowTab.end());
    const int ColMin = *std::min_element(ColTab.begin(), ColTab.end()), ColMax = *std::max_element(ColTab.begin(), ColTab.end());
    if (A.gatherRows != (Spatial ? 81 : 1) || RowMin < 0 || ColMin < 0 || (long)RowMax + (long)ColMax >= Block)
        fail(N, "internal planner error: a gather table reaches outside its board's block");
    // rowTab[gatherRows], then colTab[out.stride] with pad entries 0, each 16-byte aligned, bit for bit in the float blob
    const size_t RowInts = (size_t)roundUp(A.gatherRows, 4);
    std::vector<int32_t> Tab(RowInts + (size_t)L.out.stride, 0);
    std::copy(RowTab.begin(), RowTab.end(), Tab.begin());
    std::copy(ColTab.begin(), ColTab.end(), Tab.begin() + (long)RowInts);
    std::vector<float> Tb(Tab.size());
    std::memcpy(Tb.data(), Tab.data(), Tab.size() * sizeof(int32_t));
    A.gatherTabOff = addConst(Tb);
    const View Out = L.out;
    emit(L);
    return Out;
}

// ---- Gather of a run-time tensor along one axis with a constant scalar or 1-D index list
void Planner::gather(const Node& N) {
    const Val& X0 = get(N, 0);
    const Val& Iv = get(N, 1);
    const std::vector<int64_t> XD = !X0.runtime ? X0.dims : X0.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)X0.v.C * 81} : X0.dims;
    const std::string Shapes = "data " + dimsStr(XD) + ", indices " + dimsStr(Iv.dims) + ", axis " + std::to_string(N.attrI("axis", 0)) + ": ";
    if (Iv.runtime || !X0.runtime)
        fail(N, Shapes + "the indices are computed at run time; a Gather takes constant indices");
    const int64_t Rank = (int64_t)XD.size();
    int64_t Axis = N.attrI("axis", 0);
    if (Axis < 0) Axis += Rank;
    if (Iv.dims.size() >= 2)
        fail(N, Shapes + "indices of rank " + std::to_string(Iv.dims.size()) + "; a Gather takes a scalar or a 1-D list");
    const bool Scalar = Iv.dims.empty();
    std::vector<int64_t> Idx = ints(N, 1, "Gather's indices");
    const int64_t M = (int64_t)Idx.size();
    if (M < 1 || (Scalar && M != 1)) fail(N, Shapes + "an empty index list");
    if (Axis == 0) fail(N, Shapes + "axis 0 is the batch; a Gather selects along the channels or the squares of a board");
    if (Axis < 0 || Axis >= Rank) fail(N, Shapes + "the axis is outside the data's rank");

    const bool Token = X0.form == kFormToken;
    const bool Spatial = !Token && !X0.flatOfSpatial && isSpatialDims(X0.dims);
    const bool FlatView = !Token && X0.flatOfSpatial;
    if (!Token && !Spatial && !FlatView && flatC(X0.dims) < 0) fail(N, Shapes + "the data is neither [N,C,9,9], a token tensor [N,81,C] nor flat");
    if (Spatial && Axis >= 2)
        fail(N, Shapes + "axis " + std::to_string(Axis) + " of a spatial tensor is a board axis; a Gather selects channels (axis 1), and x.flip(2) / x.flip(3) mirror the board");
    if (Spatial && Scalar)
        fail(N, Shapes + "a scalar index on axis 1 of a spatial tensor gives [N,9,9], which is not a tensor kind; write x[:, c:c+1]");
    if (!Token && !Spatial && !FlatView && Axis != 1)
        fail(N, Shapes + "axis " + std::to_string(Axis) + " of a flat tensor has one element; a Gather selects along axis 1");
    const int64_t Dim = XD[(size_t)Axis];
    for (int64_t& I : Idx) {
        if (I < -Dim || I >= Dim)
            fail(N, Shapes + "index " + std::to_string(I) + " is outside [" + std::to_string(-Dim) + "," + std::to_string(Dim) + ") of an axis of extent " + std::to_string(Dim));
        if (I < 0) I += Dim;
    }
    if (Token && Axis == 1 && !Scalar && M != 81)
        fail(N, Shapes + "a list of " + std::to_string(M) + " squares; an index list along the squares of a token tensor re-orders all 81 (a token tensor has 81 rows)");

    const View In = ready(N.In[0]).v; // an open elementwise group that computes the source is emitted first
    const int St = In.stride, Off = In.offset;
    std::vector<int> Row, Col;
    std::vector<int64_t> OD;
    int OutForm = kFormPlain;
    long Block = 81L * St;
    if (Spatial || (Token && Axis == 2 && !Scalar)) { // channels by a list: [N,M,9,9] or [N,81,M]
        for (int R = 0; R < 81; ++R) Row.push_back(R * St);
        for (int64_t I : Idx) Col.push_back(Off + (int)I);
        OD = Token ? std::vector<int64_t>{kBatch, 81, M} : std::vector<int64_t>{kBatch, M, 9, 9};
        OutForm = Token ? kFormToken : kFormPlain;
    } else if (Token && Axis == 2) { // tok[:, :, c]: one value per square, flat [N,81]
        Row = {0};
        for (int J = 0; J < 81; ++J) Col.push_back(J * St + Off + (int)Idx[0]);
        OD = {kBatch, 81};
    } else if (Token && Scalar) { // tok[:, s]: one square's token, flat [N,C]
        Row = {(int)Idx[0] * St};
        for (int C = 0; C < In.C; ++C) Col.push_back(Off + C);
        OD = {kBatch, In.C};
    } else if (Token) { // the squares re-ordered or repeated
        for (int64_t I : Idx) Row.push_back((int)I * St);
        for (int C = 0; C < In.C; ++C) Col.push_back(Off + C);
        OD = X0.dims;
        OutForm = kFormToken;
    } else if (FlatView) { // the flattened view [N,C*81] read where its spatial rows lie: index i is channel i / 81 of square i % 81
        Row = {0};
        for (int64_t I : Idx) Col.push_back((int)(I % 81) * St + Off + (int)(I / 81));
        OD = Scalar ? std::vector<int64_t>{kBatch} : std::vector<int64_t>{kBatch, M};
    } else { // a flat row
        OD = X0.dims;
        if (Scalar) { // a view, no launch
            OD.erase(OD.begin() + 1);
            Val V = runtimeVal(N, OD);
            V.v = In;
            V.v.offset = Off + (int)Idx[0];
            V.v.C = 1;
            Vals[N.Out[0]] = V;
            return;
        }
        OD[1] = M;
        Row = {0};
        for (int64_t I : Idx) Col.push_back(Off + (int)I);
        Block = St;
    }
    Val V = runtimeVal(N, OD, OutForm);
    V.v = gatherLaunch(N, In, Block, Row, Col, Row.size() == 81);
    Vals[N.Out[0]] = V;
}

// ---- x.flip(2), x.flip(3) or both: the squares of a spatial view re-ordered (called by slice())
void Planner::flipBoard(const Node& N, Val V, bool Ranks, bool Files) {
    std::vector<int> Row, Col;
    for (int R = 0; R < 81; ++R) {
        const int Y = Ranks ? 8 - R / 9 : R / 9, X = Files ? 8 - R % 9 : R % 9;
        Row.push_back((Y * 9 + X) * V.v.stride);
    }
    for (int C = 0; C < V.v.C; ++C) Col.push_back(V.v.offset + C);
    V.v = gatherLaunch(N, V.v, 81L * V.v.stride, Row, Col, true);
    Vals[N.Out[0]] = V;
}

} // namespace nsg::graph
