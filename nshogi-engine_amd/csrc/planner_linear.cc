// planner_linear.cc -- the planner: Conv / Gemm / MatMul with their epilogue.
#include "planner.h"

#include <cstring>

namespace nsg::graph {

// A Conv's weights, bias and geometry, checked against the input X
LinearW Planner::convWeights(const Node& N, const Val& X) {
    LinearW L;
    const Val& Wt = host(N, 1, "the weight");
    if (Wt.isInt || Wt.dims.size() != 4) fail(N, "expected a 4-D float weight [Cout,Cin/group,kh,kw]");
    const int64_t Kh64 = Wt.dims[2], Kw64 = Wt.dims[3];
    const std::string KStr = std::to_string(Kh64) + "x" + std::to_string(Kw64);
    for (int64_t S : N.attrInts("strides", {1, 1}))
        if (S != 1) fail(N, "stride " + std::to_string(S) + ": only stride 1 (the output stays 9x9)");
    if (Kh64 < 1 || Kw64 < 1 || Kh64 > 9 || Kw64 > 9 || Kh64 % 2 == 0 || Kw64 % 2 == 0)
        fail(N, "a " + KStr + " kernel: only odd kernel sizes from 1 to 9 each way");
    const std::vector<int64_t> Dil = N.attrInts("dilations", {1, 1});
    if (Dil.size() != 2 || Dil[0] < 1 || Dil[1] < 1) fail(N, "two dilations of at least 1 expected");
    L.KH = (int)Kh64;
    L.KW = (int)Kw64;
    L.DH = L.KH == 1 ? 1 : (int)std::min<int64_t>(Dil[0], 64); // a dilation along an axis of one tap means nothing
    L.DW = L.KW == 1 ? 1 : (int)std::min<int64_t>(Dil[1], 64);
    const int Hy = L.DH * (L.KH - 1) / 2, Hx = L.DW * (L.KW - 1) / 2;
    if (Hy > kMaxConvHalo || Hx > kMaxConvHalo)
        fail(N, "a " + KStr + " kernel at dilation " + std::to_string(Dil[0]) + "x" + std::to_string(Dil[1]) + " reaches " +
                    std::to_string(std::max(Hy, Hx)) + " squares past the edge: the halo is at most " + std::to_string(kMaxConvHalo));
    if (N.Attrs.count("auto_pad")) fail(N, "auto_pad: only explicit pads");
    const std::vector<int64_t> Pads = N.attrInts("pads", {0, 0, 0, 0});
    if (Pads != std::vector<int64_t>{Hy, Hx, Hy, Hx}) {
        std::string Ps;
        for (int64_t P1 : Pads) Ps += (Ps.empty() ? "" : ",") + std::to_string(P1);
        fail(N, "pads [" + Ps + "] do not keep the 9x9 board: a " + KStr + " kernel at dilation " + std::to_string(L.DH) + "x" +
                    std::to_string(L.DW) + " needs [" + std::to_string(Hy) + "," + std::to_string(Hx) + "," + std::to_string(Hy) + "," + std::to_string(Hx) + "]");
    }
    L.Cout = (int)Wt.dims[0];
    if (X.flatOfSpatial || !isSpatialDims(X.dims)) fail(N, "input " + dimsStr(X.dims) + " is not [N,C,9,9]");
    const int64_t Group = N.attrI("group", 1);
    if (Group == 1) {
        L.Cin = (int)Wt.dims[1];
    } else if (Group != X.dims[1]) {
        // a grouped conv: group divides Cin and Cout, weight [Cout,Cin/group,kh,kw], Cin/group a multiple of 4, so that
        // an MFMA k-step and a 16-byte staged piece never straddle two groups
        const int64_t XC = X.dims[1];
        const std::string GStr = "group " + std::to_string(Group) + " on " + std::to_string(XC) + " input channels";
        const std::string Or = " (or group 1, or a depthwise conv)";
        if (Group < 1 || XC % Group != 0)
            fail(N, GStr + ": the group count does not divide the input channels" + Or);
        if (L.Cout % Group != 0)
            fail(N, GStr + " and " + std::to_string(L.Cout) + " output channels: the group count does not divide the output channels" + Or);
        const int64_t Per = XC / Group;
        if (Wt.dims[1] != Per)
            fail(N, GStr + " with a weight of " + std::to_string(Wt.dims[1]) + " channels per group: a grouped weight is [Cout," + std::to_string(Per) + ",kh,kw]");
        if (Per % 4 != 0)
            fail(N, GStr + " is " + std::to_string(Per) + " per group: a grouped conv needs a multiple of 4 input channels per group" + Or);
        L.Groups = (int)Group;
        L.Cin = (int)XC;
    } else {
        // depthwise: group = Cin = Cout, weight [C,1,kh,kw]
        const int64_t XC = X.dims[1];
        if (Wt.dims[1] != 1) fail(N, "group " + std::to_string(Group) + " with a weight of " + std::to_string(Wt.dims[1]) + " channels per group: a depthwise weight is [C,1,kh,kw]");
        if (L.Cout != (int)XC)
            fail(N, "a depthwise conv with channel multiplier " + std::to_string(XC > 0 ? L.Cout / XC : 0) + " (" + std::to_string(XC) + " -> " +
                        std::to_string(L.Cout) + " channels): only multiplier 1");
        L.Depthwise = true;
        L.Cin = (int)XC;
    }
    if ((int)X.dims[1] != L.Cin)
        fail(N, "the weight expects " + std::to_string(L.Cin) + " input channels, '" + N.In[0] + "' has " + std::to_string(X.dims[1]));
    L.CinW = L.Depthwise ? 1 : L.Cin / L.Groups;
    if (Wt.f.size() != (size_t)L.Cout * L.CinW * L.KH * L.KW) fail(N, "the weight's data does not match its shape");
    L.W.assign(Wt.f.begin(), Wt.f.end());
    L.Bias.assign((size_t)L.Cout, 0.0);
    if (has(N, 2)) {
        const Val& B = host(N, 2, "the bias");
        if ((int)B.count() != L.Cout) fail(N, "bias length does not match the output channels");
        for (int C = 0; C < L.Cout; ++C) L.Bias[(size_t)C] = B.at((size_t)C);
    }
    return L;
}

// A Gemm's or MatMul's weights [Cout][Cin] and bias, checked against the input X (Tok: a token tensor)
LinearW Planner::denseWeights(const Node& N, const Val& X, bool Tok) {
    LinearW L;
    const Val& Wt = host(N, 1, "the weight");
    if (Wt.isInt || Wt.dims.size() != 2) fail(N, "expected a 2-D float weight");
    bool TransB = false;
    if (N.Op == "Gemm") {
        if (N.attrF("alpha", 1.0) != 1.0 || N.attrF("beta", 1.0) != 1.0 || N.attrI("transA", 0) != 0)
            fail(N, "Gemm with alpha = beta = 1, transA = 0 only");
        TransB = N.attrI("transB", 0) != 0;
    }
    const int Cout = L.Cout = (int)(TransB ? Wt.dims[0] : Wt.dims[1]);
    const int Cin = L.Cin = L.CinW = (int)(TransB ? Wt.dims[1] : Wt.dims[0]);
    const int XC = Tok ? (int)X.dims[2] : X.flatOfSpatial ? X.v.C * 81 : flatC(X.dims);
    if (X.dims.size() != 2 && !X.flatOfSpatial && !Tok) fail(N, "input " + dimsStr(X.dims) + " is not 2-D [N,K]");
    if (XC != Cin) fail(N, "the weight expects K = " + std::to_string(Cin) + ", '" + N.In[0] + "' has " + std::to_string(XC));
    L.W.assign((size_t)Cout * Cin, 0.0);
    for (int O = 0; O < Cout; ++O)
        for (int I = 0; I < Cin; ++I)
            L.W[(size_t)O * Cin + I] = TransB ? Wt.f[(size_t)O * Cin + I] : Wt.f[(size_t)I * Cout + O];
    L.Bias.assign((size_t)Cout, 0.0);
    if (N.Op == "Gemm" && has(N, 2)) {
        const Val& B = host(N, 2, "the bias");
        if ((int)B.count() != Cout && B.count() != 1) fail(N, "bias length does not match");
        for (int C = 0; C < Cout; ++C) L.Bias[(size_t)C] = B.at(B.count() == 1 ? 0 : (size_t)C);
    }
    return L;
}

// The epilogue behind node N, absorbed while each tensor has one consumer:
//   [BatchNorm | constant per-channel Add]*  [+ runtime residual]  [activation]
// BatchNorm and the constant Adds fold into Lw's weights and bias in double.
Planner::Epilogue Planner::foldEpilogue(const Node& N, size_t Index, const std::vector<int64_t>& Dims, int ChanAxis, int OutForm,
                                        LinearW* Lw) {
    const int Cout = Lw->Cout;
    const size_t PerOut = (size_t)Lw->CinW * Lw->taps();
    Epilogue E;
    E.name = N.Name;
    E.out = N.Out[0];
    std::string& Cur = E.out;
    size_t At = Index;
    while (absorbable(Cur)) {
        const Node* C = onlyConsumer(Cur, At);
        if (!C) break;
        if (C->Op == "BatchNormalization" && E.res.empty() && E.act == kActNone && C->In.size() >= 5 && C->In[0] == Cur) {
            bool Const = true;
            for (size_t S = 1; S < 5; ++S) Const = Const && Vals.count(C->In[S]) && !Vals.at(C->In[S]).runtime && Vals.at(C->In[S]).count() == (size_t)Cout;
            if (!Const) break;
            for (int O = 0; O < Cout; ++O) {
                const BnChannel B = bnChannel(*C, (size_t)O);
                for (size_t J = (size_t)O * PerOut; J < (size_t)(O + 1) * PerOut; ++J) Lw->W[J] *= B.scale;
                Lw->Bias[(size_t)O] = (Lw->Bias[(size_t)O] - B.mean) * B.scale + B.beta;
            }
        } else if (C->Op == "Add" && C->In.size() == 2) {
            const std::string& Other = C->In[0] == Cur ? C->In[1] : C->In[0];
            auto It = Vals.find(Other);
            if (It == Vals.end() || Other == Cur) break;
            const Val& O = It->second;
            if (!O.runtime) { // a per-channel constant: the bias
                if (!E.res.empty() || E.act != kActNone) break;
                std::vector<int64_t> BD;
                if (!broadcast(Dims, O.dims, &BD) || BD != Dims) break;
                const std::vector<int> Ax = variesAlong(O.dims, Dims.size());
                if (!(Ax.empty() || (Ax.size() == 1 && Ax[0] == ChanAxis))) break;
                for (int Ch = 0; Ch < Cout; ++Ch) Lw->Bias[(size_t)Ch] += O.at(Ax.empty() ? 0 : (size_t)Ch);
            } else {
                if (!E.res.empty() || E.act != kActNone || O.flatOfSpatial || O.dims != Dims || O.form != OutForm) break;
                E.res = Other;
            }
        } else if (E.act == kActNone && !C->In.empty() && C->In[0] == Cur && nodeAct(*C) != kActNone) {
            E.act = nodeAct(*C);
        } else {
            break;
        }
        E.name += "+" + C->Name;
        Skip[indexOf(C)] = true;
        At = indexOf(C);
        Cur = C->Out[0];
        if (E.act != kActNone) break;
    }
    return E;
}

// The conv kernel's weights [tile][chunk][tap][16][64] and bias [tiles * 64]: f32 of the folded doubles
static void packDense(const LinearW& L, int Chunks, int Tiles, std::vector<float>* Pk, std::vector<float>* Bf) {
    const int Taps = L.taps();
    Pk->assign((size_t)Tiles * Chunks * Taps * kChunk * kCoutTile, 0.f);
    for (int T = 0; T < Tiles; ++T)
        for (int Ch = 0; Ch < Chunks; ++Ch)
            for (int Tp = 0; Tp < Taps; ++Tp)
                for (int Kk = 0; Kk < kChunk; ++Kk)
                    for (int Nn = 0; Nn < kCoutTile; ++Nn) {
                        const int O = T * kCoutTile + Nn, I = Ch * kChunk + Kk;
                        if (O >= L.Cout || I >= L.Cin) continue;
                        (*Pk)[((((size_t)T * Chunks + Ch) * Taps + Tp) * kChunk + Kk) * kCoutTile + Nn] =
                            (float)L.W[((size_t)O * L.Cin + I) * Taps + Tp];
                    }
    Bf->assign((size_t)Tiles * kCoutTile, 0.f);
    for (int O = 0; O < L.Cout; ++O) (*Bf)[(size_t)O] = (float)L.Bias[(size_t)O];
}

// The grouped conv kernel's weights, tables and bias.  Output o belongs to group o / (Cout /
// Groups) and reads the CinW input channels from group * CinW.  A tile of 64 outputs holds the 16-channel chunks its
// outputs' groups read -- its chunk range -- as [chunk of the range][tap][16][64], exact zeros where input and output
// channel lie in different groups; the tiles follow one another.  Tb: kGroupTabInts ints per tile, bit for bit in
// floats: the range's first chunk and chunk count, the tile's offset into Pk in floats, 0, then (first chunk, chunk
// count) of each wave's 16 outputs, a sub-range of the tile's (count 0: every output of the wave is past Cout).
static void packGrouped(const LinearW& L, int Tiles, std::vector<float>* Pk, std::vector<float>* Tb, std::vector<float>* Bf) {
    const int Taps = L.taps(), OutPer = L.Cout / L.Groups;
    std::vector<int32_t> Tab((size_t)Tiles * kGroupTabInts, 0);
    Pk->clear();
    for (int T = 0; T < Tiles; ++T) {
        int32_t* Row = &Tab[(size_t)T * kGroupTabInts];
        int First = INT_MAX, End = 0;
        for (int Wv = 0; Wv < kCoutTile / kChunk; ++Wv) {
            const int OLo = T * kCoutTile + Wv * kChunk, OHi = std::min(OLo + kChunk, L.Cout) - 1; // the wave's outputs
            if (OLo >= L.Cout) continue;
            const int CLo = (OLo / OutPer) * L.CinW / kChunk, CHi = ((OHi / OutPer + 1) * L.CinW - 1) / kChunk;
            Row[4 + 2 * Wv] = CLo;
            Row[5 + 2 * Wv] = CHi - CLo + 1;
            First = std::min(First, CLo);
            End = std::max(End, CHi + 1);
        }
        const int Count = End - First;
        const size_t Off = Pk->size();
        Row[0] = First;
        Row[1] = Count;
        Row[2] = (int32_t)Off;
        Pk->resize(Off + (size_t)Count * Taps * kChunk * kCoutTile, 0.f);
        for (int Ch = 0; Ch < Count; ++Ch)
            for (int Tp = 0; Tp < Taps; ++Tp)
                for (int Kk = 0; Kk < kChunk; ++Kk)
                    for (int Nn = 0; Nn < kCoutTile; ++Nn) {
                        const int O = T * kCoutTile + Nn, I = (First + Ch) * kChunk + Kk;
                        if (O >= L.Cout || I >= L.Cin || I / L.CinW != O / OutPer) continue;
                        (*Pk)[Off + (((size_t)Ch * Taps + Tp) * kChunk + Kk) * kCoutTile + Nn] =
                            (float)L.W[((size_t)O * L.CinW + I % L.CinW) * Taps + Tp];
                    }
    }
    Tb->resize(Tab.size());
    std::memcpy(Tb->data(), Tab.data(), Tab.size() * sizeof(int32_t));
    Bf->assign((size_t)Tiles * kCoutTile, 0.f);
    for (int O = 0; O < L.Cout; ++O) (*Bf)[(size_t)O] = (float)L.Bias[(size_t)O];
}

// The depthwise kernel's per-channel taps [chunk][tap][16] and bias [chunks * 16]
static void packDepthwise(const LinearW& L, int Chunks, std::vector<float>* Pk, std::vector<float>* Bf) {
    const int Taps = L.taps();
    Pk->assign((size_t)Chunks * Taps * kChunk, 0.f);
    for (int C = 0; C < L.Cout; ++C)
        for (int Tp = 0; Tp < Taps; ++Tp)
            (*Pk)[((size_t)(C / kChunk) * Taps + Tp) * kChunk + C % kChunk] = (float)L.W[(size_t)C * Taps + Tp];
    Bf->assign((size_t)Chunks * kChunk, 0.f);
    for (int O = 0; O < L.Cout; ++O) (*Bf)[(size_t)O] = (float)L.Bias[(size_t)O];
}

// ---- Conv / Gemm / MatMul with their epilogue: one kLaunchConv -------------------------------------------------------
void Planner::linear(const Node& N, size_t Index) {
    const Val& X = get(N, 0);
    if (!X.runtime) fail(N, "the data input is a constant");
    const bool Dense = N.Op != "Conv";
    // the token rows seq-first, [81,N,C] or the 2-D [N*81,C] (seqView): the same Linear over the same rows; the epilogue
    // folds in those shapes, a token residual behind the views back joins later (lateResidual)
    const bool Seq3 = X.form == kFormSeqTok, Seq2 = X.form == kFormSeqRows;
    const bool Tok = X.form == kFormToken || Seq3 || Seq2; // a Linear over tokens: the 1x1 form of the conv, rows = (board, square)
    if (Tok && N.Op != "MatMul" && !Seq2) fail(N, "a token tensor " + dimsStr(X.dims) + " feeds MatMul, not " + N.Op);
    Val XTok = X; // (denseWeights reads a token tensor's channels off [N,81,C])
    if (Seq3 || Seq2) XTok.dims = {kBatch, 81, (int64_t)X.v.C};
    LinearW Lw = Dense ? denseWeights(N, XTok, Tok) : convWeights(N, X);
    const int Cout = Lw.Cout;
    const std::vector<int64_t> Dims = Seq3 ? std::vector<int64_t>{81, kBatch, Cout}
                                      : Seq2 ? std::vector<int64_t>{batchTimes(81), Cout}
                                      : Tok  ? std::vector<int64_t>{kBatch, 81, Cout}
                                             : Dense ? std::vector<int64_t>{kBatch, Cout} : std::vector<int64_t>{kBatch, Cout, 9, 9};
    const int OutForm = Tok ? X.form : kFormPlain;
    const Epilogue E = foldEpilogue(N, Index, Dims, Tok && !Seq2 ? 2 : 1, OutForm, &Lw);
    Launch L;
    L.name = E.name;
    ConvArgs& A = L.args.emplace<ConvArgs>();
    A.dense = Dense && !Tok;
    A.depthwise = Lw.Depthwise;
    A.taps = Lw.taps();
    A.kh = Lw.KH;
    A.kw = Lw.KW;
    A.dh = Lw.DH;
    A.dw = Lw.DW;
    A.in = plain(N.In[0], N.Name + " (input copy)");
    A.cinPad = roundUp(Lw.Cin, kChunk);
    A.coutTiles = Lw.Depthwise ? 0 : (Cout + kCoutTile - 1) / kCoutTile;
    A.act = E.act;
    if (!E.res.empty()) A.res = ready(E.res).v;
    std::vector<float> Pk, Bf, Tb;
    if (Lw.Depthwise) packDepthwise(Lw, A.cinPad / kChunk, &Pk, &Bf);
    else if (Lw.Groups > 1) packGrouped(Lw, A.coutTiles, &Pk, &Tb, &Bf);
    else packDense(Lw, A.cinPad / kChunk, A.coutTiles, &Pk, &Bf);
    if (Pk.size() > (size_t)INT32_MAX) fail(N, "the packed weights exceed 2^31 floats");
    A.wOff = addConst(Pk);
    A.biasOff = addConst(Bf);
    if (Lw.Groups > 1) { // the tables are constants of grouped launches only: every other plan keeps its blob
        A.groups = Lw.Groups;
        A.gTabOff = addConst(Tb);
    }
    L.out = freshView(Cout, !A.dense);
    P.flopsPerPosition += 2.0 * (A.dense ? 1 : 81) * A.taps * (double)Lw.CinW * Cout;
    Val V;
    if (Seq3 || Seq2) {
        V.runtime = true;
        V.dims = Dims;
        V.form = OutForm;
        if (E.res.empty() && E.act == kActNone) OpenLinear[E.out] = P.launches.size();
    } else {
        V = runtimeVal(N, Dims, OutForm);
    }
    V.v = L.out;
    V.producer = N.Name;
    emit(L);
    Vals[E.out] = V;
}

// ---- MatMul of head rows [N,H,K] with a constant [K,M]: the dense form of graphConv<1> over N * H rows -----------------
// The rows of (board, head) lie H to a board at stride K, so the launch is a dense layer whose row count is boards * H;
// the result is head rows [N,H,M] in a flat virtual buffer of stride H * (M rounded up to 16).  The epilogue takes the
// constant per-channel Adds and one activation; a residual is not absorbed (the Add is then refused as a reader of head rows).
void Planner::headRowsDense(const Node& N, size_t Index) {
    const Val X = get(N, 0);
    const int H = X.headRows;
    LinearW Lw = denseWeights(N, X, true);
    const int Cout = Lw.Cout;
    const std::vector<int64_t> Dims{kBatch, H, Cout};
    const Epilogue E = foldEpilogue(N, Index, Dims, 2, -1, &Lw);
    Launch L;
    L.name = E.name;
    ConvArgs& A = L.args.emplace<ConvArgs>();
    A.dense = true;
    A.rowsPerBoard = H;
    A.taps = A.kh = A.kw = 1;
    A.in = X.v;
    A.cinPad = roundUp(Lw.Cin, kChunk);
    A.coutTiles = (Cout + kCoutTile - 1) / kCoutTile;
    A.act = E.act;
    std::vector<float> Pk, Bf;
    packDense(Lw, A.cinPad / kChunk, A.coutTiles, &Pk, &Bf);
    A.wOff = addConst(Pk);
    A.biasOff = addConst(Bf);
    L.out.stride = roundUp(Cout, kChunk);
    L.out.C = Cout;
    L.out.spatial = false;
    L.out.buf = newVirt(H * L.out.stride, false);
    P.flopsPerPosition += 2.0 * H * (double)Lw.Cin * Cout;
    Val V;
    V.runtime = true;
    V.dims = Dims;
    V.form = kFormHeadRows;
    V.headRows = H;
    V.v = L.out;
    V.producer = N.Name;
    emit(L);
    Vals[E.out] = V;
}

// ---- MatMul of two run-time token tensors: one kLaunchBmm ("run-time products") ---------------
// Taken when both inputs are run-time tensors that are spatial, flat, token or [N,C,81] tensors; the attention
// pattern's 4-D tensors went to attentionOp before, and every other form keeps the refusal it had.
bool Planner::bmmOperands(const Node& N) const {
    if (N.Op != "MatMul" || N.In.size() != 2) return false;
    for (const std::string& I : N.In) {
        auto It = Vals.find(I);
        if (It == Vals.end() || !It->second.runtime || It->second.normG > 0) return false;
        const int F = It->second.form;
        if (F != kFormPlain && F != kFormToken && F != kFormChan3) return false;
    }
    return true;
}

void Planner::bmm(const Node& N, size_t Index) {
    const Val A0 = get(N, 0), B0 = get(N, 1);
    auto shown = [](const Val& V) { return dimsStr(V.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)V.v.C * 81} : V.dims); };
    const std::string Shapes = "MatMul of " + shown(A0) + " and " + shown(B0) + ", both computed at run time: ";
    if (A0.form == kFormChan3 && B0.form != kFormPlain)
        fail(N, Shapes + "the first operand is transposed ([N,K,81] x [N,81,M]); only [N,81,K] x [N,K,81] and [N,81,81] x [N,81,M] are run-time products (DESIGN.md section 13.3)");
    if (A0.form != kFormToken || B0.form == kFormPlain)
        fail(N, Shapes + "a flat or spatial operand; a run-time product takes token tensors [N,81,C], the second one also as [N,K,81] (DESIGN.md section 13.3)");
    const bool NN = B0.form == kFormToken;
    const int64_t Inner = A0.dims[2], BInner = NN ? 81 : B0.dims[1];
    if (Inner != BInner)
        fail(N, Shapes + "the inner dimensions disagree (" + std::to_string(Inner) + " and " + std::to_string(BInner) + ")");
    if (!NN) { // [N,K,81] is never materialised: this MatMul is its one reader
        auto U = Uses.find(N.In[1]);
        auto S = ShapeUses.find(N.In[1]);
        const int Data = (U == Uses.end() ? 0 : U->second) - (S == ShapeUses.end() ? 0 : S->second);
        if (Outputs.count(N.In[1]) || Data != 1)
            fail(N, Shapes + "'" + N.In[1] + "' " + shown(B0) + " has a second consumer; a [N,K,81] tensor is a view for one reader");
    }
    // a view at a multiple of 4 is read where it lies, any other is copied into rows of its own first
    auto operand = [&](const std::string& Name) {
        const View V0 = ready(Name).v;
        if (V0.offset % 4 == 0) return V0;
        return Vals[Name].v = copyOf(V0, true, N.Name + " (input copy)");
    };
    Launch L;
    BmmArgs& A = L.args.emplace<BmmArgs>();
    A.in = operand(N.In[0]);
    A.bmmB = operand(N.In[1]);
    A.bmmNN = NN;
    A.bmmK = (int)Inner;
    const int Cout = NN ? (int)B0.dims[2] : 81;
    // the epilogue: constant scalar Mul / Div nodes, then at most one parameter-free activation
    std::string Name = N.Name, Cur = N.Out[0];
    double Scale = 1.0;
    size_t At = Index;
    while (absorbable(Cur)) {
        const Node* C = onlyConsumer(Cur, At);
        if (!C) break;
        double S = 0;
        if ((C->Op == "Mul" || C->Op == "Div") && C->In.size() == 2 && C->In[0] != C->In[1] &&
            (C->In[0] == Cur || C->Op == "Mul") && scalarAhead(C->In[0] == Cur ? C->In[1] : C->In[0], &S)) {
            Scale = C->Op == "Mul" ? Scale * S : Scale / S;
        } else if (!C->In.empty() && C->In[0] == Cur && nodeAct(*C) != kActNone) {
            A.act = nodeAct(*C);
        } else {
            break;
        }
        Name += "+" + C->Name;
        Skip[indexOf(C)] = true;
        At = indexOf(C);
        Cur = C->Out[0];
        if (A.act != kActNone) break;
    }
    L.name = Name;
    A.scale = (float)Scale;
    L.out = freshView(Cout, true);
    P.flopsPerPosition += 2.0 * 81 * 81 * (double)(NN ? Cout : Inner);
    Val V = runtimeVal(N, {kBatch, 81, Cout}, kFormToken);
    V.v = L.out;
    emit(L);
    Vals[Cur] = V;
}

} // namespace nsg::graph
