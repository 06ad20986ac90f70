// planner.h -- what the planner's translation units share (onnx_graph.cc and planner_*.cc).
// Internal: not installed, and not included by nsg_capi.hip or graph_exec.hip, which see onnx_graph.h only.
// A planner method builds the argument record of its launch's kind (onnx_graph.h) and hands the Launch to emit(); the
// record names its own device views, so nothing here lists view fields.
#ifndef NSG_PLANNER_H
#define NSG_PLANNER_H

#include "onnx_graph.h"
#include "onnx_proto.h"
#include "plan_lifetimes.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <set>

namespace nsg::graph {

using namespace nsg::onnx::wire;

constexpr int64_t kBatch = INT64_MIN / 2; // the symbolic batch dimension inside folded shape values
constexpr int kPending = -3; // the view of an open elementwise group: its buffer is assigned when the group is emitted

// The batch times a constant inside folded shape values: N*H and N*81 of the stock transformer modules' export
// (DESIGN.md section 13.3).  batchTimes(1) is kBatch itself; batchFactor is 0 for a plain number.
constexpr int64_t kMaxBatchFactor = 1 << 24;
inline int64_t batchTimes(int64_t K) { return kBatch + (K - 1); }
inline int64_t batchFactor(int64_t V) { return V >= kBatch && V < kBatch + kMaxBatchFactor ? V - kBatch + 1 : 0; }

inline int roundUp(int a, int b) { return (a + b - 1) / b * b; }

inline std::string dimsStr(const std::vector<int64_t>& D) {
    std::string S = "[";
    for (size_t I = 0; I < D.size(); ++I) {
        if (I) S += ",";
        S += D[I] == kBatch ? std::string("N") : batchFactor(D[I]) ? "N*" + std::to_string(batchFactor(D[I])) : std::to_string(D[I]);
    }
    return S + "]";
}

// Logical shapes a runtime tensor may have besides [N,C,9,9] and flat.  kFormToken is a full citizen (dense layers,
// elementwise ops, LayerNorm, the mean over squares); [N,C,81] exists only between a Reshape and a Transpose, where
// the token-mixing pattern (planner_mix.cc) may read and write it; the
// 4-D forms exist only inside the attention pattern and become one kLaunchAttention.
enum Form {
    kFormPlain = 0,
    kFormToken,   // [N,81,C]
    kFormChan3,   // [N,C,81]
    kFormTok4,    // [N,81,H,d]: q, k or v split into heads
    kFormHeads,   // [N,H,81,d]
    kFormHeadsT,  // [N,H,d,81]: k transposed
    kFormScores,  // [N,H,81,81] before the Softmax
    kFormProbs,   // [N,H,81,81] after it
    kFormHeadOut, // [N,H,81,d]: probs x v
    kFormTokOut4, // [N,81,H,d]
    kFormGroup3,  // [N,G,M], G M = C 81: the groups of a GroupNorm, between its two Reshapes only ([N,C,81] when G = C)
    kFormChanLast, // [N,9,9,C]: the spatial rows once more, for a LayerNorm over the channels between two Transposes
    kFormHeadRows, // [N,H,K]: rows of (board, head), a view of a flat [N,H*K]; read by a MatMul with a constant [K,M] only
    kFormScoreBias, // [N,H,81,81] or [N,1,81,81]: a flat or head-row tensor as the run-time bias of attention scores
    kFormLine,      // [N,C,9,1] rank lines, [N,C,1,9] file lines, [N,C,18,1]: rows of (board, line); read by the ops of planner_lines.cc only
    // the seq-first forms of nn.MultiheadAttention's export (seqView, planner_views.cc): the token rows under other names
    kFormSeqTok,    // [81,N,C]: the token tensor under Transpose [1,0,2]
    kFormSeqRows,   // [N*81,C]: those rows as a 2-D matrix, between a Reshape and the Linear that reads it
    kFormSeqPacked, // the packed q / k / v projection on its way to three views: [81,N,3,E], [1,81,N,3,E], [3,81,N,1,E], [3,81,N,E]
    kFormSeqHeads,  // [81,N*H,d]: q, k or v split into heads; dims hold [81,N,H,d] (Val::bh)
    kFormSeqOut,    // probs x v on the way back: [81,N,H,d] (Val::bh: [81,N*H,d]); dims hold [81,N,H,d]
};
inline bool isAttForm(int F) { return F >= kFormTok4 && F <= kFormTokOut4; }

// A tensor of the graph: a host value (constant or folded shape), or a runtime tensor on the device.
struct Val {
    bool runtime = false;
    std::vector<int64_t> dims; // runtime: logical ONNX dims, dims[0] = kBatch (the kFormSeq* forms: 81 or N*81 first)
    // host
    bool isInt = false;
    std::vector<double> f;
    std::vector<int64_t> i;
    // runtime
    View v;
    bool flatOfSpatial = false; // a flattened spatial tensor [N, C*81] (index c*81 + square); v is the spatial view
    int form = kFormPlain;      // another logical shape over the spatial rows (Form); v is the spatial view
    // the attention pattern's state (forms kFormTok4 and later), carried from the Reshape of q to the final Reshape
    double scale = 1.0;         // scalar factors folded so far
    View attQ, attK, attV;      // kFormScores and later: the q and k token views; kFormHeadOut and later: v's
    std::vector<double> bias;   // kFormScores and later: [H][81][81], empty = none
    // kFormScores and later: the run-time bias (hasRt), added as rtScale * rtBias.  kFormScoreBias: v is the view (its
    // stride the floats from board to board) and rtHead the floats from head to head, 0 for [N,1,81,81]
    bool hasRt = false;
    View rtBias;
    int rtHead = 0;
    double rtScale = 1.0;
    // kFormHeads .. kFormHeadOut and kFormSeqOut: the tensor is the 3-D form on the (board x head) axis, [N*H,81,d] for
    // [N,H,81,d]; dims hold the 4-D shape, shownDims() the tensor's own
    bool bh = false;
    bool viaSeq = false;        // the attention pattern was entered through the seq-first head split
    bool packedPart = false;    // kFormSeqTok: q, k or v taken out of the packed projection
    int headRows = 0;           // kFormHeadRows: H; v.stride is the stride of one (board, head) row, v.C = K
    std::vector<int64_t> expandTo; // a one-channel tensor behind an Expand: the shape the Expand names; dims stay the one-channel shape
    int lineLaunch = -1;        // kFormLine: the kLaunchLinePool that wrote it and has no other reader yet (-1: none)
    std::string chain;          // names of the nodes absorbed so far
    // the GroupNorm pattern's state ([N,G,M] behind its InstanceNormalization, until the Reshape back)
    int normG = 0;              // > 0: normalised per group, not yet launched
    std::vector<double> normA, normB; // the InstanceNormalization's per-group scale and bias
    double normEps = 0.0;
    int group = -1;             // open elementwise group that computes it (v not yet assigned)
    std::string producer;       // node name
    size_t count() const { return isInt ? i.size() : f.size(); }
    double at(size_t k) const { return isInt ? (double)i[k] : f[k]; }
    // the tensor's own dims: dims, but for the 3-D forms on the (board x head) axis
    std::vector<int64_t> shownDims() const {
        if (!runtime || !bh || dims.size() != 4) return dims;
        if (form == kFormSeqOut || form == kFormSeqHeads) return {dims[0], batchTimes(dims[2]), dims[3]};
        return {batchTimes(dims[1]), dims[2], dims[3]};
    }
    std::string shownStr() const { return dimsStr(shownDims()); }
};

// An elementwise chain being fused into one launch.
struct Group {
    bool open = true;
    bool spatial = false;
    int lines = 0;    // > 0: a line tensor of that many lines per board
    int C = 0;
    std::vector<EltSrc> srcs;
    std::vector<EltInstr> code;
    int nregs = 0;
    int outReg = 0;
    std::string out;  // tensor it computes
    std::string name; // nodes
};

// op classes, shapes (planner_host.cc)
bool isAct(const std::string& Op);
bool isBinary(const std::string& Op);
bool isEltExtra(const std::string& Op);
const std::set<std::string>& opSet();
bool broadcast(const std::vector<int64_t>& A, const std::vector<int64_t>& B, std::vector<int64_t>* Out);
std::vector<int> variesAlong(const std::vector<int64_t>& D, size_t R);

// The pattern rewrites (planner_rewrites.cc): swish, erf-GELU, Mish, tanh-GELU and softsign become one node each, the
// nodes they absorb are marked in Skip.
void rewritePatterns(std::vector<Node>& Nodes, std::vector<bool>& Skip, const std::map<std::string, Tensor>& Inits,
                     const std::set<std::string>& Outputs);

// Every device view a launch reads or writes: the lifetime pass and the renaming pass of assignBuffers go through it.
// The views a launch reads are named by its argument record, beside its fields (views(), onnx_graph.h); `out` comes
// last.  F(Name, View&): the name is what the lifetimes dump prints (LifetimeTrace).
template <class Fn> void forEachNamedView(Launch& L, Fn F) {
    std::visit([&](auto& A) { A.views(F); }, L.args);
    F("out", L.out);
}
template <class Fn> void forEachView(Launch& L, Fn F) {
    forEachNamedView(L, [&](const char*, View& V) { F(V); });
}

// Lifetimes -> physical buffers: renames the virtual buffers of the launches' views and of the three output views,
// and fills the plan's buffer stride tables (onnx_graph.cc).
// VirtAlsoFlat: the flat stride a spatial virtual buffer is also read at (a token tensor viewed as flat rows), 0 = none.
// Trace: where given, the record of what was renamed (plan_lifetimes.h).
void assignBuffers(GraphPlan& P, const std::vector<int>& VirtStride, const std::vector<bool>& VirtSpatial,
                   const std::vector<int>& VirtAlsoFlat, LifetimeTrace* Trace = nullptr);

// A linear layer's weights as read from the model, W[cout][CinW][taps], before packing (planner_linear.cc)
struct LinearW {
    int Cin = 0, Cout = 0, KH = 1, KW = 1, DH = 1, DW = 1;
    int CinW = 0;           // input channels per output channel in W: Cin, Cin / Groups, or 1 for a depthwise conv
    int Groups = 1;         // > 1: a grouped conv, output o reads the CinW inputs from (o / (Cout / Groups)) * CinW
    bool Depthwise = false;
    std::vector<double> W, Bias; // taps row-major over (ky, kx)
    int taps() const { return KH * KW; }
};

class Planner {
 public:
    Planner(const Graph& G, int NumChannels, GraphPlan* P, LifetimeTrace* Trace = nullptr)
        : G(G), P(*P), NumChannels(NumChannels), Trace(Trace) {}

    void run();

 private:
    const Graph& G;
    GraphPlan& P;
    const int NumChannels;
    LifetimeTrace* const Trace;
    std::map<std::string, Val> Vals;
    std::map<std::string, int> Uses; // live consumers (+1 for a graph output)
    std::map<std::string, int> ShapeUses; // ... of which Shape nodes
    std::set<std::string> Outputs;
    std::vector<bool> Skip;          // nodes absorbed into an earlier launch
    std::vector<Node> Nodes;         // after the rewrites (rewritePatterns)
    std::map<std::string, size_t> ProducerOf; // tensor -> the live node that computes it
    std::vector<Group> Groups;
    std::vector<int> VirtStride;     // per produced tensor (virtual buffer)
    std::vector<bool> VirtSpatial;
    std::vector<int> VirtAlsoFlat;   // see assignBuffers
    struct PendingLaunch { Launch L; std::string out; Val V; };
    std::map<size_t, PendingLaunch> PendingMix; // a token-mixing launch waiting for its pattern's last node (planner_mix.cc)
    // a seq-first Linear without residual or activation whose result is still read by one chain of views: tensor ->
    // launch.  The Add of a token residual behind those views joins the launch (lateResidual, planner_views.cc)
    std::map<std::string, size_t> OpenLinear;
    // an F.normalize chain waiting for its Div (planner_norms.cc): the Div's index -> the ReduceL1 / ReduceL2 at `reduce`,
    // the Clip and the optional Expand between them (`interior`, marked in Skip), none of them lowered yet
    struct PendingNormalize { size_t reduce = 0; std::vector<size_t> interior; int p = 2; float eps = 0.f; };
    std::map<size_t, PendingNormalize> OpenNormalize;

    [[noreturn]] void fail(const Node& N, const std::string& Why) const {
        throw Error("node '" + N.Name + "' (" + N.Op + "): " + Why);
    }
    const Val& get(const Node& N, size_t Idx) {
        if (Idx >= N.In.size() || N.In[Idx].empty()) fail(N, "missing input " + std::to_string(Idx));
        auto It = Vals.find(N.In[Idx]);
        if (It == Vals.end()) fail(N, "input '" + N.In[Idx] + "' is not defined before its use");
        return It->second;
    }
    bool has(const Node& N, size_t Idx) const { return Idx < N.In.size() && !N.In[Idx].empty(); }
    const Val& host(const Node& N, size_t Idx, const char* What) {
        const Val& V = get(N, Idx);
        if (V.runtime) fail(N, std::string(What) + " must be a constant (it is computed at run time)");
        return V;
    }
    std::vector<int64_t> ints(const Node& N, size_t Idx, const char* What) {
        const Val& V = host(N, Idx, What);
        std::vector<int64_t> R;
        for (size_t K = 0; K < V.count(); ++K) R.push_back(V.isInt ? V.i[K] : (int64_t)V.f[K]);
        return R;
    }
    int newVirt(int Stride, bool Spatial) {
        VirtStride.push_back(Stride);
        VirtSpatial.push_back(Spatial);
        VirtAlsoFlat.push_back(0);
        return (int)VirtStride.size() - 1;
    }
    // a line tensor of L lines per board in a buffer of its own: flat, L rows of the stride per board
    View freshLines(int C, int L) {
        View V;
        V.stride = roundUp(std::max(C, 1), kChunk);
        V.C = C;
        V.lines = V.bufLines = L;
        V.buf = newVirt(L * V.stride, false);
        return V;
    }
    static int lineCount(const std::vector<int64_t>& D) { // 9 or 18 for the dims of a line tensor, else 0
        if (D.size() != 4 || D[0] != kBatch || D[1] <= 0) return 0;
        if (D[3] == 1 && (D[2] == 9 || D[2] == 18)) return (int)D[2];
        return D[2] == 1 && D[3] == 9 ? 9 : 0;
    }
    View freshView(int C, bool Spatial) {
        View V;
        V.stride = roundUp(std::max(C, 1), kChunk);
        V.C = C;
        V.spatial = Spatial;
        V.buf = newVirt(V.stride, Spatial);
        return V;
    }
    size_t addConst(const std::vector<float>& F) {
        const size_t Off = P.weights.size();
        P.weights.insert(P.weights.end(), F.begin(), F.end());
        while (P.weights.size() % 4) P.weights.push_back(0.f); // every record 16-byte aligned
        return Off;
    }

    // runtime tensor kinds
    static bool isSpatialDims(const std::vector<int64_t>& D) {
        return D.size() == 4 && D[0] == kBatch && D[1] > 0 && D[2] == 9 && D[3] == 9;
    }
    // flat: [N], [N,C], [N,C,1], [N,C,1,1]; returns C or -1
    static int flatC(const std::vector<int64_t>& D) {
        if (D.empty() || D.size() > 4 || D[0] != kBatch) return -1;
        if (D.size() == 1) return 1;
        if (D[1] <= 0) return -1;
        for (size_t K = 2; K < D.size(); ++K)
            if (D[K] != 1) return -1;
        return (int)D[1];
    }
    static bool isTokenDims(const std::vector<int64_t>& D) {
        return D.size() == 3 && D[0] == kBatch && D[1] == 81 && D[2] > 0;
    }
    Val runtimeVal(const Node& N, const std::vector<int64_t>& Dims, int Form = kFormPlain) const {
        Val V;
        V.runtime = true;
        V.dims = Dims;
        V.producer = N.Name;
        V.form = Form;
        if (Form == kFormChanLast) {
            if (Dims.size() != 4 || Dims[0] != kBatch || Dims[1] != 9 || Dims[2] != 9 || Dims[3] <= 0)
                fail(N, "output shape " + dimsStr(Dims) + " is not the channel-last view [N,9,9,C]");
        } else if (Form == kFormToken ? !isTokenDims(Dims) : (!isSpatialDims(Dims) && flatC(Dims) < 0))
            fail(N, "output shape " + dimsStr(Dims) + " is neither [N,C,9,9], a token tensor [N,81,C] nor flat [N,C] / [N,C,1,1]");
        return V;
    }

    void emit(Launch L) {
        if (L.is<ConvArgs>()) ++P.convLaunches;
        if (L.is<AttentionArgs>()) ++P.attentionLaunches;
        P.launches.push_back(std::move(L));
    }
    void emitGroup(int Gi) {
        Group& Gr = Groups[(size_t)Gi];
        if (!Gr.open) return;
        Gr.open = false;
        Launch L;
        L.name = Gr.name;
        L.out = Gr.lines ? freshLines(Gr.C, Gr.lines) : freshView(Gr.C, Gr.spatial);
        L.args = EltProgram{Gr.srcs, Gr.code, Gr.outReg};
        emit(L);
        Val& V = Vals[Gr.out];
        V.v = L.out;
        V.group = -1;
    }
    // the value's device view, every pending launch that computes it emitted
    const Val& ready(const std::string& Name) {
        Val& V = Vals.at(Name);
        if (V.group >= 0) emitGroup(V.group);
        return Vals.at(Name);
    }
    // a copy of view V in rows of its own: one kLaunchConcat of one segment
    View copyOf(const View& V, bool Spatial, const std::string& Why) {
        const View Out = freshView(V.C, Spatial);
        emit(Launch{Why, Out, ConcatSegs{{CopySeg{V, 0}}}});
        return Out;
    }
    // a view with offset 0 in a buffer of its own kind (conv input, dense input, mean input)
    View plain(const std::string& Name, const std::string& Why) {
        const Val& V0 = ready(Name);
        if (!V0.flatOfSpatial && V0.v.offset == 0 && V0.v.stride == roundUp(V0.v.C, kChunk)) return V0.v;
        const View Out = V0.flatOfSpatial ? freshView(V0.v.C * 81, false) : copyOf(V0.v, V0.v.spatial, Why);
        if (V0.flatOfSpatial) emit(Launch{Why, Out, FlattenArgs{V0.v}});
        Val& V = Vals[Name];
        V.v = Out;
        V.flatOfSpatial = false;
        return Out;
    }

    // the stages of run(), in order (onnx_graph.cc)
    void checkContract();
    void countUses();
    void loadConstants();
    void defineInput();
    void lower(const Node& N, size_t Index); // the dispatch of one live node
    void checkOutputs();

    // planner_host.cc
    bool scalarAhead(const std::string& T, double* V, int Depth = 0) const;
    bool powExponent(const Node& N, double* E) const;
    int nodeAct(const Node& N) const;
    std::vector<int64_t> axes(const Node& N, size_t Rank, bool Added = false); // the `axes` input or attribute, none negative
    struct BnChannel { double scale, mean, beta; };         // y = (x - mean) * scale + beta
    BnChannel bnChannel(const Node& Bn, size_t Ch) const;
    void hostFold(const Node& N);
    Val foldArithmetic(const Node& N, const Val& X);
    // planner_linear.cc
    void linear(const Node& N, size_t Index);
    LinearW convWeights(const Node& N, const Val& X);
    LinearW denseWeights(const Node& N, const Val& X, bool Tok);
    struct Epilogue { std::string name, out, res; int act = kActNone; };
    Epilogue foldEpilogue(const Node& N, size_t Index, const std::vector<int64_t>& Dims, int ChanAxis, int OutForm, LinearW* Lw);
    // planner_elementwise.cc
    friend struct EltBuilder;
    void elementwise(const Node& N);
    void powOne(const Node& N);
    // planner_norms.cc
    void layerNorm(const Node& N);
    bool normOp(const Node& N, size_t Index); // InstanceNormalization, and the decomposed LayerNorm / RMSNorm chains
    void groupNorm(const Node& Last, size_t Index, const View& In, int C, int G, const std::vector<double>& A,
                   const std::vector<double>& B, double Eps, std::string Name);
    bool decomposedNorm(const Node& N, size_t Index);
    const Node* follow(const std::string& T, size_t After, const Node& From);
    bool lastAxis(const Node& N, const Val& X);
    bool normalizeOpen(const Node& N, size_t Index);  // a ReduceL1 / ReduceL2 that starts an F.normalize chain: deferred to its Div
    bool normalizeClose(const Node& N, size_t Index); // that Div: one kLaunchNormalize, or the chain's nodes lowered one by one
    // planner_pool.cc
    void pool(const Node& N);
    void reduceSquares(const Node& N);
    int channelAxis(const Node& N, const Val& X);    // a reduction's axes are the channel axis of X: 1 spatial, 2 token, 3 flat; 0: not
    void reduceChannels(const Node& N);              // ... as one kLaunchChanReduce
    // planner_lines.cc: rank and file pooling and the ops that read a line tensor
    void linePool(const Node& N, bool Files, bool Max);
    void lineOp(const Node& N, size_t Index);
    void lineConv(const Node& N, size_t Index);
    View linePlain(const std::string& Name, const std::string& Why);
    // planner_views.cc
    std::vector<int64_t> reshapeTarget(const Node& N, const std::vector<int64_t>& SD);
    bool formView(const Node& N);   // Transpose, and Reshape / Flatten to or from the forms above
    Val headsSource(const Node& N, const Val& X0);
    void attentionLaunch(const Node& N, const Val& X0, const std::vector<int64_t>& ND, int OutForm = kFormToken);
    bool seqReaders(const std::string& T) const;
    bool seqView(const Node& N);     // the seq-first forms of the stock transformer modules' export
    bool lateResidual(const Node& N); // x + (views of a seq-first Linear): the Add joins the Linear's launch
    int dataUses(const std::string& T) const { // live consumers that read the tensor's data (a Shape node does not)
        auto U = Uses.find(T);
        auto S = ShapeUses.find(T);
        return (U == Uses.end() ? 0 : U->second) - (S == ShapeUses.end() ? 0 : S->second);
    }
    bool flatFormView(const Node& N, const Val& X0); // token -> flat, flat -> head rows, flat / head rows -> score bias
    void headRowsDense(const Node& N, size_t Index); // MatMul of head rows [N,H,K] with a constant [K,M]
    bool bmmOperands(const Node& N) const;           // a MatMul of two run-time tensors outside the other patterns
    void bmm(const Node& N, size_t Index);           // ... as one kLaunchBmm (planner_linear.cc)
    // planner_mix.cc: a Linear over the 81 squares, one stage or two, as one kLaunchTokenMix
    bool mixEntry(const Node& N) const;              // a MatMul of a run-time [N,C,81] tensor with a constant
    void tokenMix(const Node& N, size_t Index);
    void mixFlush(size_t Index);
    // planner_gather.cc: Gather with constant indices and board flips, one kLaunchGather each
    void gather(const Node& N);
    void flipBoard(const Node& N, Val V, bool Ranks, bool Files); // a Slice with step -1 over whole board axes
    View gatherLaunch(const Node& N, const View& In, long Block, const std::vector<int>& RowTab, const std::vector<int>& ColTab,
                      bool Spatial);
    bool attentionOp(const Node& N); // MatMul / Mul / Div / Add / Softmax on the attention pattern's 4-D tensors
    void viewOp(const Node& N);     // Flatten / Reshape / Squeeze / Unsqueeze / Identity on a spatial or flat tensor
    void expandView(const Node& N); // Expand of a one-channel tensor over the channels: a view
    void concat(const Node& N);
    void slice(const Node& N);
    void split(const Node& N);
    // the tensor feeds one node only: the attention pattern's interior tensors are never materialised
    // (a Shape node reads no data: torch emits one on q for `q.size(-1) ** -0.5`)
    void interior(const Node& N, size_t Idx) const {
        const std::string& T = N.In[Idx];
        auto U = Uses.find(T);
        auto S = ShapeUses.find(T);
        const int Data = (U == Uses.end() ? 0 : U->second) - (S == ShapeUses.end() ? 0 : S->second);
        if (Outputs.count(T) || Data != 1)
            fail(N, "'" + N.In[Idx] + "' is an interior tensor of the attention pattern (DESIGN.md section 13.3) and has more than one consumer");
    }
    bool absorbable(const std::string& T) const {
        auto It = Uses.find(T);
        return !Outputs.count(T) && It != Uses.end() && It->second == 1;
    }
    const Node* onlyConsumer(const std::string& T, size_t After) const {
        for (size_t K = After + 1; K < Nodes.size(); ++K) {
            if (Skip[K]) continue;
            for (const std::string& I : Nodes[K].In)
                if (I == T) return &Nodes[K];
        }
        return nullptr;
    }
    size_t indexOf(const Node* N) const { return (size_t)(N - Nodes.data()); }
};

} // namespace nsg::graph

#endif
