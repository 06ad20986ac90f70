// onnx_graph.cc -- see onnx_graph.h and DESIGN.md section 13.
#include "onnx_graph.h"
#include "onnx_proto.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <set>

namespace nsg {
namespace graph {

namespace {

using namespace nsg::onnx::wire;

constexpr int64_t kBatch = INT64_MIN / 2; // the symbolic batch dimension inside folded shape values
constexpr int kNoRes = -2;
constexpr int kPending = -3; // the view of an open elementwise group: its buffer is assigned when the group is emitted

int roundUp(int a, int b) { return (a + b - 1) / b * b; }

std::string dimsStr(const std::vector<int64_t>& D) {
    std::string S = "[";
    for (size_t I = 0; I < D.size(); ++I) {
        if (I) S += ",";
        S += D[I] == kBatch ? std::string("N") : std::to_string(D[I]);
    }
    return S + "]";
}

// Logical shapes a runtime tensor may have besides [N,C,9,9] and flat.  kFormToken is a full citizen (dense layers,
// elementwise ops, LayerNorm, the mean over squares); [N,C,81] exists only between a Reshape and a Transpose; the
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
};
bool isAttForm(int F) { return F >= kFormTok4 && F <= kFormTokOut4; }

// A tensor of the graph: a host value (constant or folded shape), or a runtime tensor on the device.
struct Val {
    bool runtime = false;
    std::vector<int64_t> dims; // runtime: logical ONNX dims, dims[0] = kBatch
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
    std::string chain;          // names of the nodes absorbed so far
    // the GroupNorm pattern's state ([N,G,M] behind its InstanceNormalization, until the Reshape back)
    int normG = 0;              // > 0: normalised per group, not yet launched
    std::vector<double> normA, normB; // the InstanceNormalization's per-group scale and bias
    double normEps = 0.0;
    int group = -1;             // open elementwise group that computes it (v not yet assigned)
    std::string producer;       // node name
    size_t count() const { return isInt ? i.size() : f.size(); }
    double at(size_t k) const { return isInt ? (double)i[k] : f[k]; }
};

// An elementwise chain being fused into one launch.
struct Group {
    bool open = true;
    bool spatial = false;
    int C = 0;
    std::vector<EltSrc> srcs;
    std::vector<EltInstr> code;
    int nregs = 0;
    int outReg = 0;
    std::string out;  // tensor it computes
    std::string name; // nodes
};

class Planner {
 public:
    Planner(const Graph& G, int NumChannels, GraphPlan* P) : G(G), P(*P), NumChannels(NumChannels) {}

    void run();

 private:
    const Graph& G;
    GraphPlan& P;
    const int NumChannels;
    std::map<std::string, Val> Vals;
    std::map<std::string, int> Uses; // live consumers (+1 for a graph output)
    std::map<std::string, int> ShapeUses; // ... of which Shape nodes
    std::set<std::string> Outputs;
    std::vector<bool> Skip;          // nodes absorbed into an earlier launch
    std::vector<Node> Nodes;         // after the swish rewrite
    std::map<std::string, size_t> ProducerOf; // tensor -> the live node that computes it
    std::vector<Group> Groups;
    std::vector<int> VirtStride;     // per produced tensor (virtual buffer)
    std::vector<bool> VirtSpatial;

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
        return (int)VirtStride.size() - 1;
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
        if (L.kind == kLaunchConv) ++P.convLaunches;
        if (L.kind == kLaunchAttention) ++P.attentionLaunches;
        P.launches.push_back(std::move(L));
    }
    void emitGroup(int Gi) {
        Group& Gr = Groups[(size_t)Gi];
        if (!Gr.open) return;
        Gr.open = false;
        Launch L;
        L.kind = kLaunchElt;
        L.name = Gr.name;
        L.out = freshView(Gr.C, Gr.spatial);
        L.srcs = Gr.srcs;
        L.code = Gr.code;
        L.eltOut = Gr.outReg;
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
    // a view with offset 0 in a buffer of its own kind (conv input, dense input, mean input)
    View plain(const std::string& Name, const std::string& Why) {
        const Val& V0 = ready(Name);
        if (!V0.flatOfSpatial && V0.v.offset == 0 && V0.v.stride == roundUp(V0.v.C, kChunk)) return V0.v;
        Launch L;
        L.name = Why;
        if (V0.flatOfSpatial) {
            L.kind = kLaunchFlatten;
            L.in = V0.v;
            L.out = freshView(V0.v.C * 81, false);
        } else {
            L.kind = kLaunchConcat;
            CopySeg S;
            S.v = V0.v;
            L.segs.push_back(S);
            L.out = freshView(V0.v.C, V0.v.spatial);
        }
        const View Out = L.out;
        emit(L);
        Val& V = Vals[Name];
        V.v = Out;
        V.flatOfSpatial = false;
        return Out;
    }

    bool scalarAhead(const std::string& T, double* V, int Depth = 0) const;
    int nodeAct(const Node& N) const;
    void pool(const Node& N);
    void split(const Node& N);
    void hostFold(const Node& N);
    void linear(const Node& N, size_t Index);
    void elementwise(const Node& N);
    void layerNorm(const Node& N);
    bool normOp(const Node& N, size_t Index); // InstanceNormalization, and the decomposed LayerNorm / RMSNorm chains
    void groupNorm(const Node& Last, size_t Index, const View& In, int C, int G, const std::vector<double>& A,
                   const std::vector<double>& B, double Eps, std::string Name);
    bool decomposedNorm(const Node& N, size_t Index);
    const Node* follow(const std::string& T, size_t After, const Node& From);
    bool lastAxis(const Node& N, const Val& X);
    bool formView(const Node& N);   // Transpose, and Reshape / Flatten to or from the forms above
    bool attentionOp(const Node& N); // MatMul / Mul / Div / Add / Softmax on the attention pattern's 4-D tensors
    void rewriteGelu();
    void rewriteMath();
    bool powExponent(const Node& N, double* E) const;
    std::vector<int64_t> reshapeTarget(const Node& N, const std::vector<int64_t>& SD);
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
    void checkOutputs();
    void assignBuffers();
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

// (Swish, Gelu, MishAct, GeluTanh and Softsign are the planner's own nodes, written by its rewrites)
bool isAct(const std::string& Op) {
    return Op == "Relu" || Op == "Sigmoid" || Op == "Tanh" || Op == "Softplus" || Op == "Swish" || Op == "Erf" || Op == "Gelu" ||
           Op == "Exp" || Op == "Log" || Op == "Sqrt" || Op == "Reciprocal" || Op == "MishAct" || Op == "GeluTanh" || Op == "Softsign";
}
int actOf(const std::string& Op) {
    if (Op == "Relu") return kActRelu;
    if (Op == "Sigmoid") return kActSigmoid;
    if (Op == "Tanh") return kActTanh;
    if (Op == "Softplus") return kActSoftplus;
    if (Op == "Swish") return kActSwish;
    if (Op == "Erf") return kActErf;
    if (Op == "Gelu") return kActGelu;
    if (Op == "Exp") return kActExp;
    if (Op == "Log") return kActLog;
    if (Op == "Sqrt") return kActSqrt;
    if (Op == "Reciprocal") return kActRecip;
    if (Op == "MishAct") return kActMish;
    if (Op == "GeluTanh") return kActGeluTanh;
    if (Op == "Softsign") return kActSoftsign;
    return kActNone;
}
bool isBinary(const std::string& Op) { return Op == "Add" || Op == "Sub" || Op == "Mul" || Op == "Div"; }
// the other ops of the elementwise program: the clamp family, Max / Min of two operands, Abs, Neg
bool isEltExtra(const std::string& Op) {
    return Op == "Max" || Op == "Min" || Op == "Clip" || Op == "HardSwish" || Op == "HardSigmoid" || Op == "LeakyRelu" ||
           Op == "PRelu" || Op == "Abs" || Op == "Neg";
}

const std::set<std::string>& opSet() {
    static const std::set<std::string> S = {
        "Conv", "BatchNormalization", "Relu", "Sigmoid", "Tanh", "Softplus", "Add", "Sub", "Mul", "Div",
        "GlobalAveragePool", "ReduceMean", "Flatten", "Reshape", "Squeeze", "Unsqueeze", "Gemm", "MatMul",
        "Concat", "Slice", "Identity", "Constant", "Transpose", "LayerNormalization", "Erf", "Softmax",
        "MaxPool", "AveragePool", "GlobalMaxPool", "ReduceMax", "Split", "Clip", "HardSwish", "HardSigmoid", "LeakyRelu",
        "PRelu", "Max", "Min", "Abs", "Neg", "InstanceNormalization", "Exp", "Log", "Sqrt", "Reciprocal", "Pow",
        // folded on the host only (shape chains): refused on a runtime tensor
        "Shape", "Gather", "Cast"};
    return S;
}

// NumPy broadcast of two shapes (batch symbolic)
bool broadcast(const std::vector<int64_t>& A, const std::vector<int64_t>& B, std::vector<int64_t>* Out) {
    const size_t R = std::max(A.size(), B.size());
    Out->assign(R, 1);
    for (size_t K = 0; K < R; ++K) {
        const int64_t X = K < R - A.size() ? 1 : A[K - (R - A.size())];
        const int64_t Y = K < R - B.size() ? 1 : B[K - (R - B.size())];
        if (X == Y || Y == 1) (*Out)[K] = X;
        else if (X == 1) (*Out)[K] = Y;
        else return false;
    }
    return true;
}

// axes along which a shape, right-aligned to an output of rank R, varies (size != 1)
std::vector<int> variesAlong(const std::vector<int64_t>& D, size_t R) {
    std::vector<int> Ax;
    for (size_t K = 0; K < D.size(); ++K)
        if (D[K] != 1) Ax.push_back((int)(K + R - D.size()));
    return Ax;
}

// A constant scalar that may not be folded yet: the exporter puts a Clip's bounds behind Cast nodes that follow the
// conv whose epilogue looks ahead at the Clip.
bool Planner::scalarAhead(const std::string& T, double* V, int Depth) const {
    auto It = Vals.find(T);
    if (It != Vals.end()) {
        const Val& C = It->second;
        if (C.runtime || C.count() != 1 || (C.isInt && C.i[0] == kBatch)) return false;
        *V = C.at(0);
        return true;
    }
    auto Pr = ProducerOf.find(T);
    if (Pr == ProducerOf.end() || Depth > 4) return false;
    const Node& N = Nodes[Pr->second];
    const bool FloatCast = N.Op == "Cast" && (N.attrI("to", 1) == 1 || N.attrI("to", 1) == 11);
    if ((!FloatCast && N.Op != "Identity") || N.In.size() != 1) return false;
    return scalarAhead(N.In[0], V, Depth + 1);
}

// A Pow's exponent when it is a constant scalar (folded already, or still behind the exporter's Cast).
bool Planner::powExponent(const Node& N, double* E) const {
    return N.In.size() == 2 && !N.In[1].empty() && scalarAhead(N.In[1], E);
}

// The parameter-free activation a node is (a conv epilogue or one kEltAct instruction), or kActNone: relu6 is a Clip
// with bounds exactly 0 and 6, the hard sigmoid is taken at alpha = 1/6 (within one f32 ulp) and beta = 0.5 only.
int Planner::nodeAct(const Node& N) const {
    if (isAct(N.Op)) return actOf(N.Op);
    if (N.Op == "Pow") { // x ** 0.5 and x ** -1 are the square root and the reciprocal
        double E = 0;
        return powExponent(N, &E) && (E == 0.5 || E == -1.0) ? (E == 0.5 ? kActSqrt : kActRecip) : kActNone;
    }
    if (N.Op == "HardSwish") return kActHardSwish;
    if (N.Op == "HardSigmoid") {
        const float A = (float)N.attrF("alpha", 0.2), B = (float)N.attrF("beta", 0.5), K = 1.f / 6.f;
        return B == 0.5f && (A == K || A == std::nextafterf(K, 0.f) || A == std::nextafterf(K, 1.f)) ? kActHardSigmoid : kActNone;
    }
    if (N.Op == "Clip") {
        double Lo = 0, Hi = 0;
        if (N.In.size() == 3 && !N.In[1].empty() && !N.In[2].empty() && scalarAhead(N.In[1], &Lo) && scalarAhead(N.In[2], &Hi) &&
            Lo == 0.0 && Hi == 6.0)
            return kActRelu6;
    }
    return kActNone;
}

// ---- host folding (constants and shape chains) ---------------------------------------------------------------
void Planner::hostFold(const Node& N) {
    const std::string& Op = N.Op;
    Val R;
    auto Out = [&]() -> Val& { return Vals[N.Out[0]]; };
    if (Op == "Shape") {
        const Val& X = get(N, 0);
        std::vector<int64_t> D = X.dims;
        if (X.runtime && X.flatOfSpatial) D = {kBatch, (int64_t)X.v.C * 81};
        int64_t S = N.attrI("start", 0), E = N.attrI("end", (int64_t)D.size());
        if (S < 0) S += (int64_t)D.size();
        if (E < 0) E += (int64_t)D.size();
        S = std::max<int64_t>(0, std::min<int64_t>(S, (int64_t)D.size()));
        E = std::max<int64_t>(S, std::min<int64_t>(E, (int64_t)D.size()));
        R.isInt = true;
        R.i.assign(D.begin() + S, D.begin() + E);
        R.dims = {E - S};
        Out() = R;
        return;
    }
    if (Op == "Identity") { Out() = get(N, 0); return; }
    const Val& X = host(N, 0, "the data input");
    if (Op == "Cast") {
        const int64_t To = N.attrI("to", 1);
        R.dims = X.dims;
        if (To == 7 || To == 6) {
            R.isInt = true;
            for (size_t K = 0; K < X.count(); ++K) R.i.push_back(X.isInt ? X.i[K] : (int64_t)X.f[K]);
        } else if (To == 1 || To == 11) {
            for (size_t K = 0; K < X.count(); ++K) {
                if (X.isInt && X.i[K] == kBatch) fail(N, "cannot cast the batch dimension to a float");
                R.f.push_back(X.at(K));
            }
        } else {
            fail(N, "Cast to data type " + std::to_string(To) + " is not supported");
        }
        Out() = R;
        return;
    }
    if (Op == "Gather") {
        const std::vector<int64_t> Idx = ints(N, 1, "Gather's indices");
        const Val& Iv = host(N, 1, "Gather's indices");
        if (X.dims.size() != 1 || N.attrI("axis", 0) != 0) fail(N, "Gather is folded only on a 1-D constant along axis 0");
        R.isInt = X.isInt;
        for (int64_t K : Idx) {
            const int64_t J = K < 0 ? K + (int64_t)X.count() : K;
            if (J < 0 || J >= (int64_t)X.count()) fail(N, "Gather index out of range");
            if (X.isInt) R.i.push_back(X.i[(size_t)J]);
            else R.f.push_back(X.f[(size_t)J]);
        }
        R.dims = Iv.dims;
        Out() = R;
        return;
    }
    if (Op == "Unsqueeze" || Op == "Squeeze") {
        std::vector<int64_t> Axes = has(N, 1) ? ints(N, 1, "axes") : N.attrInts("axes", {});
        R = X;
        std::vector<int64_t> D = X.dims;
        if (Op == "Unsqueeze") {
            const int64_t Rank = (int64_t)(D.size() + Axes.size());
            for (int64_t& A : Axes) if (A < 0) A += Rank;
            std::sort(Axes.begin(), Axes.end());
            for (int64_t A : Axes) {
                if (A < 0 || A > (int64_t)D.size()) fail(N, "axis out of range");
                D.insert(D.begin() + A, 1);
            }
        } else {
            std::vector<int64_t> ND;
            for (size_t K = 0; K < D.size(); ++K) {
                bool Drop = Axes.empty() ? D[K] == 1 : false;
                for (int64_t A : Axes) Drop = Drop || (A < 0 ? A + (int64_t)D.size() : A) == (int64_t)K;
                if (!Drop) ND.push_back(D[K]);
            }
            D = ND;
        }
        R.dims = D;
        Out() = R;
        return;
    }
    if (Op == "Concat") {
        R.isInt = X.isInt;
        int64_t Total = 0;
        for (size_t K = 0; K < N.In.size(); ++K) {
            const Val& V = host(N, K, "a Concat input");
            if (V.dims.size() != 1) fail(N, "Concat of constants is folded only for 1-D values");
            if (V.isInt != R.isInt) fail(N, "Concat of mixed data types");
            R.i.insert(R.i.end(), V.i.begin(), V.i.end());
            R.f.insert(R.f.end(), V.f.begin(), V.f.end());
            Total += V.dims[0];
        }
        R.dims = {Total};
        Out() = R;
        return;
    }
    if (Op == "Slice") {
        if (X.dims.size() != 1) fail(N, "Slice of a constant is folded only for 1-D values");
        const std::vector<int64_t> St = ints(N, 1, "starts"), En = ints(N, 2, "ends");
        const std::vector<int64_t> Sp = has(N, 4) ? ints(N, 4, "steps") : std::vector<int64_t>{1};
        if (St.size() != 1 || En.size() != 1 || Sp.size() != 1 || Sp[0] != 1) fail(N, "only a unit-step 1-D slice is folded");
        const int64_t Len = (int64_t)X.count();
        int64_t S = St[0] < 0 ? St[0] + Len : St[0], E = En[0] < 0 ? En[0] + Len : En[0];
        S = std::max<int64_t>(0, std::min(S, Len));
        E = std::max<int64_t>(S, std::min(E, Len));
        R.isInt = X.isInt;
        for (int64_t K = S; K < E; ++K) {
            if (X.isInt) R.i.push_back(X.i[(size_t)K]);
            else R.f.push_back(X.f[(size_t)K]);
        }
        R.dims = {E - S};
        Out() = R;
        return;
    }
    if (Op == "Reshape") {
        const std::vector<int64_t> Sh = ints(N, 1, "the target shape");
        R = X;
        int64_t Known = 1, Infer = -1;
        for (size_t K = 0; K < Sh.size(); ++K) {
            if (Sh[K] == -1) Infer = (int64_t)K;
            else if (Sh[K] == 0 && K < X.dims.size()) Known *= X.dims[K];
            else Known *= Sh[K];
        }
        R.dims = Sh;
        for (size_t K = 0; K < Sh.size(); ++K)
            if (Sh[K] == 0 && K < X.dims.size()) R.dims[K] = X.dims[K];
        if (Infer >= 0) R.dims[(size_t)Infer] = Known ? (int64_t)X.count() / Known : 0;
        Out() = R;
        return;
    }
    if (isBinary(Op)) {
        const Val& Y = host(N, 1, "the second operand");
        std::vector<int64_t> D;
        if (!broadcast(X.dims, Y.dims, &D)) fail(N, "shapes " + dimsStr(X.dims) + " and " + dimsStr(Y.dims) + " do not broadcast");
        const size_t Cnt = std::max(X.count(), Y.count());
        if ((X.count() != Cnt && X.count() != 1) || (Y.count() != Cnt && Y.count() != 1))
            fail(N, "constant folding supports equal shapes or a scalar operand");
        R.dims = D;
        R.isInt = X.isInt && Y.isInt;
        for (size_t K = 0; K < Cnt; ++K) {
            const size_t A = X.count() == 1 ? 0 : K, B = Y.count() == 1 ? 0 : K;
            if (R.isInt) {
                const int64_t P1 = X.i[A], P2 = Y.i[B];
                int64_t V;
                const bool Sym = P1 == kBatch || P2 == kBatch;
                if (Sym) {
                    const int64_t Other = P1 == kBatch ? P2 : P1;
                    const bool Neutral = ((Op == "Mul") && Other == 1) || ((Op == "Div") && P1 == kBatch && Other == 1) ||
                                         ((Op == "Add" || Op == "Sub") && Other == 0 && !(Op == "Sub" && P2 == kBatch));
                    if (!Neutral || (P1 == kBatch && P2 == kBatch)) fail(N, "arithmetic on the symbolic batch dimension");
                    V = kBatch;
                } else if (Op == "Add") V = P1 + P2;
                else if (Op == "Sub") V = P1 - P2;
                else if (Op == "Mul") V = P1 * P2;
                else {
                    if (P2 == 0) fail(N, "integer division by zero");
                    V = P1 / P2;
                }
                R.i.push_back(V);
            } else {
                if ((X.isInt && X.i[A] == kBatch) || (Y.isInt && Y.i[B] == kBatch)) fail(N, "arithmetic on the symbolic batch dimension");
                const double P1 = X.at(A), P2 = Y.at(B);
                R.f.push_back(Op == "Add" ? P1 + P2 : Op == "Sub" ? P1 - P2 : Op == "Mul" ? P1 * P2 : P1 / P2);
            }
        }
        Out() = R;
        return;
    }
    if (Op == "Sqrt" || Op == "Pow" || Op == "Exp" || Op == "Log" || Op == "Reciprocal") { // torch emits them for `d ** -0.5` when d comes from size()
        const Val* Y = Op == "Pow" ? &host(N, 1, "the exponent") : nullptr;
        if (Y && Y->count() != 1 && Y->count() != X.count()) fail(N, "constant folding supports equal shapes or a scalar exponent");
        R.dims = X.dims;
        for (size_t K = 0; K < X.count(); ++K) {
            if (X.isInt && X.i[K] == kBatch) fail(N, "arithmetic on the symbolic batch dimension");
            const double A = X.at(K);
            R.f.push_back(Y ? std::pow(A, Y->at(Y->count() == 1 ? 0 : K)) : Op == "Sqrt" ? std::sqrt(A) : Op == "Exp" ? std::exp(A) : Op == "Log" ? std::log(A) : 1.0 / A);
        }
        Out() = R;
        return;
    }
    fail(N, "is applied to constants only; folding it is not supported");
}

// ---- Conv / Gemm / MatMul with their epilogue --------------------------------------------------------------------
void Planner::linear(const Node& N, size_t Index) {
    const Val& X = get(N, 0);
    if (!X.runtime) fail(N, "the data input is a constant");
    const bool Dense = N.Op != "Conv";
    const bool Tok = X.form == kFormToken; // a Linear over tokens: the 1x1 form of the conv, rows = (board, square)
    if (Tok && N.Op != "MatMul") fail(N, "a token tensor " + dimsStr(X.dims) + " feeds MatMul, not " + N.Op);
    int Cin = 0, Cout = 0, KH = 1, KW = 1, DH = 1, DW = 1;
    int CinW = 0;           // input channels per output channel in W: Cin, or 1 for a depthwise conv
    bool Depthwise = false;
    std::vector<double> W, Bias; // W[cout][CinW][taps], taps row-major over (ky, kx)
    std::string Name = N.Name;
    if (!Dense) {
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
        KH = (int)Kh64;
        KW = (int)Kw64;
        DH = KH == 1 ? 1 : (int)std::min<int64_t>(Dil[0], 64); // a dilation along an axis of one tap means nothing
        DW = KW == 1 ? 1 : (int)std::min<int64_t>(Dil[1], 64);
        const int Hy = DH * (KH - 1) / 2, Hx = DW * (KW - 1) / 2;
        if (Hy > kMaxConvHalo || Hx > kMaxConvHalo)
            fail(N, "a " + KStr + " kernel at dilation " + std::to_string(Dil[0]) + "x" + std::to_string(Dil[1]) + " reaches " +
                        std::to_string(std::max(Hy, Hx)) + " squares past the edge: the halo is at most " + std::to_string(kMaxConvHalo));
        if (N.Attrs.count("auto_pad")) fail(N, "auto_pad: only explicit pads");
        const std::vector<int64_t> Pads = N.attrInts("pads", {0, 0, 0, 0});
        if (Pads != std::vector<int64_t>{Hy, Hx, Hy, Hx}) {
            std::string Ps;
            for (int64_t P1 : Pads) Ps += (Ps.empty() ? "" : ",") + std::to_string(P1);
            fail(N, "pads [" + Ps + "] do not keep the 9x9 board: a " + KStr + " kernel at dilation " + std::to_string(DH) + "x" +
                        std::to_string(DW) + " needs [" + std::to_string(Hy) + "," + std::to_string(Hx) + "," + std::to_string(Hy) + "," + std::to_string(Hx) + "]");
        }
        Cout = (int)Wt.dims[0];
        if (X.flatOfSpatial || !isSpatialDims(X.dims)) fail(N, "input " + dimsStr(X.dims) + " is not [N,C,9,9]");
        const int64_t Group = N.attrI("group", 1);
        if (Group == 1) {
            Cin = (int)Wt.dims[1];
        } else {
            // depthwise only: group = Cin = Cout, weight [C,1,kh,kw]
            const int64_t XC = X.dims[1];
            if (Group != XC)
                fail(N, "group " + std::to_string(Group) + " on " + std::to_string(XC) + " input channels: only group 1 or a depthwise conv (group = input channels = output channels)");
            if (Wt.dims[1] != 1) fail(N, "group " + std::to_string(Group) + " with a weight of " + std::to_string(Wt.dims[1]) + " channels per group: a depthwise weight is [C,1,kh,kw]");
            if (Cout != (int)XC)
                fail(N, "a depthwise conv with channel multiplier " + std::to_string(XC > 0 ? Cout / XC : 0) + " (" + std::to_string(XC) + " -> " +
                            std::to_string(Cout) + " channels): only multiplier 1");
            Depthwise = true;
            Cin = (int)XC;
            CinW = 1;
        }
        if ((int)X.dims[1] != Cin)
            fail(N, "the weight expects " + std::to_string(Cin) + " input channels, '" + N.In[0] + "' has " + std::to_string(X.dims[1]));
        if (!Depthwise) CinW = Cin;
        if (Wt.f.size() != (size_t)Cout * CinW * KH * KW) fail(N, "the weight's data does not match its shape");
        W.assign(Wt.f.begin(), Wt.f.end());
        Bias.assign((size_t)Cout, 0.0);
        if (has(N, 2)) {
            const Val& B = host(N, 2, "the bias");
            if ((int)B.count() != Cout) fail(N, "bias length does not match the output channels");
            for (int C = 0; C < Cout; ++C) Bias[(size_t)C] = B.at((size_t)C);
        }
    } else {
        const Val& Wt = host(N, 1, "the weight");
        if (Wt.isInt || Wt.dims.size() != 2) fail(N, "expected a 2-D float weight");
        bool TransB = false;
        if (N.Op == "Gemm") {
            if (N.attrF("alpha", 1.0) != 1.0 || N.attrF("beta", 1.0) != 1.0 || N.attrI("transA", 0) != 0)
                fail(N, "Gemm with alpha = beta = 1, transA = 0 only");
            TransB = N.attrI("transB", 0) != 0;
        }
        Cout = (int)(TransB ? Wt.dims[0] : Wt.dims[1]);
        Cin = (int)(TransB ? Wt.dims[1] : Wt.dims[0]);
        CinW = Cin;
        const int XC = Tok ? (int)X.dims[2] : X.flatOfSpatial ? X.v.C * 81 : flatC(X.dims);
        if (X.dims.size() != 2 && !X.flatOfSpatial && !Tok) fail(N, "input " + dimsStr(X.dims) + " is not 2-D [N,K]");
        if (XC != Cin) fail(N, "the weight expects K = " + std::to_string(Cin) + ", '" + N.In[0] + "' has " + std::to_string(XC));
        W.assign((size_t)Cout * Cin, 0.0);
        for (int O = 0; O < Cout; ++O)
            for (int I = 0; I < Cin; ++I)
                W[(size_t)O * Cin + I] = TransB ? Wt.f[(size_t)O * Cin + I] : Wt.f[(size_t)I * Cout + O];
        Bias.assign((size_t)Cout, 0.0);
        if (N.Op == "Gemm" && has(N, 2)) {
            const Val& B = host(N, 2, "the bias");
            if ((int)B.count() != Cout && B.count() != 1) fail(N, "bias length does not match");
            for (int C = 0; C < Cout; ++C) Bias[(size_t)C] = B.at(B.count() == 1 ? 0 : (size_t)C);
        }
    }
    const int Taps = KH * KW;
    std::vector<int64_t> Dims = Tok ? std::vector<int64_t>{kBatch, 81, Cout}
                                    : Dense ? std::vector<int64_t>{kBatch, Cout} : std::vector<int64_t>{kBatch, Cout, 9, 9};
    const int ChanAxis = Tok ? 2 : 1;
    const int OutForm = Tok ? kFormToken : kFormPlain;
    // epilogue: [BatchNorm | constant per-channel Add]*  [+ runtime residual]  [activation]
    std::string Cur = N.Out[0];
    std::string Res;
    int Act = kActNone;
    size_t At = Index;
    while (absorbable(Cur)) {
        const Node* C = onlyConsumer(Cur, At);
        if (!C) break;
        if (C->Op == "BatchNormalization" && Res.empty() && Act == kActNone && C->In.size() >= 5 && C->In[0] == Cur) {
            bool Const = true;
            for (size_t S = 1; S < 5; ++S) Const = Const && Vals.count(C->In[S]) && !Vals.at(C->In[S]).runtime && Vals.at(C->In[S]).count() == (size_t)Cout;
            if (!Const) break;
            const double Eps = C->attrF("epsilon", 1e-5);
            for (int O = 0; O < Cout; ++O) {
                const double Gm = Vals.at(C->In[1]).at((size_t)O), Bt = Vals.at(C->In[2]).at((size_t)O);
                const double Mn = Vals.at(C->In[3]).at((size_t)O), Vr = Vals.at(C->In[4]).at((size_t)O);
                const double S = Gm / std::sqrt(Vr + Eps);
                for (size_t J = (size_t)O * CinW * Taps; J < (size_t)(O + 1) * CinW * Taps; ++J) W[J] *= S;
                Bias[(size_t)O] = (Bias[(size_t)O] - Mn) * S + Bt;
            }
        } else if (C->Op == "Add" && C->In.size() == 2) {
            const std::string& Other = C->In[0] == Cur ? C->In[1] : C->In[0];
            auto It = Vals.find(Other);
            if (It == Vals.end() || Other == Cur) break;
            const Val& O = It->second;
            if (!O.runtime) { // a per-channel constant: the bias
                if (!Res.empty() || Act != kActNone) break;
                std::vector<int64_t> BD;
                if (!broadcast(Dims, O.dims, &BD) || BD != Dims) break;
                const std::vector<int> Ax = variesAlong(O.dims, Dims.size());
                if (!(Ax.empty() || (Ax.size() == 1 && Ax[0] == ChanAxis))) break;
                for (int Ch = 0; Ch < Cout; ++Ch) Bias[(size_t)Ch] += O.at(Ax.empty() ? 0 : (size_t)Ch);
            } else {
                if (!Res.empty() || Act != kActNone || O.flatOfSpatial || O.dims != Dims || O.form != OutForm) break;
                Res = Other;
            }
        } else if (Act == kActNone && !C->In.empty() && C->In[0] == Cur && nodeAct(*C) != kActNone) {
            Act = nodeAct(*C);
        } else {
            break;
        }
        Name += "+" + C->Name;
        Skip[indexOf(C)] = true;
        At = indexOf(C);
        Cur = C->Out[0];
        if (Act != kActNone) break;
    }
    Launch L;
    L.kind = kLaunchConv;
    L.name = Name;
    L.dense = Dense && !Tok;
    L.depthwise = Depthwise;
    L.taps = Taps;
    L.kh = KH;
    L.kw = KW;
    L.dh = DH;
    L.dw = DW;
    L.in = plain(N.In[0], N.Name + " (input copy)");
    L.cinPad = roundUp(Cin, kChunk);
    L.coutTiles = Depthwise ? 0 : (Cout + kCoutTile - 1) / kCoutTile;
    L.act = Act;
    L.res.buf = kNoRes;
    if (!Res.empty()) L.res = ready(Res).v;
    if (Depthwise) { // per-channel taps packed [chunk][tap][16], BatchNorm folded into them in double
        const int Chunks = L.cinPad / kChunk;
        std::vector<float> Pk((size_t)Chunks * Taps * kChunk, 0.f);
        for (int C = 0; C < Cout; ++C)
            for (int Tp = 0; Tp < Taps; ++Tp)
                Pk[((size_t)(C / kChunk) * Taps + Tp) * kChunk + C % kChunk] = (float)W[(size_t)C * Taps + Tp];
        L.wOff = addConst(Pk);
        std::vector<float> Bf((size_t)L.cinPad, 0.f);
        for (int O = 0; O < Cout; ++O) Bf[(size_t)O] = (float)Bias[(size_t)O];
        L.biasOff = addConst(Bf);
    } else {   // packed [tile][chunk][tap][16][64], f32 of the double product (BatchNorm folded in double)
        const int Chunks = L.cinPad / kChunk;
        std::vector<float> Pk((size_t)L.coutTiles * Chunks * Taps * kChunk * kCoutTile, 0.f);
        for (int T = 0; T < L.coutTiles; ++T)
            for (int Ch = 0; Ch < Chunks; ++Ch)
                for (int Tp = 0; Tp < Taps; ++Tp)
                    for (int Kk = 0; Kk < kChunk; ++Kk)
                        for (int Nn = 0; Nn < kCoutTile; ++Nn) {
                            const int O = T * kCoutTile + Nn, I = Ch * kChunk + Kk;
                            if (O >= Cout || I >= Cin) continue;
                            Pk[((((size_t)T * Chunks + Ch) * Taps + Tp) * kChunk + Kk) * kCoutTile + Nn] =
                                (float)W[((size_t)O * Cin + I) * Taps + Tp];
                        }
        L.wOff = addConst(Pk);
        std::vector<float> Bf((size_t)L.coutTiles * kCoutTile, 0.f);
        for (int O = 0; O < Cout; ++O) Bf[(size_t)O] = (float)Bias[(size_t)O];
        L.biasOff = addConst(Bf);
    }
    L.out = freshView(Cout, !L.dense);
    P.flopsPerPosition += 2.0 * (L.dense ? 1 : 81) * Taps * (double)CinW * Cout;
    Val V = runtimeVal(N, Dims, OutForm);
    V.v = L.out;
    V.producer = N.Name;
    emit(L);
    Vals[Cur] = V;
}

// ---- elementwise ops: fused into groups ------------------------------------------------------------------------
void Planner::elementwise(const Node& N) {
    std::vector<std::vector<int64_t>> InDims;
    std::vector<int64_t> D;
    const std::string& Op = N.Op;
    const bool MinMax = Op == "Max" || Op == "Min";
    if (MinMax && N.In.size() != 2) fail(N, Op + " of " + std::to_string(N.In.size()) + " operands: two only");
    const int ActCode = nodeAct(N);
    const size_t Arity = isBinary(Op) || MinMax || Op == "PRelu" ? 2 : 1;
    if (Op == "PRelu") host(N, 1, "the slope");
    // Pow(x, c) at a constant scalar c, decided here: 2, 3, 4 as products, -0.5 and -2 as a reciprocal behind the square
    // root or the square (0.5 and -1 are activations, 1 never gets here), anything else powf with c as a scalar source
    double PowE = 0;
    if (Op == "Pow") {
        const Val& E = get(N, 1);
        if (E.runtime || E.count() != 1 || (E.isInt && E.i[0] == kBatch)) fail(N, "the exponent must be a constant scalar");
        PowE = E.at(0);
    }
    const bool PowTwoStep = Op == "Pow" && (PowE == 3.0 || PowE == 4.0 || PowE == -0.5 || PowE == -2.0);
    const bool PowGeneral = Op == "Pow" && ActCode == kActNone && PowE != 2.0 && !PowTwoStep;
    // what the node adds to the program behind its operands, beyond one instruction and one register
    const bool ClipLo = Op == "Clip" && (has(N, 1) || N.Attrs.count("min")), ClipHi = Op == "Clip" && (has(N, 2) || N.Attrs.count("max"));
    int XSrcs = 0, XCode = 0, XRegs = 0;
    if (ActCode == kActNone) {
        if (Op == "Clip") XSrcs = ClipLo + ClipHi, XCode = XRegs = 2 * XSrcs;
        else if (Op == "HardSigmoid") XSrcs = 4, XCode = XRegs = 8;
        else if (Op == "LeakyRelu") XSrcs = 1, XCode = XRegs = 2;
        else if (Op == "PRelu") XCode = XRegs = 1; // LeakyRelu's budget; the slope's source and load count as an operand to come
        else if (Op == "BatchNormalization") XSrcs = 2, XCode = XRegs = 3;
        else if (PowTwoStep) XCode = XRegs = 1;
        else if (PowGeneral) XSrcs = 1, XCode = XRegs = 1;
    }
    for (size_t K = 0; K < Arity; ++K) {
        const Val& V = get(N, K);
        std::vector<int64_t> Di = V.runtime && V.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)V.v.C * 81} : V.dims;
        // a PRelu slope [C] on [N,C,9,9] is read per channel, like [C,1,1]
        if (Op == "PRelu" && K == 1 && Di.size() == 1 && D.size() == 4 && Di[0] == D[1] && Di[0] != D[3]) Di = {Di[0], 1, 1};
        std::vector<int64_t> Bd;
        if (K == 0) D = Di;
        else if (!broadcast(D, Di, &Bd)) fail(N, "shapes " + dimsStr(D) + " and " + dimsStr(Di) + " do not broadcast");
        else D = Bd;
        InDims.push_back(Di);
    }
    bool Tok = false; // a token operand makes the result a token tensor
    for (size_t K = 0; K < Arity; ++K) Tok = Tok || (get(N, K).runtime && get(N, K).form == kFormToken);
    if (Tok && !isTokenDims(D)) fail(N, "a token tensor broadcast to " + dimsStr(D));
    const bool Spatial = isSpatialDims(D);
    const int C = Tok ? (int)D[2] : Spatial ? (int)D[1] : flatC(D);
    if (C < 0) fail(N, "output shape " + dimsStr(D) + " is neither [N,C,9,9], a token tensor nor flat");
    const int ChanAxis = Tok ? 2 : 1;
    Group NG;
    NG.spatial = Spatial || Tok;
    NG.C = C;
    NG.name = N.Name;
    NG.out = N.Out[0];
    // operand -> register
    auto operand = [&](size_t K) -> int {
        const std::string& Name = N.In[K];
        Val& V = Vals.at(Name);
        if (!V.runtime) {
            const std::vector<int> Ax = variesAlong(InDims[K], D.size());
            EltSrc S;
            if (Ax.empty()) {
                if (V.count() < 1) fail(N, "empty constant");
                S.mode = kSrcScalar;
                S.scalar = (float)V.at(0);
            } else if (Ax.size() == 1 && Ax[0] == ChanAxis && D.size() >= 2) {
                std::vector<float> F((size_t)C);
                for (int Ch = 0; Ch < C; ++Ch) F[(size_t)Ch] = (float)V.at((size_t)Ch);
                S.mode = kSrcChannel;
                S.constOff = addConst(F);
            } else if ((Tok && Ax == std::vector<int>{1, 2}) || (Spatial && Ax == std::vector<int>{1, 2, 3})) {
                // a learned positional embedding, [81,C] on tokens or [C,9,9] on a spatial tensor: stored [square][C]
                if (V.count() != (size_t)C * 81) fail(N, "constant of shape " + dimsStr(InDims[K]) + " does not cover " + dimsStr(D));
                std::vector<float> F((size_t)C * 81);
                for (int Sq = 0; Sq < 81; ++Sq)
                    for (int Ch = 0; Ch < C; ++Ch)
                        F[(size_t)Sq * C + Ch] = (float)V.at(Tok ? (size_t)Sq * C + Ch : (size_t)Ch * 81 + Sq);
                S.mode = kSrcSquareChannel;
                S.constOff = addConst(F);
            } else {
                fail(N, "constant of shape " + dimsStr(InDims[K]) + " broadcast to " + dimsStr(D) +
                            " (per-channel, per-(square, channel) and scalar constants only)");
            }
            if (NG.srcs.size() >= (size_t)kMaxEltSrcs) fail(N, "too many inputs for one fused launch");
            NG.srcs.push_back(S);
            const int R = NG.nregs++;
            NG.code.push_back(EltInstr{kEltLoad, (uint8_t)R, (uint8_t)(NG.srcs.size() - 1), 0});
            return R;
        }
        // runtime operand: how it varies relative to the output
        const std::vector<int64_t>& Di = InDims[K];
        const bool Same = Tok ? (V.form == kFormToken && Di == D) : (Di == D || (flatC(Di) == C && !Spatial && flatC(D) == C));
        const bool Board = !Tok && Spatial && !V.flatOfSpatial && flatC(Di) == C && Di.size() == 4;
        if (!Same && !Board) fail(N, "operand " + dimsStr(Di) + " broadcast to " + dimsStr(D) + " is not supported");
        // an open group used only here: inline its program
        const Group* Open = V.group >= 0 ? &Groups[(size_t)V.group] : nullptr;
        const bool Domain = Open && !V.flatOfSpatial && Open->C == C &&
                            (Open->spatial == NG.spatial || (Board && !Open->spatial));
        if (Domain && absorbable(Name)) {
            Group& Gr = Groups[(size_t)V.group];
            // inline it only if the rest of the node still fits behind it: every operand still to come takes at least
            // one source and one register (a constant, or a tensor read from memory), then the node's scalars and its
            // own instruction.  Otherwise the group is launched and read as one source, which cuts the chain here.
            const size_t Rest = Arity - 1 - K;
            if (NG.srcs.size() + Gr.srcs.size() + Rest + XSrcs <= (size_t)kMaxEltSrcs &&
                NG.code.size() + Gr.code.size() + 2 + XCode <= (size_t)kMaxEltCode &&
                NG.nregs + Gr.nregs + (int)Rest + 1 + XRegs <= kMaxEltRegs) {
                const int RB = NG.nregs, SB = (int)NG.srcs.size();
                for (EltSrc S : Gr.srcs) {
                    if (Board && S.mode == kSrcSame) S.mode = kSrcBoard;
                    NG.srcs.push_back(S);
                }
                for (EltInstr I : Gr.code) {
                    I.dst = (uint8_t)(I.dst + RB);
                    if (I.op == kEltLoad) I.a = (uint8_t)(I.a + SB);
                    else {
                        I.a = (uint8_t)(I.a + RB);
                        if (I.op != kEltAct) I.b = (uint8_t)(I.b + RB);
                    }
                    NG.code.push_back(I);
                }
                NG.nregs += Gr.nregs;
                NG.name = Gr.name + "+" + NG.name;
                Gr.open = false;
                V.group = -1;
                return RB + Gr.outReg;
            }
        }
        const View Vw = V.flatOfSpatial ? plain(Name, N.Name + " (flatten)") : ready(Name).v;
        if (NG.srcs.size() >= (size_t)kMaxEltSrcs) fail(N, "too many inputs for one fused launch");
        EltSrc S;
        S.mode = Board ? kSrcBoard : kSrcSame;
        S.v = Vw;
        NG.srcs.push_back(S);
        const int R = NG.nregs++;
        NG.code.push_back(EltInstr{kEltLoad, (uint8_t)R, (uint8_t)(NG.srcs.size() - 1), 0});
        return R;
    };
    auto scalarReg = [&](double Value) -> int {
        if (NG.srcs.size() >= (size_t)kMaxEltSrcs) fail(N, "too many inputs for one fused launch");
        EltSrc S;
        S.mode = kSrcScalar;
        S.scalar = (float)Value;
        NG.srcs.push_back(S);
        const int R = NG.nregs++;
        NG.code.push_back(EltInstr{kEltLoad, (uint8_t)R, (uint8_t)(NG.srcs.size() - 1), 0});
        return R;
    };
    auto instr = [&](int Code, int A, int B) -> int {
        const int R = NG.nregs++;
        NG.code.push_back(EltInstr{(uint8_t)Code, (uint8_t)R, (uint8_t)A, (uint8_t)B});
        return R;
    };
    auto bound = [&](size_t Idx, const char* Attr, const char* What) -> double {
        if (!has(N, Idx)) return N.attrF(Attr, 0.0);
        const Val& B = host(N, Idx, What);
        if (B.count() != 1 || (B.isInt && B.i[0] == kBatch)) fail(N, std::string(What) + " must be a scalar constant");
        return B.at(0);
    };
    int Out;
    if (ActCode != kActNone) {
        Out = instr(kEltAct, operand(0), ActCode);
    } else if (isBinary(Op) || MinMax) {
        const int A = operand(0), B = operand(1);
        Out = instr(Op == "Add" ? kEltAdd : Op == "Sub" ? kEltSub : Op == "Mul" ? kEltMul : Op == "Div" ? kEltDiv : Op == "Max" ? kEltMax : kEltMin, A, B);
    } else if (Op == "Clip") { // min(max(x, lo), hi), either bound optional
        Out = operand(0);
        if (ClipLo) Out = instr(kEltMax, Out, scalarReg(bound(1, "min", "Clip's lower bound")));
        if (ClipHi) Out = instr(kEltMin, Out, scalarReg(bound(2, "max", "Clip's upper bound")));
    } else if (Op == "HardSigmoid") { // min(max(alpha x + beta, 0), 1) at any alpha and beta
        Out = operand(0); // before the scalars: the operand's budget counts them as still to come
        Out = instr(kEltMul, Out, scalarReg(N.attrF("alpha", 0.2)));
        Out = instr(kEltAdd, Out, scalarReg(N.attrF("beta", 0.5)));
        Out = instr(kEltMax, Out, scalarReg(0.0));
        Out = instr(kEltMin, Out, scalarReg(1.0));
    } else if (Op == "LeakyRelu") {
        Out = operand(0);
        Out = instr(kEltLeaky, Out, scalarReg(N.attrF("alpha", 0.01)));
    } else if (Op == "PRelu") { // the slope: a scalar or per-channel constant, loaded like any constant operand
        const int A = operand(0), B = operand(1);
        Out = instr(kEltLeaky, A, B);
    } else if (Op == "Abs" || Op == "Neg") {
        Out = instr(Op == "Abs" ? kEltAbs : kEltNeg, operand(0), 0);
    } else if (Op == "Pow") {
        const int A = operand(0);
        if (PowE == 2.0) {
            Out = instr(kEltMul, A, A);
        } else if (PowE == 3.0) {
            const int Sq = instr(kEltMul, A, A);
            Out = instr(kEltMul, Sq, A);
        } else if (PowE == 4.0) {
            const int Sq = instr(kEltMul, A, A);
            Out = instr(kEltMul, Sq, Sq);
        } else if (PowE == -0.5) {
            const int Rt = instr(kEltAct, A, kActSqrt);
            Out = instr(kEltAct, Rt, kActRecip);
        } else if (PowE == -2.0) {
            const int Sq = instr(kEltMul, A, A);
            Out = instr(kEltAct, Sq, kActRecip);
        } else {
            Out = instr(kEltPow, A, scalarReg(PowE));
        }
    } else { // BatchNormalization on a runtime tensor: y = x * s + t per channel
        if (N.In.size() < 5) fail(N, "expected scale, bias, mean and variance");
        const double Eps = N.attrF("epsilon", 1e-5);
        std::vector<float> Sc((size_t)C), Sh((size_t)C);
        for (size_t S = 1; S < 5; ++S)
            if (host(N, S, "a BatchNormalization statistic").count() != (size_t)C) fail(N, "statistic length does not match the channels");
        for (int Ch = 0; Ch < C; ++Ch) {
            const double Gm = get(N, 1).at((size_t)Ch), Bt = get(N, 2).at((size_t)Ch);
            const double Mn = get(N, 3).at((size_t)Ch), Vr = get(N, 4).at((size_t)Ch);
            const double S = Gm / std::sqrt(Vr + Eps);
            Sc[(size_t)Ch] = (float)S;
            Sh[(size_t)Ch] = (float)(Bt - Mn * S);
        }
        const int A = operand(0);
        EltSrc S1, S2;
        S1.mode = S2.mode = kSrcChannel;
        S1.constOff = addConst(Sc);
        S2.constOff = addConst(Sh);
        if (NG.srcs.size() + 2 > (size_t)kMaxEltSrcs) fail(N, "too many inputs for one fused launch");
        NG.srcs.push_back(S1);
        NG.srcs.push_back(S2);
        const int RS = NG.nregs++, RT = NG.nregs++, RM = NG.nregs++;
        Out = NG.nregs++;
        NG.code.push_back(EltInstr{kEltLoad, (uint8_t)RS, (uint8_t)(NG.srcs.size() - 2), 0});
        NG.code.push_back(EltInstr{kEltLoad, (uint8_t)RT, (uint8_t)(NG.srcs.size() - 1), 0});
        NG.code.push_back(EltInstr{kEltMul, (uint8_t)RM, (uint8_t)A, (uint8_t)RS});
        NG.code.push_back(EltInstr{kEltAdd, (uint8_t)Out, (uint8_t)RM, (uint8_t)RT});
    }
    if (NG.nregs > kMaxEltRegs || NG.code.size() > (size_t)kMaxEltCode) fail(N, "elementwise chain too long for one launch");
    NG.outReg = Out;
    Groups.push_back(NG);
    Val V = runtimeVal(N, D, Tok ? kFormToken : kFormPlain);
    V.group = (int)Groups.size() - 1;
    V.v.buf = kPending;
    V.v.C = C;
    V.v.spatial = NG.spatial;
    V.v.stride = roundUp(std::max(C, 1), kChunk);
    Vals[N.Out[0]] = V;
}

// ---- LayerNormalization over the channels of a token tensor or of a flat [N,C] tensor ------------------------------
void Planner::layerNorm(const Node& N) {
    const Val& X = get(N, 0);
    const bool Tok = X.form == kFormToken || X.form == kFormChanLast;
    if (!Tok && (X.form != kFormPlain || X.flatOfSpatial || X.dims.size() != 2 || flatC(X.dims) < 0))
        fail(N, "input " + dimsStr(X.dims) + " is neither a token tensor [N,81,C], a channel-last view [N,9,9,C] nor flat [N,C]");
    const int64_t Rank = (int64_t)X.dims.size();
    int64_t Axis = N.attrI("axis", -1);
    if (Axis < 0) Axis += Rank;
    if (Axis != Rank - 1) fail(N, "LayerNormalization over the last axis (the channels) only");
    const int C = (int)X.dims[(size_t)Rank - 1];
    const Val& Sc = host(N, 1, "the scale");
    if (Sc.count() != (size_t)C) fail(N, "scale length does not match the channels");
    std::vector<float> Gm((size_t)C), Bt((size_t)C, 0.f);
    for (int Ch = 0; Ch < C; ++Ch) Gm[(size_t)Ch] = (float)Sc.at((size_t)Ch);
    if (has(N, 2)) {
        const Val& B = host(N, 2, "the bias");
        if (B.count() != (size_t)C) fail(N, "bias length does not match the channels");
        for (int Ch = 0; Ch < C; ++Ch) Bt[(size_t)Ch] = (float)B.at((size_t)Ch);
    }
    if (N.Out.size() > 1 && !N.Out[1].empty() && Uses.count(N.Out[1])) fail(N, "the mean / inverse-deviation outputs are not supported");
    Launch L;
    L.kind = kLaunchLayerNorm;
    L.name = N.Name;
    L.in = ready(N.In[0]).v;
    L.out = freshView(C, Tok);
    L.wOff = addConst(Gm);
    L.biasOff = addConst(Bt);
    L.eps = (float)N.attrF("epsilon", 1e-5);
    Val V = runtimeVal(N, X.dims, X.form);
    V.v = L.out;
    emit(L);
    Vals[N.Out[0]] = V;
}

// ---- GroupNorm / InstanceNorm: one kLaunchGroupNorm.  `Last` is the node whose output the normalised [N,C,9,9] tensor
// is (the InstanceNormalization itself, or the Reshape that closes the GroupNorm pattern); A, B: the
// InstanceNormalization's constants per group.  While each tensor has one consumer, a constant per-channel Mul and Add
// (either operand order) fold in double into gamma and beta, and at most one parameter-free activation joins.
void Planner::groupNorm(const Node& Last, size_t Index, const View& In, int C, int G, const std::vector<double>& A,
                        const std::vector<double>& B, double Eps, std::string Name) {
    const int Cg = C / G;
    std::vector<double> Gm((size_t)C), Bt((size_t)C);
    for (int Ch = 0; Ch < C; ++Ch) {
        Gm[(size_t)Ch] = A[(size_t)(Ch / Cg)];
        Bt[(size_t)Ch] = B[(size_t)(Ch / Cg)];
    }
    const std::vector<int64_t> Dims = {kBatch, C, 9, 9};
    std::string Cur = Last.Out[0];
    size_t At = Index;
    int Act = kActNone;
    while (absorbable(Cur) && Act == kActNone) {
        const Node* Nx = onlyConsumer(Cur, At);
        if (!Nx) break;
        if ((Nx->Op == "Mul" || Nx->Op == "Add") && Nx->In.size() == 2 && Nx->In[0] != Nx->In[1]) {
            auto It = Vals.find(Nx->In[0] == Cur ? Nx->In[1] : Nx->In[0]);
            if (It == Vals.end() || It->second.runtime || It->second.isInt) break;
            const Val& O = It->second;
            std::vector<int64_t> BD;
            if (!broadcast(Dims, O.dims, &BD) || BD != Dims) break;
            const std::vector<int> Ax = variesAlong(O.dims, 4);
            if (!(Ax.empty() || (Ax.size() == 1 && Ax[0] == 1)) || O.count() != (Ax.empty() ? 1u : (size_t)C)) break;
            for (int Ch = 0; Ch < C; ++Ch) {
                const double K = O.at(Ax.empty() ? 0 : (size_t)Ch);
                if (Nx->Op == "Mul") { Gm[(size_t)Ch] *= K; Bt[(size_t)Ch] *= K; }
                else Bt[(size_t)Ch] += K;
            }
        } else if (!Nx->In.empty() && Nx->In[0] == Cur && nodeAct(*Nx) != kActNone) {
            Act = nodeAct(*Nx);
        } else {
            break;
        }
        Name += "+" + Nx->Name;
        Skip[indexOf(Nx)] = true;
        At = indexOf(Nx);
        Cur = Nx->Out[0];
    }
    Launch L;
    L.kind = kLaunchGroupNorm;
    L.name = Name;
    L.in = In; // a view at any channel offset: the kernel reads it where it lies
    L.groups = G;
    L.act = Act;
    L.eps = (float)Eps;
    L.wOff = addConst(std::vector<float>(Gm.begin(), Gm.end()));
    L.biasOff = addConst(std::vector<float>(Bt.begin(), Bt.end()));
    L.out = freshView(C, true);
    Val V = runtimeVal(Last, Dims);
    V.v = L.out;
    emit(L);
    Vals[Cur] = V;
}

// ReduceMean over the last axis (given as -1 or as rank - 1) with keepdims = 1
bool Planner::lastAxis(const Node& N, const Val& X) {
    if (has(N, 1) && Vals.count(N.In[1]) && Vals.at(N.In[1]).runtime) return false;
    std::vector<int64_t> Axes = has(N, 1) ? ints(N, 1, "axes") : N.attrInts("axes", {});
    const int64_t Rank = (int64_t)X.dims.size();
    return Axes.size() == 1 && (Axes[0] < 0 ? Axes[0] + Rank : Axes[0]) == Rank - 1 && N.attrI("keepdims", 1) != 0;
}

// The one node that reads the interior tensor T of a decomposed normalisation; a second reader, or T as a graph output,
// is refused at that reader (at `From`, T's producer, when there is none to name).
const Node* Planner::follow(const std::string& T, size_t After, const Node& From) {
    std::vector<const Node*> Cs;
    for (size_t K = After + 1; K < Nodes.size(); ++K)
        if (!Skip[K] && std::count(Nodes[K].In.begin(), Nodes[K].In.end(), T)) Cs.push_back(&Nodes[K]);
    const std::string What = "'" + T + "' is an interior tensor of the decomposed normalisation that starts at '" + From.Name +
                             "' (DESIGN.md section 13.3)";
    if (Outputs.count(T)) fail(From, What + " and a graph output");
    if (Cs.empty()) fail(From, What + " and is never read");
    if (Cs.size() > 1) fail(*Cs[1], What + ": only the pattern's own nodes read it");
    return Cs[0];
}

// LayerNorm and RMSNorm written out in elementary ops, over the last axis of a token, flat or channel-last tensor:
//   LayerNorm  m = ReduceMean(x); d = Sub(x, m); v = ReduceMean(square(d)); y = d / Sqrt(Add(v, eps)) [* gamma] [+ beta]
//   RMSNorm    v = ReduceMean(square(x));                                   y = x / Sqrt(Add(v, eps)) [* gamma]
// square(t) is Pow(t, 2) or Mul(t, t); t / s is Div(t, s), or Div(1, s) followed by Mul with t.  Matched forward from the
// first node; the rest is absorbed (Skip) into one kLaunchLayerNorm / kLaunchRmsNorm.  Returns false when N starts no
// such chain; a chain that starts and then deviates is refused at the deviating node.
bool Planner::decomposedNorm(const Node& N, size_t Index) {
    const bool Mean = N.Op == "ReduceMean";
    if (!Mean && N.Op != "Pow" && !(N.Op == "Mul" && N.In.size() == 2 && N.In[0] == N.In[1])) return false;
    const Val& X0 = get(N, 0);
    if (!X0.runtime) return false;
    if (X0.form != kFormToken && X0.form != kFormChanLast &&
        !(X0.form == kFormPlain && !X0.flatOfSpatial && X0.dims.size() == 2 && flatC(X0.dims) > 0))
        return false;
    const std::string Where = " in the decomposed normalisation that starts at '" + N.Name + "' (DESIGN.md section 13.3)";
    auto square = [&](const Node& S, const std::string& T) {
        double E = 0;
        if (S.Op == "Pow") return S.In.size() == 2 && S.In[0] == T && scalarAhead(S.In[1], &E) && E == 2.0;
        return S.Op == "Mul" && S.In.size() == 2 && S.In[0] == T && S.In[1] == T;
    };
    std::vector<const Node*> Absorbed;
    std::string Base;        // the tensor that is squared and divided: x - mean, or x
    const Node* Mn = nullptr; // the ReduceMean of the squares
    const Node* Closing = nullptr; // LayerNorm: the other reader of x - mean
    if (Mean) {
        if (!lastAxis(N, X0) || Outputs.count(N.Out[0]) || Uses[N.Out[0]] != 1) return false;
        const Node* Sub = onlyConsumer(N.Out[0], Index);
        if (!Sub || Sub->Op != "Sub" || Sub->In.size() != 2 || Sub->In[0] != N.In[0] || Sub->In[1] != N.Out[0]) return false;
        Base = Sub->Out[0];
        std::vector<const Node*> Rd;
        for (size_t K = indexOf(Sub) + 1; K < Nodes.size(); ++K)
            if (!Skip[K] && std::count(Nodes[K].In.begin(), Nodes[K].In.end(), Base)) Rd.push_back(&Nodes[K]);
        if (Outputs.count(Base) || Rd.size() < 2) fail(*Sub, "x - mean" + Where + " is read by its square and by the division, nothing else");
        if (Rd.size() > 2) fail(*Rd[2], "reads x - mean" + Where + ": only its square and the division do");
        if (!square(*Rd[0], Base)) fail(*Rd[0], "follows x - mean" + Where + ": expected its square, Pow(d, 2) or Mul(d, d)");
        Closing = Rd[1];
        Mn = follow(Rd[0]->Out[0], indexOf(Rd[0]), *Rd[0]);
        if (Mn->Op != "ReduceMean" || !lastAxis(*Mn, X0)) fail(*Mn, "follows the square" + Where + ": expected ReduceMean over the last axis with keepdims = 1");
        Absorbed = {Sub, Rd[0], Mn};
    } else {
        if (!square(N, N.In[0]) || Outputs.count(N.Out[0]) || Uses[N.Out[0]] != 1) return false;
        Mn = onlyConsumer(N.Out[0], Index);
        if (!Mn || Mn->Op != "ReduceMean" || !lastAxis(*Mn, X0)) return false;
        Base = N.In[0];
        Absorbed = {Mn};
    }
    const Node* Ad = follow(Mn->Out[0], indexOf(Mn), *Mn);
    double Eps = 0;
    if (Ad->Op != "Add" || Ad->In.size() != 2 || !scalarAhead(Ad->In[0] == Mn->Out[0] ? Ad->In[1] : Ad->In[0], &Eps))
        fail(*Ad, "follows the mean of squares" + Where + ": expected Add of a constant scalar epsilon");
    const Node* Sr = follow(Ad->Out[0], indexOf(Ad), *Ad);
    if (Sr->Op != "Sqrt") fail(*Sr, "follows the Add of epsilon" + Where + ": expected Sqrt");
    const Node* Dv = follow(Sr->Out[0], indexOf(Sr), *Sr);
    if (Dv->Op != "Div" || Dv->In.size() != 2 || Dv->In[1] != Sr->Out[0]) fail(*Dv, "follows the Sqrt" + Where + ": expected a division by it");
    Absorbed.insert(Absorbed.end(), {Ad, Sr, Dv});
    const Node* Y = Dv;
    double One = 0;
    if (Dv->In[0] != Base) {
        if (!scalarAhead(Dv->In[0], &One) || One != 1.0) fail(*Dv, "divides neither the normalised tensor nor 1 by the deviation" + Where);
        Y = follow(Dv->Out[0], indexOf(Dv), *Dv);
        if (Y->Op != "Mul" || Y->In.size() != 2 || (Y->In[0] == Dv->Out[0] ? Y->In[1] : Y->In[0]) != Base)
            fail(*Y, "follows the reciprocal deviation" + Where + ": expected its product with the tensor that was squared");
        Absorbed.push_back(Y);
    }
    if (Closing && Closing != Y) fail(*Closing, "reads x - mean" + Where + ": only its square and the division do");
    // gamma and beta: constants over the last axis, either operand order, both optional
    const int C = (int)X0.dims.back();
    std::vector<float> Gm((size_t)C, 1.f), Bt((size_t)C, 0.f);
    auto affine = [&](const char* OpName, std::vector<float>& Dst) {
        const std::string& Cur = Y->Out[0];
        if (!absorbable(Cur)) return;
        const Node* Nx = onlyConsumer(Cur, indexOf(Y));
        if (!Nx || Nx->Op != OpName || Nx->In.size() != 2 || Nx->In[0] == Nx->In[1]) return;
        auto It = Vals.find(Nx->In[0] == Cur ? Nx->In[1] : Nx->In[0]);
        if (It == Vals.end() || It->second.runtime || It->second.isInt) return;
        const Val& O = It->second;
        const std::vector<int> Ax = variesAlong(O.dims, X0.dims.size());
        if (O.count() != (size_t)C || O.dims.empty() || !(C == 1 || (Ax.size() == 1 && Ax[0] == (int)X0.dims.size() - 1))) return;
        for (int Ch = 0; Ch < C; ++Ch) Dst[(size_t)Ch] = (float)O.at((size_t)Ch);
        Absorbed.push_back(Nx);
        Y = Nx;
    };
    affine("Mul", Gm);
    if (Mean) affine("Add", Bt);
    Launch L;
    L.kind = Mean ? kLaunchLayerNorm : kLaunchRmsNorm;
    L.name = N.Name;
    for (const Node* A : Absorbed) {
        L.name += "+" + A->Name;
        Skip[indexOf(A)] = true;
    }
    L.in = ready(N.In[0]).v;
    L.out = freshView(C, X0.form != kFormPlain);
    L.wOff = addConst(Gm);
    if (Mean) L.biasOff = addConst(Bt);
    L.eps = (float)Eps;
    Val V = runtimeVal(*Y, X0.dims, X0.form);
    V.v = L.out;
    emit(L);
    Vals[Y->Out[0]] = V;
    return true;
}

// ---- the normalisations beyond BatchNorm and the single LayerNormalization node.  Returns false when N is none.
bool Planner::normOp(const Node& N, size_t Index) {
    if (N.Op == "LayerNormalization" && get(N, 0).runtime && get(N, 0).form == kFormChanLast) {
        layerNorm(N);
        return true;
    }
    if (N.Op != "InstanceNormalization") return decomposedNorm(N, Index);
    const Val& X = get(N, 0);
    if (!X.runtime) fail(N, "the data input is a constant");
    const bool Groups = X.form == kFormGroup3 || X.form == kFormChan3;
    const bool Spatial = X.form == kFormPlain && !X.flatOfSpatial && isSpatialDims(X.dims);
    if (!Groups && !Spatial)
        fail(N, "input " + dimsStr(X.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)X.v.C * 81} : X.dims) +
                    " is neither [N,C,9,9] nor the groups [N,G,M] of a GroupNorm pattern: InstanceNormalization runs on a spatial tensor only");
    if (X.normG > 0) fail(N, "'" + N.In[0] + "' is normalised already: only the Reshape back to [N,C,9,9] reads it");
    const int G = (int)X.dims[1];
    const Val& Sc = host(N, 1, "the scale");
    const Val& Bi = host(N, 2, "the bias");
    if (Sc.isInt || Bi.isInt || Sc.count() != (size_t)G || Bi.count() != (size_t)G)
        fail(N, "scale and bias of length " + std::to_string(G) + " expected, one value per " + (Groups ? "group" : "channel"));
    std::vector<double> A(Sc.f.begin(), Sc.f.end()), B(Bi.f.begin(), Bi.f.end());
    const double Eps = N.attrF("epsilon", 1e-5);
    if (Spatial) {
        groupNorm(N, Index, ready(N.In[0]).v, G, G, A, B, Eps, N.Name);
        return true;
    }
    Val V = X; // [N,G,M] stays a view of the spatial rows; the launch is emitted at the Reshape back
    V.normG = G;
    V.normA = A;
    V.normB = B;
    V.normEps = Eps;
    V.producer = N.Name;
    V.chain = N.Name;
    Vals[N.Out[0]] = V;
    return true;
}

// The dims a Reshape of a tensor of dims SD produces (batch symbolic).
std::vector<int64_t> Planner::reshapeTarget(const Node& N, const std::vector<int64_t>& SD) {
    int64_t Rest = 1;
    for (size_t J = 1; J < SD.size(); ++J) Rest *= SD[J];
    std::vector<int64_t> ND;
    const std::vector<int64_t> Sh = ints(N, 1, "the target shape");
    int64_t Known = 1;
    int Infer = -1;
    ND.assign(Sh.size(), 0);
    for (size_t J = 0; J < Sh.size(); ++J) {
        int64_t V = Sh[J];
        if (V == 0 && J < SD.size()) V = SD[J];
        if (V == -1) { Infer = (int)J; continue; }
        ND[J] = V;
        if (V != kBatch) Known *= V;
    }
    const bool HasBatch = std::count(ND.begin(), ND.end(), kBatch) == 1;
    if (Infer >= 0) {
        if (HasBatch) {
            if (Known <= 0 || Rest % Known) fail(N, "cannot infer the -1 dimension");
            ND[(size_t)Infer] = Rest / Known;
        } else {
            if (Known != Rest) fail(N, "reshape would mix boards");
            ND[(size_t)Infer] = kBatch;
        }
    }
    if (ND.empty() || ND[0] != kBatch) fail(N, "the target shape " + dimsStr(ND) + " does not keep the batch first");
    int64_t NR = 1;
    for (size_t J = 1; J < ND.size(); ++J) NR *= ND[J];
    if (NR != Rest) fail(N, "element count changes: " + dimsStr(SD) + " -> " + dimsStr(ND));
    return ND;
}

// ---- views between [N,C,9,9], [N,C,81], tokens [N,81,C] and the attention pattern's 4-D shapes: no launch, except
// the Reshape that closes the attention pattern.  Returns false when N is not such a view (the caller goes on).
bool Planner::formView(const Node& N) {
    const std::string& Op = N.Op;
    if (Op != "Transpose" && Op != "Reshape" && Op != "Flatten" && Op != "Identity") return false;
    const Val& X0 = get(N, 0);
    if (!X0.runtime) return false;
    if (Op == "Identity") {
        if (X0.form == kFormPlain) return false;
        if (X0.form >= kFormChan3) interior(N, 0);
        Val V = ready(N.In[0]);
        Vals[N.Out[0]] = V;
        return true;
    }
    if (X0.normG > 0 && Op != "Reshape")
        fail(N, "'" + N.In[0] + "' " + dimsStr(X0.dims) + " is the normalised tensor of a GroupNorm pattern: only the Reshape back to [N,C,9,9] reads it (DESIGN.md section 13.3)");
    const std::vector<int64_t> Perm = N.attrInts("perm", {});
    auto set = [&](Val V, int Form, std::vector<int64_t> Dims) {
        V.form = Form;
        V.dims = std::move(Dims);
        V.producer = N.Name;
        V.chain += (V.chain.empty() ? "" : "+") + N.Name;
        Vals[N.Out[0]] = V;
        return true;
    };
    if (Op == "Transpose") {
        const int F = X0.form;
        // the channel-last view of a spatial tensor and the way back: the same rows, no launch
        if (F == kFormPlain && !X0.flatOfSpatial && isSpatialDims(X0.dims) && Perm == std::vector<int64_t>{0, 2, 3, 1}) {
            Val V = ready(N.In[0]);
            V.chain.clear();
            return set(V, kFormChanLast, {kBatch, 9, 9, X0.dims[1]});
        }
        if (F == kFormChanLast) {
            if (Perm != std::vector<int64_t>{0, 3, 1, 2})
                fail(N, "Transpose of the channel-last view " + dimsStr(X0.dims) + " with perm " + dimsStr(Perm) + ": only [0,3,1,2], back to [N,C,9,9]");
            Val V = X0;
            V.chain.clear();
            return set(V, kFormPlain, {kBatch, X0.dims[3], 9, 9});
        }
        if (F == kFormGroup3) fail(N, "Transpose of " + dimsStr(X0.dims) + ": the groups [N,G,M] of a GroupNorm pattern feed an InstanceNormalization only");
        if (F == kFormPlain) return false; // refused by the caller, with the shapes
        if (F >= kFormChan3) interior(N, 0);
        const Val X = F == kFormToken ? ready(N.In[0]) : X0;
        const std::vector<int64_t>& D = X.dims;
        if ((F == kFormToken || F == kFormChan3) && Perm == std::vector<int64_t>{0, 2, 1}) {
            Val V = X;
            V.chain.clear();
            return set(V, F == kFormToken ? kFormChan3 : kFormToken, {kBatch, D[2], D[1]});
        }
        if (F == kFormTok4 && Perm == std::vector<int64_t>{0, 2, 1, 3}) return set(X, kFormHeads, {kBatch, D[2], 81, D[3]});
        if (F == kFormTok4 && Perm == std::vector<int64_t>{0, 2, 3, 1}) return set(X, kFormHeadsT, {kBatch, D[2], D[3], 81});
        if (F == kFormHeads && Perm == std::vector<int64_t>{0, 1, 3, 2}) return set(X, kFormHeadsT, {kBatch, D[1], D[3], 81});
        if (F == kFormHeadOut && Perm == std::vector<int64_t>{0, 2, 1, 3}) return set(X, kFormTokOut4, {kBatch, 81, D[1], D[3]});
        fail(N, "Transpose of " + dimsStr(D) + " with perm " + dimsStr(Perm) + " is outside the token-view and attention patterns (DESIGN.md section 13.3)");
    }
    // Reshape / Flatten
    const int F = X0.form;
    const bool PlainSpatial = F == kFormPlain && !X0.flatOfSpatial && isSpatialDims(X0.dims);
    if (F == kFormPlain && !PlainSpatial) return false;
    if (PlainSpatial) {
        // only Reshape to [N,C,81] is taken here (torch's flatten(2)); every other view is the existing code's.  ONNX's
        // own Flatten with axis 2 gives [N*C,81], which mixes boards, and is refused there.
        if (Op != "Reshape") return false;
        const Val& ShV = get(N, 1);
        if (ShV.runtime || ShV.count() != 3) return false;
        const std::vector<int64_t> ND = reshapeTarget(N, X0.dims);
        if (ND != std::vector<int64_t>{kBatch, X0.dims[1], 81}) {
            // [N,G,M] with G M = C 81 in front of an InstanceNormalization: the groups of a GroupNorm
            if (ND[1] <= 0 || ND[2] <= 0 || ND[1] * ND[2] != X0.dims[1] * 81) return false;
            bool Norm = false;
            for (size_t K = indexOf(&N) + 1; K < Nodes.size(); ++K)
                Norm = Norm || (!Skip[K] && Nodes[K].Op == "InstanceNormalization" && !Nodes[K].In.empty() && Nodes[K].In[0] == N.Out[0]);
            if (!Norm) return false;
            if (X0.dims[1] % ND[1] != 0)
                fail(N, "a GroupNorm of " + std::to_string(ND[1]) + " groups over " + std::to_string(X0.dims[1]) + " channels: the group count does not divide the channels");
            Val V = ready(N.In[0]);
            V.chain.clear();
            return set(V, kFormGroup3, ND);
        }
        Val V = ready(N.In[0]);
        V.chain.clear();
        return set(V, kFormChan3, ND);
    }
    if (Op == "Flatten" && !(F == kFormChan3 && N.attrI("axis", 1) == 1))
        fail(N, "Flatten of " + dimsStr(X0.dims) + " is outside the token-view patterns");
    if (X0.normG > 0) { // the Reshape that closes the GroupNorm pattern: one launch, with what follows it
        const std::vector<int64_t> Back = reshapeTarget(N, X0.dims);
        if (Back != std::vector<int64_t>{kBatch, (int64_t)X0.v.C, 9, 9})
            fail(N, "the normalised groups " + dimsStr(X0.dims) + " are reshaped to " + dimsStr(Back) + ", not back to [N," + std::to_string(X0.v.C) + ",9,9]");
        groupNorm(N, indexOf(&N), X0.v, X0.v.C, X0.normG, X0.normA, X0.normB, X0.normEps, X0.chain + "+" + N.Name);
        return true;
    }
    if (F == kFormGroup3) fail(N, "Reshape of " + dimsStr(X0.dims) + ": the groups [N,G,M] of a GroupNorm pattern feed an InstanceNormalization only");
    if (F == kFormChanLast) fail(N, "Reshape of the channel-last view " + dimsStr(X0.dims) + ": only a LayerNorm over the channels and Transpose [0,3,1,2] read it");
    if (F >= kFormChan3) interior(N, 0);
    const std::vector<int64_t> ND = Op == "Flatten" ? std::vector<int64_t>{kBatch, X0.dims[1] * 81} : reshapeTarget(N, X0.dims);
    if (F == kFormChan3) { // the way back: [N,C,81] -> [N,C,9,9] or the flattened [N,C*81]
        Val V = X0;
        V.form = kFormPlain;
        V.producer = N.Name;
        V.chain.clear();
        if (isSpatialDims(ND) && ND[1] == X0.dims[1]) V.dims = ND;
        else if (ND == std::vector<int64_t>{kBatch, X0.dims[1] * 81}) { V.dims = {kBatch, X0.dims[1], 9, 9}; V.flatOfSpatial = true; }
        else fail(N, "a [N,C,81] tensor can become [N,C,9,9] or [N,C*81], not " + dimsStr(ND));
        Vals[N.Out[0]] = V;
        return true;
    }
    if (F == kFormToken) {
        if (ND == X0.dims) { Val V = ready(N.In[0]); V.producer = N.Name; Vals[N.Out[0]] = V; return true; }
        const int C = (int)X0.dims[2];
        if (ND.size() != 4 || ND[1] != 81 || ND[2] <= 0 || ND[3] <= 0 || ND[2] * ND[3] != C)
            fail(N, "a token tensor " + dimsStr(X0.dims) + " can be split into heads [N,81,H,d], not reshaped to " + dimsStr(ND));
        const int64_t Hd = ND[3];
        if (Hd % 4 != 0 || Hd > kMaxHeadDim)
            fail(N, "head dimension " + std::to_string(Hd) + ": the attention kernel takes multiples of 4 up to " + std::to_string(kMaxHeadDim));
        // q * scale (or k * scale) right before the split: an open group of one scalar Mul / Div is folded into the scale
        Val V;
        bool Peeled = false;
        if (X0.group >= 0 && absorbable(N.In[0])) {
            const Group& Gr = Groups[(size_t)X0.group];
            if (Gr.open && Gr.srcs.size() == 2 && Gr.code.size() == 3 && Gr.code[0].op == kEltLoad && Gr.code[1].op == kEltLoad &&
                (Gr.code[2].op == kEltMul || Gr.code[2].op == kEltDiv)) {
                const int A = Gr.code[2].a, B = Gr.code[2].b; // registers loaded by code[0] and code[1]
                const EltSrc& SA = Gr.srcs[Gr.code[A == Gr.code[0].dst ? 0 : 1].a];
                const EltSrc& SB = Gr.srcs[Gr.code[B == Gr.code[0].dst ? 0 : 1].a];
                const bool Mul = Gr.code[2].op == kEltMul;
                const EltSrc* Rt = SA.mode == kSrcSame ? &SA : (Mul && SB.mode == kSrcSame) ? &SB : nullptr;
                const EltSrc* Cs = Rt == &SA ? &SB : &SA;
                if (A != B && Rt && Cs->mode == kSrcScalar && Gr.outReg == Gr.code[2].dst) {
                    V = X0;
                    V.group = -1;
                    V.v = Rt->v;
                    V.scale = Mul ? (double)Cs->scalar : 1.0 / (double)Cs->scalar;
                    V.chain = Gr.name;
                    Groups[(size_t)X0.group].open = false;
                    Peeled = true;
                }
            }
        }
        if (!Peeled) {
            V = ready(N.In[0]);
            V.scale = 1.0;
            V.chain.clear();
        }
        if (V.v.offset % 4 != 0) fail(N, "'" + N.In[0] + "' starts at channel " + std::to_string(V.v.offset) + " of its row: the attention kernel reads views at multiples of 4");
        return set(V, kFormTok4, ND);
    }
    if (F == kFormTokOut4) { // the Reshape that closes the pattern: one launch
        const int64_t H = X0.dims[2], Hd = X0.dims[3];
        if (ND != std::vector<int64_t>{kBatch, 81, H * Hd})
            fail(N, "the attention output " + dimsStr(X0.dims) + " is reshaped to " + dimsStr(ND) + ", not to [N,81,H*d]");
        Launch L;
        L.kind = kLaunchAttention;
        L.name = X0.chain + "+" + N.Name;
        L.in = X0.attQ;
        L.attK = X0.attK;
        L.attV = X0.attV;
        L.heads = (int)H;
        L.headDim = (int)Hd;
        L.scale = (float)X0.scale;
        L.hasBias = !X0.bias.empty();
        if (L.hasBias) {
            std::vector<float> Bf(X0.bias.begin(), X0.bias.end());
            L.biasOff = addConst(Bf);
        }
        L.out = freshView((int)(H * Hd), true);
        P.flopsPerPosition += 2.0 * (2.0 * 81 * 81 * (double)Hd) * (double)H; // q k^T and probs x v
        Val V = runtimeVal(N, ND, kFormToken);
        V.v = L.out;
        emit(L);
        Vals[N.Out[0]] = V;
        return true;
    }
    fail(N, "Reshape of " + dimsStr(X0.dims) + " is outside the token-view and attention patterns (DESIGN.md section 13.3)");
}

// ---- the attention pattern's arithmetic: q k^T, the scalar factors, the constant bias, the Softmax, probs x v.
// Nothing is launched here: the state travels in the Val until the closing Reshape (formView).
bool Planner::attentionOp(const Node& N) {
    const std::string& Op = N.Op;
    const bool Binary = Op == "MatMul" || Op == "Mul" || Op == "Div" || Op == "Add";
    if (!Binary && Op != "Softmax") return false;
    const Val& A = get(N, 0);
    const Val* B = Binary ? &get(N, 1) : nullptr;
    const int FA = A.runtime ? A.form : kFormPlain, FB = B && B->runtime ? B->form : kFormPlain;
    if (!isAttForm(FA) && !isAttForm(FB)) return false;
    auto put = [&](Val V, int Form, std::vector<int64_t> Dims) {
        V.form = Form;
        V.dims = std::move(Dims);
        V.producer = N.Name;
        V.chain += "+" + N.Name;
        Vals[N.Out[0]] = V;
        return true;
    };
    if (Op == "Softmax") {
        if (FA != kFormScores) fail(N, "Softmax on " + dimsStr(A.dims) + ": only the softmax over the keys of [N,H,81,81] attention scores is supported");
        int64_t Axis = N.attrI("axis", -1);
        if (Axis < 0) Axis += 4;
        if (Axis != 3) fail(N, "Softmax over axis " + std::to_string(N.attrI("axis", -1)) + " of the attention scores: the keys (axis -1) only");
        interior(N, 0);
        return put(A, kFormProbs, A.dims);
    }
    if (Op == "MatMul") {
        if (FA == kFormHeads && FB == kFormHeadsT) {
            interior(N, 0);
            interior(N, 1);
            if (A.dims[1] != B->dims[1] || A.dims[3] != B->dims[2])
                fail(N, "q " + dimsStr(A.dims) + " and k^T " + dimsStr(B->dims) + " do not agree in heads and head dimension");
            Val V = A;
            V.attQ = A.v;
            V.attK = B->v;
            V.scale = A.scale * B->scale;
            V.chain = A.chain + "+" + B->chain;
            V.bias.clear();
            return put(V, kFormScores, {kBatch, A.dims[1], 81, 81});
        }
        if (FA == kFormProbs && FB == kFormHeads) {
            interior(N, 0);
            interior(N, 1);
            if (B->scale != 1.0) fail(N, "a scalar factor on v is not part of the attention pattern");
            if (A.dims[1] != B->dims[1]) fail(N, "the attention weights have " + std::to_string(A.dims[1]) + " heads, v has " + std::to_string(B->dims[1]));
            const int64_t QD = A.attQ.C / A.dims[1];
            if (QD != B->dims[3]) fail(N, "q and k have head dimension " + std::to_string(QD) + ", v has " + std::to_string(B->dims[3]));
            Val V = A;
            V.attV = B->v;
            V.chain = A.chain + "+" + B->chain;
            return put(V, kFormHeadOut, {kBatch, A.dims[1], 81, B->dims[3]});
        }
        fail(N, "MatMul of " + dimsStr(A.dims) + " and " + dimsStr(B->dims) + " is outside the attention pattern (q k^T, then softmax x v; DESIGN.md section 13.3)");
    }
    // Mul / Div / Add with a constant
    const bool AR = isAttForm(FA);
    const Val& T = AR ? A : *B;
    const Val& Cst = AR ? *B : A;
    if (Cst.runtime) fail(N, "the other operand of " + Op + " on " + dimsStr(T.dims) + " is computed at run time: only constants enter the attention pattern");
    interior(N, AR ? 0 : 1);
    if (Op == "Mul" || Op == "Div") {
        if (Cst.count() != 1) fail(N, "only a scalar constant scales the attention pattern's tensors");
        if (Op == "Div" && !AR) fail(N, "a constant divided by " + dimsStr(T.dims) + " is outside the attention pattern");
        if (T.form != kFormTok4 && T.form != kFormHeads && T.form != kFormHeadsT && T.form != kFormScores)
            fail(N, Op + " on " + dimsStr(T.dims) + " is outside the attention pattern");
        const double S = Op == "Mul" ? Cst.at(0) : 1.0 / Cst.at(0);
        Val V = T;
        V.scale *= S;
        for (double& Bv : V.bias) Bv *= S;
        return put(V, T.form, T.dims);
    }
    // Add: a constant bias on the scores
    if (T.form != kFormScores) fail(N, "Add on " + dimsStr(T.dims) + " is outside the attention pattern (a constant bias is added to the scores)");
    const int64_t H = T.dims[1];
    std::vector<int64_t> CD = Cst.dims;
    if (CD.size() == 4 && CD[0] == 1) CD.erase(CD.begin());
    const bool PerHead = CD == std::vector<int64_t>{H, 81, 81};
    if (!PerHead && CD != std::vector<int64_t>{81, 81} && CD != std::vector<int64_t>{1, 81, 81})
        fail(N, "an attention bias of shape " + dimsStr(Cst.dims) + ": [H,81,81], [1,H,81,81] or [81,81] only");
    Val V = T;
    if (V.bias.empty()) V.bias.assign((size_t)H * 81 * 81, 0.0);
    for (size_t J = 0; J < V.bias.size(); ++J) V.bias[J] += Cst.at(PerHead ? J : J % (81 * 81));
    return put(V, kFormScores, T.dims);
}

// The exact GELU as the exporter writes it, x * (1 + erf(x / sqrt(2))) * 0.5 over five nodes, becomes one Gelu node
// (then an activation like any other: it fuses into a dense epilogue).
void Planner::rewriteGelu() {
    std::map<std::string, int> Cnt;
    std::map<std::string, size_t> Producer;
    for (size_t K = 0; K < Nodes.size(); ++K) {
        if (Skip[K]) continue;
        for (const std::string& I : Nodes[K].In) ++Cnt[I];
        for (const std::string& O : Nodes[K].Out) Producer[O] = K;
    }
    auto scalar = [&](const std::string& T, double* V) {
        auto It = G.Inits.find(T);
        if (It == G.Inits.end() || !It->second.IsFloat || It->second.F.size() != 1) return false;
        *V = It->second.F[0];
        return true;
    };
    // the node producing T when it has op `Op`, one consumer, and T is no graph output
    auto inner = [&](const std::string& T, const char* OpName) -> int {
        auto It = Producer.find(T);
        if (It == Producer.end() || Nodes[It->second].Op != OpName || Cnt[T] != 1 || Outputs.count(T)) return -1;
        return (int)It->second;
    };
    // a two-input node as (runtime operand, scalar constant)
    auto withScalar = [&](const Node& N, std::string* T, double* V) {
        if (N.In.size() != 2) return false;
        for (int Side = 0; Side < 2; ++Side)
            if (scalar(N.In[(size_t)Side], V)) { *T = N.In[(size_t)(1 - Side)]; return true; }
        return false;
    };
    for (size_t K = 0; K < Nodes.size(); ++K) {
        Node& Half = Nodes[K];
        std::string T1, T2, T3, Xs;
        double V = 0;
        if (Skip[K] || Half.Op != "Mul" || !withScalar(Half, &T1, &V) || V != 0.5) continue;
        const int IM = inner(T1, "Mul"); // x * (erf + 1)
        if (IM < 0 || Nodes[(size_t)IM].In.size() != 2) continue;
        for (int Side = 0; Side < 2; ++Side) {
            const std::string& X = Nodes[(size_t)IM].In[(size_t)Side];
            const int IA = inner(Nodes[(size_t)IM].In[(size_t)(1 - Side)], "Add");
            if (IA < 0 || !withScalar(Nodes[(size_t)IA], &T2, &V) || V != 1.0) continue;
            const int IE = inner(T2, "Erf");
            if (IE < 0 || Nodes[(size_t)IE].In.size() != 1) continue;
            const int ID = inner(Nodes[(size_t)IE].In[0], "Div");
            const int IS = inner(Nodes[(size_t)IE].In[0], "Mul");
            const int IX = ID >= 0 ? ID : IS;
            if (IX < 0 || !withScalar(Nodes[(size_t)IX], &T3, &V) || T3 != X) continue;
            if (ID >= 0 && (Nodes[(size_t)ID].In[0] != X || std::fabs(V - std::sqrt(2.0)) > 1e-6)) continue;
            if (ID < 0 && std::fabs(V - std::sqrt(0.5)) > 1e-6) continue;
            Xs = X;
            for (int I : {IM, IA, IE, IX}) {
                Skip[(size_t)I] = true;
                Half.Name = Nodes[(size_t)I].Name + "+" + Half.Name;
            }
            break;
        }
        if (Xs.empty()) continue;
        Half.Op = "Gelu";
        Half.In = {Xs};
        Cnt.clear(); // the counts the next candidate sees
        for (size_t J = 0; J < Nodes.size(); ++J) {
            if (Skip[J]) continue;
            for (const std::string& I : Nodes[J].In) ++Cnt[I];
        }
    }
}

// Mish, tanh-GELU and softsign as the exporter writes them become one node each (MishAct, GeluTanh, Softsign), then an
// activation like any other.  x is the one tensor a pattern reads more than once; every other tensor inside has one
// consumer and is no graph output; commutative nodes match in either operand order; the constants are compared as
// f32 within one ulp.  A chain that starts like a pattern and then deviates is left as it is: plain elementwise nodes.
//   Mish       Mul(x, Tanh(Softplus(x)))
//   tanh-GELU  Mul(Mul(x, Add(Tanh(Mul(Add(x, Mul(x^3, 0.044715)), sqrt(2/pi))), 1)), 0.5), the 0.5 on either Mul;
//              x^3 is Mul(Mul(x, x), x) or Pow(x, 3)
//   softsign   Div(x, Add(Abs(x), 1))
void Planner::rewriteMath() {
    std::map<std::string, int> Cnt;
    std::map<std::string, size_t> Producer;
    for (size_t K = 0; K < Nodes.size(); ++K) {
        if (Skip[K]) continue;
        for (const std::string& I : Nodes[K].In) ++Cnt[I];
        for (const std::string& O : Nodes[K].Out) Producer[O] = K;
    }
    auto near = [](double V, double Want) {
        const float A = (float)V, B = (float)Want;
        return A == B || A == std::nextafterf(B, 0.f) || A == std::nextafterf(B, 2.f * B);
    };
    auto scalar = [&](const std::string& T, double Want) {
        auto It = G.Inits.find(T);
        return It != G.Inits.end() && It->second.IsFloat && It->second.F.size() == 1 && near(It->second.F[0], Want);
    };
    // the node producing the interior tensor T when it has op `OpName`, or -1
    auto inner = [&](const std::string& T, const char* OpName, size_t Arity) -> int {
        auto It = Producer.find(T);
        if (It == Producer.end() || Skip[It->second] || Nodes[It->second].Op != OpName || Nodes[It->second].In.size() != Arity ||
            Cnt[T] != 1 || Outputs.count(T))
            return -1;
        return (int)It->second;
    };
    // the other operand of a two-input node one of whose operands is the scalar `Want`, or of which one operand is T
    auto beside = [&](int I, double Want, std::string* Other) {
        const Node& N = Nodes[(size_t)I];
        for (int Side = 0; Side < 2; ++Side)
            if (scalar(N.In[(size_t)Side], Want)) { *Other = N.In[(size_t)(1 - Side)]; return true; }
        return false;
    };
    auto partner = [&](int I, const std::string& T, std::string* Other) {
        const Node& N = Nodes[(size_t)I];
        for (int Side = 0; Side < 2; ++Side)
            if (N.In[(size_t)Side] == T && N.In[(size_t)(1 - Side)] != T) { *Other = N.In[(size_t)(1 - Side)]; return true; }
        return false;
    };
    auto become = [&](size_t K, const char* OpName, const std::string& X, std::vector<int> Absorbed) {
        Node& N = Nodes[K];
        std::sort(Absorbed.begin(), Absorbed.end());
        std::string Name;
        for (int I : Absorbed) {
            Skip[(size_t)I] = true;
            Name += Nodes[(size_t)I].Name + "+";
        }
        N.Name = Name + N.Name;
        N.Op = OpName;
        N.In = {X};
    };
    // x^3 of X as the tensor T: the nodes that compute it
    auto cube = [&](const std::string& T, const std::string& X, std::vector<int>* Absorbed) {
        const int IP = inner(T, "Pow", 2);
        if (IP >= 0) {
            if (Nodes[(size_t)IP].In[0] != X || !scalar(Nodes[(size_t)IP].In[1], 3.0)) return false;
            Absorbed->push_back(IP);
            return true;
        }
        const int IM = inner(T, "Mul", 2);
        std::string Sq;
        if (IM < 0 || !partner(IM, X, &Sq)) return false;
        const int IS = inner(Sq, "Mul", 2);
        if (IS < 0 || Nodes[(size_t)IS].In[0] != X || Nodes[(size_t)IS].In[1] != X) return false;
        Absorbed->insert(Absorbed->end(), {IM, IS});
        return true;
    };
    // tanh(sqrt(2/pi) (x + 0.044715 x^3)) + 1 as the tensor T
    auto geluTail = [&](const std::string& T, const std::string& X, std::vector<int>* Absorbed) {
        std::string Th, Arg, Sum, Cb, X3;
        const int IA = inner(T, "Add", 2);
        if (IA < 0 || !beside(IA, 1.0, &Th)) return false;
        const int IT = inner(Th, "Tanh", 1);
        if (IT < 0) return false;
        const int IK = inner(Nodes[(size_t)IT].In[0], "Mul", 2);
        if (IK < 0 || !beside(IK, 0.7978845608028654, &Sum)) return false;
        const int IS = inner(Sum, "Add", 2);
        if (IS < 0 || !partner(IS, X, &Cb)) return false;
        const int IC = inner(Cb, "Mul", 2);
        if (IC < 0 || !beside(IC, 0.044715, &X3) || !cube(X3, X, Absorbed)) return false;
        Absorbed->insert(Absorbed->end(), {IA, IT, IK, IS, IC});
        return true;
    };
    for (size_t K = 0; K < Nodes.size(); ++K) {
        const Node& N = Nodes[K];
        if (Skip[K] || N.In.size() != 2) continue;
        if (N.Op == "Div") { // softsign
            std::string Ab;
            const int IA = inner(N.In[1], "Add", 2);
            if (IA < 0 || !beside(IA, 1.0, &Ab)) continue;
            const int IB = inner(Ab, "Abs", 1);
            if (IB < 0 || Nodes[(size_t)IB].In[0] != N.In[0]) continue;
            become(K, "Softsign", std::string(N.In[0]), {IA, IB});
            continue;
        }
        if (N.Op != "Mul") continue;
        bool Done = false;
        for (int Side = 0; Side < 2 && !Done; ++Side) { // Mish: Mul(x, Tanh(Softplus(x)))
            const std::string X = N.In[(size_t)Side];
            const int IT = inner(N.In[(size_t)(1 - Side)], "Tanh", 1);
            if (IT < 0) continue;
            const int IS = inner(Nodes[(size_t)IT].In[0], "Softplus", 1);
            if (IS < 0 || Nodes[(size_t)IS].In[0] != X) continue;
            become(K, "MishAct", X, {IT, IS});
            Done = true;
        }
        if (Done) continue;
        // tanh-GELU: (x * tail) * 0.5, or (x * 0.5) * tail
        std::string Prod, X;
        if (beside((int)K, 0.5, &Prod)) {
            const int IM = inner(Prod, "Mul", 2);
            for (int Side = 0; Side < 2 && IM >= 0 && !Done; ++Side) {
                std::vector<int> Absorbed = {IM};
                X = Nodes[(size_t)IM].In[(size_t)Side];
                if (!geluTail(Nodes[(size_t)IM].In[(size_t)(1 - Side)], X, &Absorbed)) continue;
                become(K, "GeluTanh", X, Absorbed);
                Done = true;
            }
            if (Done) continue;
        }
        for (int Side = 0; Side < 2 && !Done; ++Side) {
            const int IH = inner(N.In[(size_t)Side], "Mul", 2);
            if (IH < 0 || !beside(IH, 0.5, &X)) continue;
            std::vector<int> Absorbed = {IH};
            if (!geluTail(N.In[(size_t)(1 - Side)], X, &Absorbed)) continue;
            become(K, "GeluTanh", X, Absorbed);
            Done = true;
        }
    }
}

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
        L.kind = kLaunchMax;
        L.in = ready(N.In[0]).v;
        L.out = freshView(C, false);
        Val V = runtimeVal(N, {kBatch, C, 1, 1});
        V.v = L.out;
        emit(L);
        Vals[N.Out[0]] = V;
        return;
    }
    for (int64_t S : N.attrInts("strides", {1, 1}))
        if (S != 1) fail(N, "stride " + std::to_string(S) + ": only stride 1 (the output stays 9x9)");
    if (Ks[0] < 1 || Ks[1] < 1 || Ks[0] > 9 || Ks[1] > 9 || Ks[0] % 2 == 0 || Ks[1] % 2 == 0)
        fail(N, "a " + KStr + " kernel: only odd kernel sizes from 1 to 9 each way");
    if (Ceil) fail(N, "ceil_mode 1: only ceil_mode 0");
    if (!Max && Dil != std::vector<int64_t>{1, 1}) fail(N, "a dilated AveragePool: dilations on MaxPool only");
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
    L.kind = kLaunchPool;
    L.kh = KH;
    L.kw = KW;
    L.dh = DH;
    L.dw = DW;
    L.poolMode = Max ? kPoolMax : N.attrI("count_include_pad", 0) != 0 ? kPoolAvgInclude : kPoolAvgExclude;
    L.in = ready(N.In[0]).v; // a view at any channel offset: the kernel reads an unaligned one with scalar loads
    L.out = freshView(C, true);
    Val V = runtimeVal(N, X.dims);
    V.v = L.out;
    emit(L);
    Vals[N.Out[0]] = V;
}

// ---- Split along the channels: every output is a view, like Slice
void Planner::split(const Node& N) {
    const Val& X = get(N, 0);
    if (X.flatOfSpatial) fail(N, "Split of a flattened [N,C*81] view of a spatial tensor");
    const Val Src = ready(N.In[0]);
    const int64_t Rank = (int64_t)Src.dims.size(), ChanAxis = Src.form == kFormToken ? 2 : 1;
    int64_t Axis = N.attrI("axis", 0);
    if (Axis < 0) Axis += Rank;
    if (Axis != ChanAxis || Rank < 2) fail(N, "Split of " + dimsStr(Src.dims) + " along axis " + std::to_string(N.attrI("axis", 0)) + ": along the channels only");
    const int64_t C = Src.v.C;
    std::vector<int64_t> Sizes = has(N, 1) ? ints(N, 1, "the split sizes") : N.attrInts("split", {});
    if (Sizes.empty()) {
        const int64_t Parts = (int64_t)N.Out.size();
        if (C % Parts) fail(N, std::to_string(C) + " channels do not split into " + std::to_string(Parts) + " equal parts");
        Sizes.assign((size_t)Parts, C / Parts);
    }
    int64_t Sum = 0;
    for (int64_t S : Sizes) {
        if (S <= 0) fail(N, "an empty part");
        Sum += S;
    }
    if (Sizes.size() != N.Out.size() || Sum != C)
        fail(N, "the split sizes do not cover the " + std::to_string(C) + " channels with one part per output");
    int64_t Off = 0;
    for (size_t J = 0; J < Sizes.size(); Off += Sizes[J], ++J) {
        if (N.Out[J].empty()) continue;
        Val V = Src;
        V.producer = N.Name;
        V.v.offset += (int)Off;
        V.v.C = (int)Sizes[J];
        V.dims[(size_t)ChanAxis] = Sizes[J];
        Vals[N.Out[J]] = V;
    }
}

// ---- the plan ----------------------------------------------------------------------------------------------------
void Planner::run() {
    // tensor contract (trt.cc:144-227)
    std::set<std::string> Ins;
    for (const std::string& I : G.Inputs)
        if (!G.Inits.count(I)) Ins.insert(I);
    std::string OutList;
    for (const std::string& O : G.Outputs) OutList += (OutList.empty() ? "" : ", ") + O;
    Outputs.insert(G.Outputs.begin(), G.Outputs.end());
    if (!Ins.count("input")) throw Error("tensor contract: the graph has no input named 'input'");
    for (const char* O : {"policy", "value", "draw"})
        if (!Outputs.count(O))
            throw Error(std::string("tensor contract: graph output '") + O + "' is missing (the graph's outputs: " + OutList + ")");
    for (const std::string& I : Ins)
        if (I != "input") throw Error("tensor contract: unexpected graph input '" + I + "'");

    // (checked on the file's own nodes, before the rewrites below name theirs)
    for (const Node& N : G.Nodes)
        if (!opSet().count(N.Op) && N.Op != "Swish" && N.Op != "Gelu") fail(N, "op '" + N.Op + "' is outside the supported op set (DESIGN.md section 13)");

    // the swish rewrite: Mul(x, Sigmoid(x)) -> Swish(x) when the Sigmoid feeds only the Mul
    Nodes = G.Nodes;
    P.nodes = (int)Nodes.size();
    Skip.assign(Nodes.size(), false);
    {
        std::map<std::string, int> Cnt;
        std::map<std::string, size_t> Producer;
        for (size_t K = 0; K < Nodes.size(); ++K) {
            for (const std::string& I : Nodes[K].In) ++Cnt[I];
            for (const std::string& O : Nodes[K].Out) Producer[O] = K;
        }
        for (Node& N : Nodes) {
            if (N.Op != "Mul" || N.In.size() != 2) continue;
            for (int Side = 0; Side < 2; ++Side) {
                const std::string& S = N.In[(size_t)Side];
                const std::string& X = N.In[(size_t)(1 - Side)];
                auto It = Producer.find(S);
                if (It == Producer.end()) continue;
                const Node& Sg = Nodes[It->second];
                if (Sg.Op != "Sigmoid" || Sg.In.size() != 1 || Sg.In[0] != X || Cnt[S] != 1 || Outputs.count(S)) continue;
                Skip[It->second] = true;
                N.Op = "Swish";
                N.In = {X};
                break;
            }
        }
    }
    rewriteGelu();
    rewriteMath();
    for (size_t K = 0; K < Nodes.size(); ++K) {
        if (Skip[K]) continue;
        const Node& N = Nodes[K];
        for (const std::string& I : N.In)
            if (!I.empty()) {
                ++Uses[I];
                if (N.Op == "Shape") ++ShapeUses[I];
            }
    }
    for (const std::string& O : G.Outputs) ++Uses[O];
    for (size_t K = 0; K < Nodes.size(); ++K)
        if (!Skip[K])
            for (const std::string& O : Nodes[K].Out) ProducerOf[O] = K;

    // constants
    for (const auto& KV : G.Inits) {
        Val V;
        V.dims = KV.second.Dims;
        V.isInt = !KV.second.IsFloat;
        if (V.isInt) V.i = KV.second.I;
        else {
            V.f.assign(KV.second.F.begin(), KV.second.F.end());
            P.params += KV.second.F.size();
        }
        Vals[KV.first] = V;
    }
    {   // the graph input: [N, numChannels, 9, 9] as the plane expansion writes it
        for (size_t K = 0; K < G.Inputs.size(); ++K) {
            if (G.Inputs[K] != "input") continue;
            std::vector<int64_t> Decl;
            if (K < G.InputInfos.size() && valueInfoDims(G.InputInfos[K], &Decl)) {
                std::string First;
                for (const Node& N : Nodes)
                    for (const std::string& I : N.In)
                        if (I == "input" && First.empty()) First = N.Name;
                if (Decl.size() != 4 || (Decl[2] != 9 && Decl[2] != -1) || (Decl[3] != 9 && Decl[3] != -1))
                    throw Error("graph input 'input' (read by node '" + First + "') is declared " + dimsStr(Decl) + ", not [N,C,9,9]");
                if (Decl[1] > 0 && Decl[1] != NumChannels)
                    throw Error("graph input 'input' (read by node '" + First + "') has " + std::to_string(Decl[1]) +
                                " planes, the evaluator has " + std::to_string(NumChannels));
            }
        }
        Val In;
        In.runtime = true;
        In.dims = {kBatch, NumChannels, 9, 9};
        In.v.buf = -1;
        In.v.C = NumChannels;
        In.v.stride = roundUp(NumChannels, kChunk);
        In.v.spatial = true;
        In.producer = "input";
        Vals["input"] = In;
        P.planeStride = In.v.stride;
    }

    for (size_t K = 0; K < Nodes.size(); ++K) {
        if (Skip[K]) continue;
        const Node& N = Nodes[K];
        const std::string& Op = N.Op;
        if (N.Out.empty()) fail(N, "no output");
        if (Op == "Constant") {
            if (!Vals.count(N.Out[0])) fail(N, "unsupported Constant attribute (value tensor or value_float only)");
            continue;
        }
        bool AnyRuntime = false;
        for (const std::string& I : N.In)
            if (!I.empty()) {
                auto It = Vals.find(I);
                if (It == Vals.end()) fail(N, "input '" + I + "' is not defined before its use");
                AnyRuntime = AnyRuntime || It->second.runtime;
            }
        if (Op == "Shape" || !AnyRuntime) {
            hostFold(N);
            continue;
        }
        const Val& X = get(N, 0);
        double PowOne = 0;
        if (formView(N) || attentionOp(N) || normOp(N, K)) continue;
        // [N,C,81] and the 4-D tensors exist only inside the patterns the calls above follow
        for (size_t J = 0; J < N.In.size(); ++J) {
            if (N.In[J].empty()) continue;
            const Val& I = Vals.at(N.In[J]);
            if (I.runtime && (I.form == kFormGroup3 || I.normG > 0))
                fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " exists only inside the GroupNorm pattern: Reshape, InstanceNormalization, Reshape back to [N,C,9,9] (DESIGN.md section 13.3)");
            if (I.runtime && I.form == kFormChanLast)
                fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " is a channel-last view: only a LayerNorm over its last axis and Transpose [0,3,1,2] read it (DESIGN.md section 13.3)");
            if (I.runtime && I.form >= kFormChan3)
                fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " is consumed outside the token-view and attention patterns (DESIGN.md section 13.3)");
        }
        if (Op == "Softmax") {
            fail(N, "Softmax on " + dimsStr(X.dims) + ": only the softmax over the keys of the attention pattern, on [N,H,81,81] scores, is supported");
        } else if (Op == "Transpose") {
            fail(N, "Transpose of " + dimsStr(X.dims) + " with perm " + dimsStr(N.attrInts("perm", {})) + " is outside the token-view and attention patterns");
        } else if (Op == "LayerNormalization") {
            layerNorm(N);
        } else if (Op == "Conv" || Op == "Gemm" || Op == "MatMul") {
            linear(N, K);
        } else if (Op == "Pow" && powExponent(N, &PowOne) && PowOne == 1.0 && X.runtime) {
            // x ** 1 is x: an open elementwise group read only here stays open under the new name
            const bool MoveGroup = X.group >= 0 && absorbable(N.In[0]);
            Val V = MoveGroup ? X : ready(N.In[0]);
            V.producer = N.Name;
            if (MoveGroup) Groups[(size_t)V.group].out = N.Out[0];
            Vals[N.Out[0]] = V;
        } else if (isAct(Op) || isBinary(Op) || isEltExtra(Op) || Op == "BatchNormalization" || Op == "Pow") {
            if (Op == "BatchNormalization" && !X.runtime) fail(N, "expected a runtime input");
            if (isBinary(Op) && !get(N, 0).runtime && !get(N, 1).runtime) fail(N, "constant operands only");
            elementwise(N);
        } else if (Op == "MaxPool" || Op == "AveragePool") {
            pool(N);
        } else if (Op == "Split") {
            split(N);
        } else if (Op == "GlobalAveragePool" || Op == "ReduceMean" || Op == "GlobalMaxPool" || Op == "ReduceMax") {
            const bool Reduce = Op == "ReduceMean" || Op == "ReduceMax";
            const bool Tok = X.form == kFormToken && Reduce;
            if (!Tok && (X.flatOfSpatial || !isSpatialDims(X.dims))) fail(N, "input " + dimsStr(X.dims) + " is not [N,C,9,9]");
            bool Keep = true;
            if (Reduce) {
                std::vector<int64_t> Axes = has(N, 1) ? ints(N, 1, "axes") : N.attrInts("axes", {});
                for (int64_t& A : Axes) if (A < 0) A += Tok ? 3 : 4;
                std::sort(Axes.begin(), Axes.end());
                if (Tok ? Axes != std::vector<int64_t>{1} : Axes != std::vector<int64_t>{2, 3})
                    fail(N, Op + " over the squares only: axes {2,3} of [N,C,9,9], axis 1 of a token tensor");
                Keep = N.attrI("keepdims", 1) != 0;
                if (Tok && Keep) fail(N, Op + " of a token tensor with keepdims = 0 only");
            }
            const int C = Tok ? (int)X.dims[2] : (int)X.dims[1];
            Launch L;
            L.kind = Op == "GlobalMaxPool" || Op == "ReduceMax" ? kLaunchMax : kLaunchMean;
            L.name = N.Name;
            L.in = ready(N.In[0]).v;
            L.out = freshView(C, false);
            Val V = runtimeVal(N, Keep ? std::vector<int64_t>{kBatch, C, 1, 1} : std::vector<int64_t>{kBatch, C});
            V.v = L.out;
            emit(L);
            Vals[N.Out[0]] = V;
        } else if (X.form == kFormToken && Op != "Slice" && Op != "Identity") { // (Split on tokens is taken above)
            fail(N, "op '" + Op + "' is not supported on a token tensor " + dimsStr(X.dims));
        } else if (Op == "Flatten" || Op == "Reshape" || Op == "Squeeze" || Op == "Unsqueeze" || Op == "Identity") {
            // an open elementwise group read only here stays open: the reshaped tensor is its new result
            // (a [N,C,9,9] group that becomes [N,C*81] is emitted first: the flattened view reads its buffer)
            bool MoveGroup = Vals.at(N.In[0]).group >= 0 && absorbable(N.In[0]);
            Val Src = MoveGroup ? Vals.at(N.In[0]) : ready(N.In[0]);
            const std::vector<int64_t> SD = Src.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)Src.v.C * 81} : Src.dims;
            int64_t Rest = 1;
            for (size_t J = 1; J < SD.size(); ++J) Rest *= SD[J];
            std::vector<int64_t> ND;
            if (Op == "Identity") ND = SD;
            else if (Op == "Flatten") {
                if (N.attrI("axis", 1) != 1) fail(N, "Flatten with axis 1 only");
                ND = {kBatch, Rest};
            } else if (Op == "Reshape") {
                const std::vector<int64_t> Sh = ints(N, 1, "the target shape");
                int64_t Known = 1;
                int Infer = -1;
                ND.assign(Sh.size(), 0);
                for (size_t J = 0; J < Sh.size(); ++J) {
                    int64_t V = Sh[J];
                    if (V == 0 && J < SD.size()) V = SD[J];
                    if (V == -1) { Infer = (int)J; continue; }
                    ND[J] = V;
                    if (V != kBatch) Known *= V;
                }
                bool HasBatch = std::count(ND.begin(), ND.end(), kBatch) == 1;
                if (Infer >= 0) {
                    if (HasBatch) {
                        if (Known <= 0 || Rest % Known) fail(N, "cannot infer the -1 dimension");
                        ND[(size_t)Infer] = Rest / Known;
                    } else {
                        if (Known != Rest) fail(N, "reshape would mix boards");
                        ND[(size_t)Infer] = kBatch;
                    }
                }
                if (ND.empty() || ND[0] != kBatch) fail(N, "the target shape " + dimsStr(ND) + " does not keep the batch first");
            } else {
                std::vector<int64_t> Axes = has(N, 1) ? ints(N, 1, "axes") : N.attrInts("axes", {});
                ND = SD;
                if (Op == "Unsqueeze") {
                    const int64_t Rank = (int64_t)(SD.size() + Axes.size());
                    for (int64_t& A : Axes) if (A < 0) A += Rank;
                    std::sort(Axes.begin(), Axes.end());
                    for (int64_t A : Axes) {
                        if (A <= 0 || A > (int64_t)ND.size()) fail(N, "cannot unsqueeze the batch axis");
                        ND.insert(ND.begin() + A, 1);
                    }
                } else {
                    std::vector<int64_t> Keep;
                    for (size_t J = 0; J < SD.size(); ++J) {
                        bool Drop = Axes.empty() ? (J > 0 && SD[J] == 1) : false;
                        for (int64_t A : Axes) Drop = Drop || (A < 0 ? A + (int64_t)SD.size() : A) == (int64_t)J;
                        if (Drop && (J == 0 || SD[J] != 1)) fail(N, "squeezes a dimension that is not 1");
                        if (!Drop) Keep.push_back(SD[J]);
                    }
                    ND = Keep;
                }
            }
            int64_t NR = 1;
            for (size_t J = 1; J < ND.size(); ++J) NR *= ND[J];
            if (NR != Rest) fail(N, "element count changes: " + dimsStr(SD) + " -> " + dimsStr(ND));
            const bool SrcSpatial = Src.flatOfSpatial || isSpatialDims(Src.dims);
            const int64_t SrcC = Src.flatOfSpatial ? (int64_t)Src.v.C : SrcSpatial ? Src.dims[1] : -1;
            if (MoveGroup && SrcSpatial && !isSpatialDims(ND)) {
                MoveGroup = false;
                Src = ready(N.In[0]);
            }
            Val V = Src;
            V.producer = N.Name;
            V.dims = ND;
            if (SrcSpatial) {
                if (isSpatialDims(ND) && ND[1] == SrcC) V.flatOfSpatial = false;
                else if (ND.size() == 2) V.flatOfSpatial = true;
                else fail(N, "a [N,C,9,9] tensor can become [N,C*81] or stay [N,C,9,9], not " + dimsStr(ND));
            } else if (flatC(ND) < 0) {
                fail(N, "a flat tensor cannot become " + dimsStr(ND));
            }
            if (!V.flatOfSpatial && !isSpatialDims(V.dims)) V.dims = ND;
            if (MoveGroup) Groups[(size_t)V.group].out = N.Out[0];
            Vals[N.Out[0]] = V;
        } else if (Op == "Concat") {
            int64_t Ax = N.attrI("axis", 1);
            const size_t Rank = X.flatOfSpatial ? 2 : X.dims.size();
            if (Ax < 0) Ax += (int64_t)Rank;
            if (Ax != 1) fail(N, "Concat of runtime tensors along axis 1 only");
            if (N.In.size() > (size_t)kMaxCopySegs) fail(N, "more than " + std::to_string(kMaxCopySegs) + " inputs");
            Launch L;
            L.kind = kLaunchConcat;
            L.name = N.Name;
            int Total = 0;
            bool Sp = false;
            std::vector<int64_t> D0;
            for (size_t J = 0; J < N.In.size(); ++J) {
                const Val& V = get(N, J);
                if (!V.runtime) fail(N, "Concat of a runtime tensor and a constant");
                if (V.form != kFormPlain) fail(N, "Concat of a token tensor " + dimsStr(V.dims));
                const bool VS = !V.flatOfSpatial && isSpatialDims(V.dims);
                if (J == 0) Sp = VS;
                if (VS != Sp) fail(N, "Concat of [N,C,9,9] and flat tensors");
                if (!Sp && (V.flatOfSpatial ? 2 : V.dims.size()) != Rank) fail(N, "Concat of different ranks");
                CopySeg S;
                S.v = V.flatOfSpatial ? plain(N.In[J], N.Name + " (flatten)") : ready(N.In[J]).v;
                S.dstOff = Total;
                Total += S.v.C;
                L.segs.push_back(S);
            }
            L.out = freshView(Total, Sp);
            std::vector<int64_t> ND = Sp ? std::vector<int64_t>{kBatch, Total, 9, 9} : std::vector<int64_t>{kBatch, Total};
            if (!Sp) for (size_t J = 2; J < Rank; ++J) ND.push_back(1);
            Val V = runtimeVal(N, ND);
            V.v = L.out;
            emit(L);
            Vals[N.Out[0]] = V;
        } else if (Op == "Slice") {
            const Val Src = X.flatOfSpatial ? (plain(N.In[0], N.Name + " (flatten)"), Vals.at(N.In[0])) : ready(N.In[0]);
            const std::vector<int64_t> St = ints(N, 1, "starts"), En = ints(N, 2, "ends");
            std::vector<int64_t> Axes = has(N, 3) ? ints(N, 3, "axes") : std::vector<int64_t>();
            const std::vector<int64_t> Sp = has(N, 4) ? ints(N, 4, "steps") : std::vector<int64_t>(St.size(), 1);
            if (Axes.empty()) for (size_t J = 0; J < St.size(); ++J) Axes.push_back((int64_t)J);
            if (St.size() != En.size() || Axes.size() != St.size() || Sp.size() != St.size()) fail(N, "malformed Slice");
            Val V = Src;
            V.producer = N.Name;
            const int64_t ChanAxis = Src.form == kFormToken ? 2 : 1;
            for (size_t J = 0; J < Axes.size(); ++J) {
                int64_t A = Axes[J] < 0 ? Axes[J] + (int64_t)Src.dims.size() : Axes[J];
                if (Sp[J] != 1) fail(N, "Slice with a step other than 1");
                if (A == ChanAxis) {
                    const int64_t Len = Src.v.C;
                    int64_t S = St[J] < 0 ? St[J] + Len : St[J], E = En[J] < 0 ? En[J] + Len : En[J];
                    S = std::max<int64_t>(0, std::min(S, Len));
                    E = std::max<int64_t>(S, std::min(E, Len));
                    if (E == S) fail(N, "empty slice");
                    V.v.offset += (int)S;
                    V.v.C = (int)(E - S);
                    V.dims[(size_t)ChanAxis] = E - S;
                } else {
                    const int64_t Dim = A < (int64_t)Src.dims.size() ? Src.dims[(size_t)A] : 1;
                    if (St[J] != 0 || (Dim != kBatch && En[J] < Dim)) fail(N, "Slice along an axis other than the channels");
                }
            }
            Vals[N.Out[0]] = V;
        } else if (Op == "Gather" || Op == "Cast") {
            fail(N, "applied to a runtime tensor (folded on shape values only)");
        } else {
            fail(N, "op '" + Op + "' is not supported on runtime tensors");
        }
    }
    checkOutputs();
    assignBuffers();
}

void Planner::checkOutputs() {
    auto producerNode = [&](const std::string& T) -> const Node* {
        for (const Node& N : Nodes)
            for (const std::string& O : N.Out)
                if (O == T) return &N;
        return nullptr;
    };
    auto outFail = [&](const std::string& T, const std::string& Why) {
        const Node* N = producerNode(T);
        if (N) fail(*N, "output '" + T + "' " + Why);
        throw Error("output '" + T + "' " + Why);
    };
    for (const char* O : {"policy", "value", "draw"}) {
        auto It = Vals.find(O);
        if (It == Vals.end()) outFail(O, "is never computed");
        if (!It->second.runtime) outFail(O, "is a constant");
        ready(O);
    }
    {
        const Val& V = Vals.at("policy");
        if (V.flatOfSpatial || isSpatialDims(V.dims)) {
            if (V.v.C * 81 != 2187) outFail("policy", "has " + std::to_string(V.v.C * 81) + " values per position (expected: 2187)");
            P.policy = V.v;
        } else {
            const int C = flatC(V.dims);
            if (C != 2187) outFail("policy", "has " + std::to_string(C) + " values per position (expected: 2187)");
            P.policy = V.v;
        }
    }
    for (const char* O : {"value", "draw"}) {
        const Val& V = Vals.at(O);
        if (V.flatOfSpatial || isSpatialDims(V.dims) || flatC(V.dims) != 1)
            outFail(O, "must hold one value per position, it is " + dimsStr(V.dims));
        (O[0] == 'v' ? P.value : P.draw) = V.v;
    }
}

// lifetimes -> physical buffers (a launch's output never shares a buffer with its inputs)
void Planner::assignBuffers() {
    const size_t NV = VirtStride.size();
    std::vector<int> Last(NV, -1);
    auto use = [&](const View& V, int I) {
        if (V.buf >= 0) Last[(size_t)V.buf] = std::max(Last[(size_t)V.buf], I);
    };
    const int NL = (int)P.launches.size();
    for (int I = 0; I < NL; ++I) {
        const Launch& L = P.launches[(size_t)I];
        use(L.in, I);
        use(L.res, I);
        use(L.attK, I);
        use(L.attV, I);
        for (const EltSrc& S : L.srcs) if (S.mode == kSrcSame || S.mode == kSrcBoard) use(S.v, I);
        for (const CopySeg& S : L.segs) use(S.v, I);
        use(L.out, I);
    }
    use(P.policy, NL);
    use(P.value, NL);
    use(P.draw, NL);
    std::vector<int> Phys(NV, -1);
    std::vector<bool> Free;
    auto take = [&](int V) {
        int Best = -1;
        for (size_t K = 0; K < Free.size(); ++K)
            if (Free[K]) {
                const int S = VirtSpatial[(size_t)V] ? P.bufSpatialStride[K] : P.bufFlatStride[K];
                if (Best < 0 || S >= VirtStride[(size_t)V]) { Best = (int)K; if (S >= VirtStride[(size_t)V]) break; }
            }
        if (Best < 0) {
            Best = (int)Free.size();
            Free.push_back(false);
            P.bufSpatialStride.push_back(0);
            P.bufFlatStride.push_back(0);
        }
        Free[(size_t)Best] = false;
        int& S = VirtSpatial[(size_t)V] ? P.bufSpatialStride[(size_t)Best] : P.bufFlatStride[(size_t)Best];
        S = std::max(S, VirtStride[(size_t)V]);
        Phys[(size_t)V] = Best;
    };
    for (int I = 0; I < NL; ++I) {
        const Launch& L = P.launches[(size_t)I];
        take(L.out.buf);
        for (size_t V = 0; V < NV; ++V)
            if (Last[V] == I && Phys[V] >= 0) Free[(size_t)Phys[V]] = true;
    }
    auto map = [&](View& V) {
        if (V.buf == kPending) throw Error("internal planner error: a launch reads an elementwise result before it is computed");
        if (V.buf >= 0) V.buf = Phys[(size_t)V.buf];
    };
    for (Launch& L : P.launches) {
        map(L.in);
        map(L.res);
        map(L.attK);
        map(L.attV);
        map(L.out);
        for (EltSrc& S : L.srcs) if (S.mode == kSrcSame || S.mode == kSrcBoard) map(S.v);
        for (CopySeg& S : L.segs) map(S.v);
    }
    map(P.policy);
    map(P.value);
    map(P.draw);
    size_t Bytes = (size_t)P.planeStride * 81 * 4;
    for (size_t K = 0; K < P.bufSpatialStride.size(); ++K)
        Bytes += 4 * std::max((size_t)P.bufSpatialStride[K] * 81, (size_t)P.bufFlatStride[K]);
    P.activationBytesPerPosition = Bytes;
}

} // namespace

bool buildPlan(const void* Data, size_t Size, int NumChannels, GraphPlan* Plan, std::string* Err) {
    try {
        const Graph G = readModel(Span{(const unsigned char*)Data, Size});
        GraphPlan P;
        P.numChannels = NumChannels;
        Planner(G, NumChannels, &P).run();
        *Plan = std::move(P);
        return true;
    } catch (const std::exception& E) {
        if (Err) *Err = E.what();
        return false;
    }
}

int countNodes(const void* Data, size_t Size) {
    try {
        return (int)readModel(Span{(const unsigned char*)Data, Size}).Nodes.size();
    } catch (const std::exception&) {
        return 0;
    }
}

} // namespace graph
} // namespace nsg
