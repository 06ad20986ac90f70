// planner_host.cc -- the planner on constants: op classes, constant scalars, host folding.
#include "planner.h"

namespace nsg::graph {

// (Swish, Gelu, MishAct, GeluTanh and Softsign are the planner's own nodes, written by its rewrites)
static int actOf(const std::string& Op) {
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
bool isAct(const std::string& Op) { return actOf(Op) != kActNone; }
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
        "ReduceMin", "ReduceSum", "Expand", "ReduceL1", "ReduceL2", "ReduceSumSquare", "ReduceLogSumExp",
        // Shape and Cast are folded on the host only (shape chains); a Gather of a runtime tensor is planner_gather.cc's
        "Shape", "Gather", "Cast",
        // Mod is folded on host constants only (the shape checks of torch's unflatten); on a run-time tensor it is refused
        // in the words of an op outside the set (lower, onnx_graph.cc)
        "Mod"};
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

// The `axes` of a Squeeze, Unsqueeze or reduction: input 1 from opset 13 on, the attribute before; a negative axis counts
// from Rank, or from the rank of the result when the axes are `Added` to it (Unsqueeze).  In the model's order.
std::vector<int64_t> Planner::axes(const Node& N, size_t Rank, bool Added) {
    std::vector<int64_t> Axes = has(N, 1) ? ints(N, 1, "axes") : N.attrInts("axes", {});
    for (int64_t& A : Axes)
        if (A < 0) A += (int64_t)(Rank + (Added ? Axes.size() : 0));
    return Axes;
}

// An inference BatchNormalization's channel, in double: inputs 1 to 4 are constants (gamma, beta, mean, variance)
Planner::BnChannel Planner::bnChannel(const Node& Bn, size_t Ch) const {
    const double Gm = Vals.at(Bn.In[1]).at(Ch), Vr = Vals.at(Bn.In[4]).at(Ch);
    return {Gm / std::sqrt(Vr + Bn.attrF("epsilon", 1e-5)), Vals.at(Bn.In[3]).at(Ch), Vals.at(Bn.In[2]).at(Ch)};
}

// ---- host folding (constants and shape chains) ---------------------------------------------------------------
void Planner::hostFold(const Node& N) {
    const std::string& Op = N.Op;
    Val R;
    auto Out = [&]() -> Val& { return Vals[N.Out[0]]; };
    if (Op == "Shape") {
        const Val& X = get(N, 0);
        std::vector<int64_t> D = X.shownDims();
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
                if (X.isInt && batchFactor(X.i[K])) fail(N, "cannot cast the batch dimension to a float");
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
        R = X;
        std::vector<int64_t> D = X.dims;
        std::vector<int64_t> Axes = axes(N, D.size(), Op == "Unsqueeze");
        if (Op == "Unsqueeze") {
            std::sort(Axes.begin(), Axes.end());
            for (int64_t A : Axes) {
                if (A < 0 || A > (int64_t)D.size()) fail(N, "axis out of range");
                D.insert(D.begin() + A, 1);
            }
        } else {
            std::vector<int64_t> ND;
            for (size_t K = 0; K < D.size(); ++K) {
                bool Drop = Axes.empty() ? D[K] == 1 : false;
                for (int64_t A : Axes) Drop = Drop || A == (int64_t)K;
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
    Out() = foldArithmetic(N, X);
}

// Add / Sub / Mul / Div and the unary maths on constants; the symbolic batch dimension survives only what leaves it as it is
Val Planner::foldArithmetic(const Node& N, const Val& X) {
    const std::string& Op = N.Op;
    Val R;
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
                const int64_t F1 = batchFactor(P1), F2 = batchFactor(P2);
                const bool Sym = F1 || F2;
                if (Sym && Op == "Mul" && !(F1 && F2) && (F1 ? P2 : P1) >= 1 && (F1 + F2) * (F1 ? P2 : P1) < kMaxBatchFactor) {
                    V = batchTimes((F1 + F2) * (F1 ? P2 : P1)); // the batch times a constant: N*H, N*81 (planner.h)
                } else if (Sym && (F1 > 1 || F2 > 1)) {
                    fail(N, "arithmetic on a multiple of the symbolic batch dimension (" + dimsStr({P1}) + " " + Op + " " + dimsStr({P2}) +
                                "): only a product with a positive constant is followed");
                } else if (Sym) {
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
                if ((X.isInt && batchFactor(X.i[A])) || (Y.isInt && batchFactor(Y.i[B]))) fail(N, "arithmetic on the symbolic batch dimension");
                const double P1 = X.at(A), P2 = Y.at(B);
                R.f.push_back(Op == "Add" ? P1 + P2 : Op == "Sub" ? P1 - P2 : Op == "Mul" ? P1 * P2 : P1 / P2);
            }
        }
        return R;
    }
    if (Op == "Mod") { // integers only, fmod = 0: the sign follows the divisor (torch's `dim % rank` in unflatten)
        const Val& Y = host(N, 1, "the divisor");
        if (!X.isInt || !Y.isInt || N.attrI("fmod", 0) != 0) fail(N, "Mod is folded on integer constants with fmod = 0 only");
        if (Y.count() != 1 && Y.count() != X.count()) fail(N, "constant folding supports equal shapes or a scalar divisor");
        R.isInt = true;
        R.dims = X.dims;
        for (size_t K = 0; K < X.count(); ++K) {
            const int64_t A = X.i[K], B = Y.i[Y.count() == 1 ? 0 : K];
            if (batchFactor(A) || batchFactor(B)) fail(N, "arithmetic on the symbolic batch dimension");
            if (B == 0) fail(N, "integer division by zero");
            const int64_t M = A % B;
            R.i.push_back(M != 0 && (M < 0) != (B < 0) ? M + B : M);
        }
        return R;
    }
    if (Op == "Sqrt" || Op == "Pow" || Op == "Exp" || Op == "Log" || Op == "Reciprocal") { // torch emits them for `d ** -0.5` when d comes from size()
        const Val* Y = Op == "Pow" ? &host(N, 1, "the exponent") : nullptr;
        if (Y && Y->count() != 1 && Y->count() != X.count()) fail(N, "constant folding supports equal shapes or a scalar exponent");
        R.dims = X.dims;
        for (size_t K = 0; K < X.count(); ++K) {
            if (X.isInt && batchFactor(X.i[K])) fail(N, "arithmetic on the symbolic batch dimension");
            const double A = X.at(K);
            R.f.push_back(Y ? std::pow(A, Y->at(Y->count() == 1 ? 0 : K)) : Op == "Sqrt" ? std::sqrt(A) : Op == "Exp" ? std::exp(A) : Op == "Log" ? std::log(A) : 1.0 / A);
        }
        return R;
    }
    fail(N, "is applied to constants only; folding it is not supported");
}

} // namespace nsg::graph
