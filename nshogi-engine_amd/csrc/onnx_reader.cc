// onnx_reader.cc -- see onnx_reader.h.
#include "onnx_reader.h"
#include "onnx_proto.h"

#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>

namespace nsg {
namespace onnx {

namespace {

using namespace wire;

// ---- topology matching ----------------------------------------------------------------------
[[noreturn]] void fail(const Node& N, const std::string& Why) {
    throw Error("unsupported ONNX structure at node '" + N.Name + "' (" + N.Op + "): " + Why);
}

struct ConvBn {
    std::vector<float> W;     // [n][cin][k][k]
    std::vector<float> Stats; // [4][n]: gamma, beta, mean, var
    int N = 0, Cin = 0;
    bool NoBn = false; // identity statistics: var is set to 1 - eps once the model's epsilon is known
    std::string Out;
};

class Matcher {
 public:
    explicit Matcher(const Graph& Gr) : G(Gr) {}

    const Node& only(const std::string& T, const char* What) const {
        auto It = G.Consumers.find(T);
        const size_t C = It == G.Consumers.end() ? 0 : It->second.size();
        if (C != 1) throw Error(std::string(What) + ": tensor '" + T + "' has " + std::to_string(C) + " consumers, expected 1");
        return *It->second[0];
    }
    std::vector<const Node*> consumers(const std::string& T) const {
        auto It = G.Consumers.find(T);
        return It == G.Consumers.end() ? std::vector<const Node*>() : It->second;
    }
    const Tensor* init(const std::string& Name) const {
        auto It = G.Inits.find(Name);
        return It == G.Inits.end() ? nullptr : &It->second;
    }
    const Tensor& needFloat(const Node& N, size_t Idx, const char* What) const {
        const Tensor* T = Idx < N.In.size() ? init(N.In[Idx]) : nullptr;
        if (!T || !T->IsFloat) fail(N, std::string("expected a constant float32 ") + What);
        return *T;
    }

    ConvBn convBn(const std::string& X, const Node& Nd, int K) {
        if (Nd.Op != "Conv" || Nd.In.empty() || Nd.In[0] != X) fail(Nd, "expected a Conv of '" + X + "'");
        const Tensor& Wt = needFloat(Nd, 1, "weight");
        if (Wt.Dims.size() != 4 || Wt.Dims[2] != K || Wt.Dims[3] != K)
            fail(Nd, "expected a constant " + std::to_string(K) + "x" + std::to_string(K) + " weight");
        const int64_t Pad = K / 2;
        bool Ok = Nd.attrI("group", 1) == 1;
        for (int64_t S : Nd.attrInts("strides", {1, 1})) Ok = Ok && S == 1;
        for (int64_t D : Nd.attrInts("dilations", {1, 1})) Ok = Ok && D == 1;
        const std::vector<int64_t> Pads = Nd.attrInts("pads", {Pad, Pad, Pad, Pad});
        Ok = Ok && Pads.size() == 4;
        for (int64_t P : Pads) Ok = Ok && P == Pad;
        if (!Ok) fail(Nd, "only stride 1, dilation 1, group 1, 'same' padding");
        ConvBn R;
        R.N = (int)Wt.Dims[0];
        R.Cin = (int)Wt.Dims[1];
        R.W = Wt.F;
        std::vector<float> Bias((size_t)R.N, 0.f);
        if (Nd.In.size() > 2 && !Nd.In[2].empty()) {
            const Tensor& B = needFloat(Nd, 2, "bias");
            if ((int)B.count() != R.N) fail(Nd, "bias length does not match the output channels");
            Bias = B.F;
        }
        R.Stats.resize((size_t)4 * R.N);
        const std::string& Y = Nd.Out[0];
        const auto Next = consumers(Y);
        if (Next.size() == 1 && Next[0]->Op == "BatchNormalization") {
            const Node& B = *Next[0];
            if (B.In.size() < 5) fail(B, "expected scale, bias, mean and variance inputs");
            for (int S = 0; S < 4; ++S) {
                const Tensor& T = needFloat(B, (size_t)S + 1, "BatchNormalization statistic");
                if ((int)T.count() != R.N) fail(B, "statistic length does not match the channels");
                for (int I = 0; I < R.N; ++I) R.Stats[(size_t)S * R.N + I] = T.F[I];
            }
            for (int I = 0; I < R.N; ++I) R.Stats[(size_t)2 * R.N + I] -= Bias[I]; // a conv bias folds into the BN mean
            EpsSeen.push_back(B.attrF("epsilon", kEpsDefault));
            R.Out = B.Out[0];
            return R;
        }
        // no BN: identity statistics carrying the conv bias (var + eps == 1: folded scale 1; the
        // variance is rewritten by finishIdentity() with the epsilon the NSGW header will hold)
        R.NoBn = true;
        for (int I = 0; I < R.N; ++I) {
            R.Stats[I] = 1.f;
            R.Stats[(size_t)R.N + I] = Bias[I];
            R.Stats[(size_t)2 * R.N + I] = 0.f;
            R.Stats[(size_t)3 * R.N + I] = (float)(1.0 - kEpsDefault);
        }
        R.Out = Y;
        return R;
    }

    std::string relu(const std::string& T) const {
        const Node& Nd = only(T, "activation");
        if (Nd.Op != "Relu") fail(Nd, "expected Relu");
        return Nd.Out[0];
    }

    bool reaches(const std::string& From, const std::string& Goal) const {
        std::set<std::string> Seen;
        std::vector<std::string> Todo{From};
        while (!Todo.empty()) {
            const std::string U = Todo.back();
            Todo.pop_back();
            if (U == Goal) return true;
            for (const Node* C : consumers(U))
                for (const std::string& O : C->Out)
                    if (Seen.insert(O).second) Todo.push_back(O);
        }
        return false;
    }

    struct Dense {
        std::vector<float> W; // [out][in]
        std::vector<float> B;
        int Out = 0, In = 0;
        std::string Y;
    };

    Dense dense(const std::string& T, const Node& Nd) const {
        Dense D;
        if (Nd.Op == "Gemm" && !Nd.In.empty() && Nd.In[0] == T) {
            if (Nd.attrF("alpha", 1.0) != 1.0 || Nd.attrF("beta", 1.0) != 1.0 || Nd.attrI("transA", 0) != 0)
                fail(Nd, "Gemm with alpha = beta = 1, transA = 0 only");
            const Tensor& Wt = needFloat(Nd, 1, "weight");
            if (Wt.Dims.size() != 2) fail(Nd, "expected a 2-D weight");
            const bool TransB = Nd.attrI("transB", 0) != 0;
            D.Out = (int)(TransB ? Wt.Dims[0] : Wt.Dims[1]);
            D.In = (int)(TransB ? Wt.Dims[1] : Wt.Dims[0]);
            D.W.resize((size_t)D.Out * D.In);
            for (int O = 0; O < D.Out; ++O)
                for (int I = 0; I < D.In; ++I)
                    D.W[(size_t)O * D.In + I] = TransB ? Wt.F[(size_t)O * D.In + I] : Wt.F[(size_t)I * D.Out + O];
            D.B.assign((size_t)D.Out, 0.f);
            if (Nd.In.size() > 2 && !Nd.In[2].empty()) {
                const Tensor& B = needFloat(Nd, 2, "bias");
                if ((int)B.count() != D.Out) fail(Nd, "bias length does not match");
                D.B = B.F;
            }
            D.Y = Nd.Out[0];
            return D;
        }
        if (Nd.Op == "MatMul" && !Nd.In.empty() && Nd.In[0] == T) {
            const Tensor& Wt = needFloat(Nd, 1, "weight");
            if (Wt.Dims.size() != 2) fail(Nd, "expected a 2-D weight");
            D.In = (int)Wt.Dims[0];
            D.Out = (int)Wt.Dims[1];
            D.W.resize((size_t)D.Out * D.In);
            for (int O = 0; O < D.Out; ++O)
                for (int I = 0; I < D.In; ++I) D.W[(size_t)O * D.In + I] = Wt.F[(size_t)I * D.Out + O];
            const Node& Add = only(Nd.Out[0], "bias add");
            if (Add.Op != "Add") fail(Add, "expected MatMul + Add");
            const Tensor* B = nullptr;
            for (const std::string& I : Add.In)
                if (const Tensor* C = init(I)) B = C;
            if (!B || !B->IsFloat || (int)B->count() != D.Out) fail(Add, "expected a constant bias");
            D.B = B->F;
            D.Y = Add.Out[0];
            return D;
        }
        fail(Nd, "expected Gemm or MatMul+Add");
    }

    // the scalar constant among a binary node's inputs (the other input must be T)
    double scalarOperand(const Node& Nd, const std::string& T) const {
        if (Nd.In.size() != 2) fail(Nd, "expected two inputs");
        const bool First = Nd.In[0] == T;
        if (!First && Nd.In[1] != T) fail(Nd, "unexpected operand");
        if (Nd.Op == "Div" && !First) fail(Nd, "constant / x is not part of the value head");
        const Tensor* C = init(Nd.In[First ? 1 : 0]);
        if (!C || !C->IsFloat || C->count() != 1) fail(Nd, "expected a scalar float constant");
        return (double)C->F[0];
    }

    static constexpr double kEpsDefault = 1e-5;
    std::vector<double> EpsSeen;

 private:
    const Graph& G;
};

void put(std::vector<unsigned char>* Blob, const void* P, size_t N) {
    const unsigned char* B = (const unsigned char*)P;
    Blob->insert(Blob->end(), B, B + N);
}

void convert(Span Data, std::vector<unsigned char>* Blob) {
    const Graph G = readModel(Data);
    std::set<std::string> Ins;
    for (const std::string& I : G.Inputs)
        if (!G.Inits.count(I)) Ins.insert(I);
    const std::set<std::string> Outs(G.Outputs.begin(), G.Outputs.end());
    if (!Ins.count("input") || !Outs.count("policy") || !Outs.count("value") || !Outs.count("draw"))
        throw Error("tensor contract (trt.cc:144-227): need input 'input' and outputs 'policy', 'value', 'draw'");
    Matcher M(G);

    ConvBn Stem = M.convBn("input", M.only("input", "stem"), 3);
    std::string X = M.relu(Stem.Out);
    std::vector<ConvBn> Blocks; // w1, w2, w1, w2, ...
    for (;;) {
        const auto Cs = M.consumers(X);
        const Node* Conv3 = nullptr;
        const Node* Add = nullptr;
        int NumConv3 = 0, NumAdd = 0;
        for (const Node* C : Cs) {
            if (C->Op == "Add") { Add = C; ++NumAdd; }
            if (C->Op == "Conv" && C->In.size() > 1) {
                const Tensor* W = M.init(C->In[1]);
                if (W && W->Dims.size() == 4 && W->Dims[2] == 3 && W->Dims[3] == 3) { Conv3 = C; ++NumConv3; }
            }
        }
        if (!(NumConv3 == 1 && NumAdd == 1 && Cs.size() == 2)) break;
        ConvBn A = M.convBn(X, *Conv3, 3);
        const std::string Y = M.relu(A.Out);
        ConvBn B = M.convBn(Y, M.only(Y, "second conv of a block"), 3);
        const Node& Sum = M.only(B.Out, "residual add");
        const bool Operands = Sum.In.size() == 2 && ((Sum.In[0] == X && Sum.In[1] == B.Out) || (Sum.In[1] == X && Sum.In[0] == B.Out));
        if (&Sum != Add || !Operands) fail(Sum, "expected x + conv path");
        X = M.relu(Sum.Out[0]);
        Blocks.push_back(std::move(A));
        Blocks.push_back(std::move(B));
    }
    const auto Heads = M.consumers(X);
    if (Heads.size() != 2 || Heads[0]->Op != "Conv" || Heads[1]->Op != "Conv")
        throw Error("after " + std::to_string(Blocks.size() / 2) + " residual blocks expected the policy and value 1x1 convs");
    const bool FirstIsPolicy = M.reaches(Heads[0]->Out[0], "policy");
    const bool SecondIsPolicy = M.reaches(Heads[1]->Out[0], "policy");
    if (FirstIsPolicy == SecondIsPolicy) throw Error("cannot tell the policy head from the value head");
    const Node& PolNode = *Heads[FirstIsPolicy ? 0 : 1];
    const Node& ValNode = *Heads[FirstIsPolicy ? 1 : 0];

    ConvBn Pol = M.convBn(X, PolNode, 1);
    for (int I = 0; I < Pol.N; ++I)
        if (!Pol.NoBn)
            fail(PolNode, "the policy conv must be followed directly by the flatten (no BN)");
    {
        const Node& Fl = M.only(Pol.Out, "policy flatten");
        if ((Fl.Op != "Flatten" && Fl.Op != "Reshape") || Fl.Out[0] != "policy") fail(Fl, "expected Flatten/Reshape -> policy");
    }
    std::vector<float> PolB((size_t)Pol.N);
    for (int I = 0; I < Pol.N; ++I) PolB[I] = Pol.Stats[(size_t)Pol.N + I] - Pol.Stats[(size_t)2 * Pol.N + I];

    ConvBn Val = M.convBn(X, ValNode, 1);
    const std::string VRelu = M.relu(Val.Out);
    const Node& VFl = M.only(VRelu, "value flatten");
    if (VFl.Op != "Flatten" && VFl.Op != "Reshape") fail(VFl, "expected Flatten/Reshape");
    Matcher::Dense Fc1 = M.dense(VFl.Out[0], M.only(VFl.Out[0], "value MLP layer 1"));
    const std::string H = M.relu(Fc1.Y);

    std::vector<float> Fc2W((size_t)2 * Fc1.Out, 0.f);
    float Fc2B[2] = {0.f, 0.f};
    bool Have[2] = {false, false};
    for (const Node* Nd : M.consumers(H)) {
        Matcher::Dense D = M.dense(H, *Nd);
        if (D.Out != 1) fail(*Nd, "one dense node per output expected (value, draw)");
        float Scale = 1.f;
        std::string Name;
        const Node& Sq = M.only(D.Y, "output squashing");
        if (Sq.Op == "Tanh") { // (tanh(o) + 1) / 2
            const Node& A = M.only(Sq.Out[0], "tanh shift");
            if (A.Op != "Add" || M.scalarOperand(A, Sq.Out[0]) != 1.0) fail(A, "expected tanh + 1");
            const Node& S = M.only(A.Out[0], "tanh scale");
            const bool Half = (S.Op == "Mul" && M.scalarOperand(S, A.Out[0]) == 0.5) ||
                              (S.Op == "Div" && M.scalarOperand(S, A.Out[0]) == 2.0);
            if (!Half) fail(S, "expected (tanh + 1) * 0.5 or (tanh + 1) / 2");
            Name = S.Out[0];
            if (Name == "draw") Scale = 2.f; // the device evaluates draw as sigmoid(o): (tanh(z) + 1) / 2 = sigmoid(2 z)
        } else if (Sq.Op == "Sigmoid") {
            Name = Sq.Out[0];
            if (Name == "value") Scale = 0.5f; // sigmoid(z) = (tanh(z / 2) + 1) / 2
        } else {
            fail(Sq, "expected Tanh or Sigmoid");
        }
        const int Row = Name == "value" ? 0 : Name == "draw" ? 1 : -1;
        if (Row < 0) fail(Sq, "the value MLP must end in the outputs 'value' and 'draw'");
        if (D.In != Fc1.Out) fail(*Nd, "width does not match the hidden layer");
        for (int I = 0; I < D.In; ++I) Fc2W[(size_t)Row * Fc1.Out + I] = D.W[I] * Scale;
        Fc2B[Row] = D.B[0] * Scale;
        Have[Row] = true;
    }
    if (!Have[0] || !Have[1]) throw Error("value MLP outputs: need both 'value' and 'draw'");

    const int F = Stem.N, Cin = Stem.Cin, NumBlocks = (int)Blocks.size() / 2;
    for (const ConvBn& B : Blocks)
        if (B.N != F || B.Cin != F) throw Error("residual blocks must keep the trunk width");
    if (Pol.Cin != F || Val.Cin != F) throw Error("head convolutions must read the trunk");
    if (Fc1.In != Val.N * 81) throw Error("value MLP layer 1 must read value_channels * 81 features");
    if (Pol.N * 81 != 2187) throw Error("Unexpected PolicySize: " + std::to_string(Pol.N * 81) + " (expected: 2187)."); // trt.cc:205
    double Eps = M.EpsSeen.empty() ? Matcher::kEpsDefault : M.EpsSeen[0];
    for (double E : M.EpsSeen)
        if (std::fabs(E - Eps) > 1e-12) throw Error("the BatchNormalization nodes use different epsilons; the NSGW header holds one");
    // a conv without BN folds with scale 1 only if its variance + THIS model's epsilon is 1
    auto FinishIdentity = [&](ConvBn* C) {
        if (!C->NoBn) return;
        for (int I = 0; I < C->N; ++I) C->Stats[(size_t)3 * C->N + I] = (float)(1.0 - (double)(float)Eps);
    };
    FinishIdentity(&Stem);
    for (ConvBn& B : Blocks) FinishIdentity(&B);
    FinishIdentity(&Val);

    Blob->clear();
    unsigned char Header[64] = {0};
    std::memcpy(Header, "NSGW", 4);
    const uint32_t Hd[7] = {1u, (uint32_t)Cin, (uint32_t)F, (uint32_t)NumBlocks, (uint32_t)Pol.N, (uint32_t)Val.N, (uint32_t)Fc1.Out};
    std::memcpy(Header + 4, Hd, sizeof(Hd));
    const float EpsF = (float)Eps;
    std::memcpy(Header + 32, &EpsF, 4);
    put(Blob, Header, 64);
    auto PutF = [&](const std::vector<float>& V) { put(Blob, V.data(), V.size() * 4); };
    PutF(Stem.W); PutF(Stem.Stats);
    for (const ConvBn& B : Blocks) { PutF(B.W); PutF(B.Stats); }
    PutF(Pol.W); PutF(PolB);
    PutF(Val.W); PutF(Val.Stats);
    PutF(Fc1.W); PutF(Fc1.B);
    PutF(Fc2W);
    put(Blob, Fc2B, 8);
}

} // namespace

bool isNsgw(const void* Data, size_t Size) {
    return Size >= 4 && std::memcmp(Data, "NSGW", 4) == 0;
}

bool convertToNsgw(const void* Data, size_t Size, std::vector<unsigned char>* Blob, std::string* Error_) {
    try {
        convert(Span{(const unsigned char*)Data, Size}, Blob);
        return true;
    } catch (const std::exception& E) {
        if (Error_) *Error_ = E.what();
        return false;
    }
}

} // namespace onnx
} // namespace nsg
