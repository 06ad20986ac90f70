// planner_mix.cc -- the planner: token-mixing MLPs, a Linear over the 81 squares ("token mixing").
#include "planner.h"

namespace nsg::graph {

// A MatMul of a run-time [N,C,81] tensor with a constant: the entry of the pattern.  (Two run-time operands went to
// bmmOperands before and keep that refusal.)
bool Planner::mixEntry(const Node& N) const {
    if (N.Op != "MatMul" || N.In.size() != 2) return false;
    auto A = Vals.find(N.In[0]), B = Vals.find(N.In[1]);
    return A != Vals.end() && B != Vals.end() && A->second.runtime && A->second.form == kFormChan3 && A->second.normG == 0 &&
           !B->second.runtime;
}

// The launch of a pattern that absorbed nodes, emitted at its last node (lower() finds it there).
void Planner::mixFlush(size_t Index) {
    auto It = PendingMix.find(Index);
    emit(It->second.L);
    Vals[It->second.out] = It->second.V;
    PendingMix.erase(It);
}

// One stage is MatMul with a constant [K,D'], constant Adds of a bias over the last axis, at most one parameter-free
// activation; the pattern is one stage [81,81] or two stages [81,D], [D,81].  The walk looks ahead from the first MatMul,
// as foldEpilogue does, and marks what it absorbs in Skip; the one kLaunchTokenMix is emitted where the pattern ends.
void Planner::tokenMix(const Node& N, size_t Index) {
    const Val X0 = get(N, 0);
    const int64_t C = X0.dims[1];
    auto uses = [&](const std::string& T) {
        auto U = Uses.find(T);
        auto S = ShapeUses.find(T);
        return (U == Uses.end() ? 0 : U->second) - (S == ShapeUses.end() ? 0 : S->second);
    };
    auto shape = [&](int64_t Last) { return dimsStr({kBatch, C, Last}); };
    if (Outputs.count(N.In[0]) || uses(N.In[0]) != 1)
        fail(N, "MatMul of '" + N.In[0] + "' " + shape(81) + " with a constant: the tensor has a second consumer; a [N,C,81] tensor is a view for one reader");

    struct Stage {
        int64_t K = 0, D = 0;
        std::vector<double> W, B; // W[k][d], row-major as the model holds it
        int act = kActNone;
    };
    std::vector<Stage> St;
    const Node* M = &N;
    size_t At = Index;
    std::string Name, Cur;
    int64_t Last = 81;
    const std::string Ref = " (DESIGN.md section 13.3)";
    auto absorb = [&](const Node* A) {
        Name += (Name.empty() ? "" : "+") + A->Name;
        if (A != &N) Skip[indexOf(A)] = true;
        At = indexOf(A);
        Cur = A->Out[0];
    };
    for (;;) {
        // M: the MatMul of the running tensor [N,C,Last] with a constant
        const Val& Wt = Vals.at(M->In[1]);
        const std::string Both = "MatMul of " + shape(Last) + " with a constant " + dimsStr(Wt.dims) + ": ";
        if (St.size() == 2)
            fail(*M, Both + "a third MatMul; a token-mixing pattern is one stage [81,81] or two stages [81,D] and [D,81]" + Ref);
        if (Wt.isInt || Wt.dims.size() != 2 || Wt.dims[0] < 1 || Wt.dims[1] < 1 || Wt.f.size() != (size_t)(Wt.dims[0] * Wt.dims[1]))
            fail(*M, Both + "a token-mixing stage takes a 2-D float weight [" + std::to_string(Last) + ",D]" + Ref);
        Stage S;
        S.K = Wt.dims[0];
        S.D = Wt.dims[1];
        if (S.K != Last)
            fail(*M, Both + "the constant's first dimension is " + std::to_string(S.K) + ", the tensor's last one is " + std::to_string(Last));
        if (St.empty() && S.D > kMaxMixHidden)
            fail(*M, Both + "D = " + std::to_string(S.D) + " hidden units; a token-mixing stage takes 1 to " + std::to_string(kMaxMixHidden) + Ref);
        if (!St.empty() && S.D != 81)
            fail(*M, Both + "the second stage of a token-mixing pattern goes back to the 81 squares, with a constant [" + std::to_string(Last) + ",81]" + Ref);
        S.W = Wt.f;
        S.B.assign((size_t)S.D, 0.0);
        St.push_back(S);
        Stage& T = St.back();
        absorb(M);
        Last = T.D;
        // the stage's epilogue, while the tensor has one reader
        const Node* Cn = nullptr;
        for (;;) {
            Cn = absorbable(Cur) ? onlyConsumer(Cur, At) : nullptr;
            if (!Cn) break;
            const std::string On = " " + shape(Last) + " inside a token-mixing pattern: ";
            if (Cn->Op == "Add" && Cn->In.size() == 2 && Cn->In[0] != Cn->In[1] && T.act == kActNone) {
                const std::string& Other = Cn->In[0] == Cur ? Cn->In[1] : Cn->In[0];
                auto It = Vals.find(Other);
                if (It == Vals.end() || It->second.runtime)
                    fail(*Cn, "Add of '" + Other + "' to" + On + "the bias is computed at run time; a stage takes constant biases over the last axis" + Ref);
                const Val& O = It->second;
                const std::vector<int64_t>& OD = O.dims;
                bool Lead = OD.size() <= 3; // [D], [1,D], [1,1,D], or one element
                for (size_t J = 0; J + 1 < OD.size(); ++J) Lead = Lead && OD[J] == 1;
                if (!(O.count() == 1 || (Lead && !OD.empty() && OD.back() == Last && (int64_t)O.count() == Last)))
                    fail(*Cn, "Add of a constant " + dimsStr(OD) + " to" + On + "the bias varies along C or does not fit the last axis; a stage takes a bias of shape [D], [1,D] or [1,1,D]" + Ref);
                for (int64_t J = 0; J < Last; ++J) T.B[(size_t)J] += O.at(O.count() == 1 ? 0 : (size_t)J);
            } else if (!Cn->In.empty() && Cn->In[0] == Cur && T.act == kActNone && nodeAct(*Cn) != kActNone) {
                T.act = nodeAct(*Cn);
            } else if (!Cn->In.empty() && Cn->In[0] == Cur && T.act == kActNone &&
                       (Cn->Op == "LeakyRelu" || Cn->Op == "PRelu" || Cn->Op == "Clip" || Cn->Op == "HardSigmoid")) {
                fail(*Cn, Cn->Op + " on" + On + "an activation with a parameter does not fold into the launch, only the parameter-free ones do" + Ref);
            } else {
                break;
            }
            absorb(Cn);
        }
        // the next stage: a MatMul of this tensor with a constant
        if (Cn && Cn->Op == "MatMul" && Cn->In.size() == 2 && Cn->In[0] == Cur && Cn->In[1] != Cur) {
            auto It = Vals.find(Cn->In[1]);
            if (It != Vals.end() && !It->second.runtime) {
                M = Cn;
                continue;
            }
        }
        if (Last != 81) { // the hidden tensor [N,C,D] fits no tensor kind: it lives inside the launch only
            const std::string Hid = "'" + Cur + "' " + shape(Last) + ", the hidden tensor of a token-mixing pattern";
            if (!Cn)
                fail(Nodes[At], Hid + ", is an interior tensor and has " + (Outputs.count(Cur) ? std::string("a graph output as") : std::to_string(uses(Cur)) + " consumers, not") +
                                    " one; it never leaves the launch" + Ref);
            fail(*Cn, "input " + Hid + " (D = " + std::to_string(Last) + ", not 81), is read by the second stage's nodes only: constant Adds over the last axis, one parameter-free activation, and the MatMul with a constant [" +
                          std::to_string(Last) + ",81]" + Ref);
        }
        break;
    }

    // the constant record: W1^T [Dp][84], b1 [Dp], W2^T [96][Dp], b2 [96], folded in double and rounded once
    const bool Two = St.size() == 2;
    const int D = (int)St[0].D, Dp = roundUp(D, kChunk);
    std::vector<float> Rec((size_t)Dp * 84 + Dp + (Two ? (size_t)96 * Dp + 96 : 0), 0.f);
    for (int Dd = 0; Dd < D; ++Dd) {
        for (int S = 0; S < 81; ++S) Rec[(size_t)Dd * 84 + S] = (float)St[0].W[(size_t)S * D + Dd];
        Rec[(size_t)Dp * 84 + Dd] = (float)St[0].B[(size_t)Dd];
    }
    if (Two) {
        const size_t W2 = (size_t)Dp * 84 + Dp, B2 = W2 + (size_t)96 * Dp;
        for (int J = 0; J < 81; ++J) {
            for (int Dd = 0; Dd < D; ++Dd) Rec[W2 + (size_t)J * Dp + Dd] = (float)St[1].W[(size_t)Dd * 81 + J];
            Rec[B2 + J] = (float)St[1].B[(size_t)J];
        }
    }

    Launch L;
    L.name = Name;
    TokenMixArgs& A = L.args.emplace<TokenMixArgs>();
    // a view at a multiple of 4 is read where it lies, any other is copied into rows of its own first
    A.in = ready(N.In[0]).v;
    if (A.in.offset % 4 != 0) Vals[N.In[0]].v = A.in = copyOf(A.in, true, N.Name + " (input copy)");
    A.wOff = addConst(Rec);
    A.mixD = D;
    A.mixStages = Two ? 2 : 1;
    A.act = St[0].act;
    A.mixAct2 = Two ? St[1].act : kActNone;
    L.out = freshView((int)C, true);
    P.flopsPerPosition += 2.0 * 81 * (double)D * (double)C * (Two ? 2.0 : 1.0);
    Val V = X0;
    V.form = kFormChan3;
    V.dims = {kBatch, C, 81};
    V.v = L.out;
    V.group = -1;
    V.producer = Nodes[At].Name;
    V.chain.clear();
    if (At == Index) {
        emit(L);
        Vals[Cur] = V;
        return;
    }
    Skip[At] = false; // the pattern's last node stays live: lower() reaches it and emits the launch there
    PendingMix[At] = PendingLaunch{L, Cur, V};
}

} // namespace nsg::graph
