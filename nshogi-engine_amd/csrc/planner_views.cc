// planner_views.cc -- the planner: views, channel ops and the attention pattern.
#include "planner.h"

namespace nsg::graph {

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

// [N,C,81] tensor T is read by Transposes alone, [0,2,1] to tokens or [2,0,1] to the seq-first tokens, and by one of the
// latter at least: what the exporter writes for tokens that go into a stock transformer module
bool Planner::seqReaders(const std::string& T) const {
    if (Outputs.count(T)) return false;
    bool Seq = false;
    for (size_t K = 0; K < Nodes.size(); ++K) {
        if (Skip[K] || Nodes[K].Op == "Shape") continue;
        for (const std::string& I : Nodes[K].In) {
            if (I != T) continue;
            const std::vector<int64_t> Perm = Nodes[K].attrInts("perm", {});
            const bool S = Perm == std::vector<int64_t>{2, 0, 1};
            if (Nodes[K].Op != "Transpose" || !(S || Perm == std::vector<int64_t>{0, 2, 1})) return false;
            Seq = Seq || S;
        }
    }
    return Seq;
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
        // ([N,C,81] read seq-first as well, by Transpose [2,0,1]: both Transposes are views of the same rows, seqView)
        if (F >= kFormChan3 && !(F == kFormChan3 && seqReaders(N.In[0]))) interior(N, 0);
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
    if (F == kFormPlain && !PlainSpatial) return flatFormView(N, X0);
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
    if ((F == kFormToken || F == kFormHeadRows) && flatFormView(N, X0)) return true;
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
        const Val V = headsSource(N, X0);
        if (V.v.offset % 4 != 0) fail(N, "'" + N.In[0] + "' starts at channel " + std::to_string(V.v.offset) + " of its row: the attention kernel reads views at multiples of 4");
        return set(V, kFormTok4, ND);
    }
    if (F == kFormTokOut4) { // the Reshape that closes the pattern: one launch
        const int64_t H = X0.dims[2], Hd = X0.dims[3];
        if (ND != std::vector<int64_t>{kBatch, 81, H * Hd})
            fail(N, "the attention output " + dimsStr(X0.dims) + " is reshaped to " + dimsStr(ND) + ", not to [N,81,H*d]");
        attentionLaunch(N, X0, ND);
        return true;
    }
    fail(N, "Reshape of " + dimsStr(X0.dims) + " is outside the token-view and attention patterns (DESIGN.md section 13.3)");
}

// The views around a bias generator, none of which costs a launch:
//   token [N,81,C] -> flat [N,81*C] in the tokens' own order sq * C + c, C a multiple of 16: a board's 81 rows are contiguous
//   flat [N,H*K] -> head rows [N,H,K], K a multiple of 16: rows of (board, head) at stride K
//   flat [N,H*6561] or [N,6561], head rows [N,H,6561] -> the run-time attention bias [N,H,81,81] or [N,1,81,81]
// Returns false when N is none of them (the caller goes on, and refuses what nothing takes).
bool Planner::flatFormView(const Node& N, const Val& X0) {
    const int F = X0.form;
    auto put = [&](Val V, int Form, const std::vector<int64_t>& Dims) {
        V.form = Form;
        V.dims = Dims;
        V.producer = N.Name;
        V.chain.clear();
        V.group = -1;
        Vals[N.Out[0]] = V;
        return true;
    };
    if (F == kFormToken) {
        const int64_t C = X0.dims[2];
        if (N.Op == "Flatten" ? N.attrI("axis", 1) != 1 : reshapeTarget(N, X0.dims) != std::vector<int64_t>{kBatch, 81 * C}) return false;
        if (C % kChunk != 0)
            fail(N, "a token tensor " + dimsStr(X0.dims) + " flattened to [N," + std::to_string(81 * C) + "]: a board's 81 rows are contiguous only when C is a multiple of " +
                        std::to_string(kChunk) + " (C = " + std::to_string(C) + ")");
        const View Src = plain(N.In[0], N.Name + " (input copy)");
        if (Src.buf < 0) fail(N, "the graph input viewed as tokens cannot be flattened in the tokens' order");
        VirtAlsoFlat[(size_t)Src.buf] = std::max(VirtAlsoFlat[(size_t)Src.buf], (int)(81 * C));
        Val V = Vals.at(N.In[0]);
        V.v.stride = V.v.C = (int)(81 * C);
        V.v.spatial = false;
        return put(V, kFormPlain, {kBatch, 81 * C});
    }
    if (N.Op != "Reshape") {
        if (F == kFormHeadRows) fail(N, N.Op + " of head rows " + dimsStr(X0.dims) + ": only a MatMul with a constant [K,M] or the Reshape to an attention bias [N,H,81,81] reads them");
        return false;
    }
    if (F == kFormHeadRows) {
        const std::vector<int64_t> ND = reshapeTarget(N, X0.dims);
        const int64_t H = X0.headRows;
        if (ND != std::vector<int64_t>{kBatch, H, 81, 81})
            fail(N, "head rows " + dimsStr(X0.dims) + " can become an attention bias [N,H,81,81] (K = 6561), not " + dimsStr(ND));
        Val V = X0;
        V.rtHead = H == 1 ? 0 : X0.v.stride;
        V.v.stride = (int)H * X0.v.stride;
        V.v.C = (int)H * X0.v.stride;
        V.headRows = 0;
        return put(V, kFormScoreBias, ND);
    }
    if (X0.flatOfSpatial || X0.dims.size() != 2 || flatC(X0.dims) <= 0) return false;
    const Val& ShV = get(N, 1);
    if (ShV.runtime) return false;
    const std::vector<int64_t> ND = reshapeTarget(N, X0.dims);
    if (flatC(ND) >= 0) return false;
    if (ND.size() == 3) {
        const int64_t H = ND[1], K = ND[2];
        if (H <= 0 || K <= 0) return false;
        // head rows only where something reads them as such -- a MatMul (its data input) or the score-bias Reshape;
        // any other [N,A,B] of a flat tensor keeps the refusal it had
        bool Read = false;
        for (size_t J = indexOf(&N) + 1; J < Nodes.size(); ++J)
            Read = Read || (!Skip[J] && (Nodes[J].Op == "MatMul" || Nodes[J].Op == "Reshape") && !Nodes[J].In.empty() && Nodes[J].In[0] == N.Out[0]);
        if (!Read) return false;
        if (K % kChunk != 0)
            fail(N, "head rows " + dimsStr(ND) + " of a flat " + dimsStr(X0.dims) + ": the rows of (board, head) are rows of the layout only when K is a multiple of " +
                        std::to_string(kChunk) + " (K = " + std::to_string(K) + ")");
        plain(N.In[0], N.Name + " (input copy)");
        Val V = Vals.at(N.In[0]);
        V.v.stride = V.v.C = (int)K;
        V.headRows = (int)H;
        return put(V, kFormHeadRows, ND);
    }
    if (ND.size() == 4 && ND[1] > 0 && ND[2] == 81 && ND[3] == 81) {
        Val V = ready(N.In[0]);
        V.rtHead = ND[1] == 1 ? 0 : 81 * 81;
        return put(V, kFormScoreBias, ND);
    }
    return false;
}

// The token tensor a Reshape splits into heads.  q * scale (or k * scale) right before the split: an open group of one
// scalar Mul / Div is folded into the scale and never launched.
Val Planner::headsSource(const Node& N, const Val& X0) {
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
                Val V = X0;
                V.group = -1;
                V.v = Rt->v;
                V.scale = Mul ? (double)Cs->scalar : 1.0 / (double)Cs->scalar;
                V.chain = Gr.name;
                Groups[(size_t)X0.group].open = false;
                return V;
            }
        }
    }
    Val V = ready(N.In[0]);
    V.scale = 1.0;
    V.chain.clear();
    return V;
}

// The Reshape of [N,81,H,d] to ND = [N,81,H*d] that closes the attention pattern: its one launch
// (OutForm: kFormToken, or the seq-first form the closing Reshape of nn.MultiheadAttention's export names, X0 then [81,N,H,d])
void Planner::attentionLaunch(const Node& N, const Val& X0, const std::vector<int64_t>& ND, int OutForm) {
    const int64_t H = X0.dims[2], Hd = X0.dims[3];
    Launch L;
    L.name = X0.chain + "+" + N.Name;
    AttentionArgs& A = L.args.emplace<AttentionArgs>();
    A.in = X0.attQ;
    A.attK = X0.attK;
    A.attV = X0.attV;
    A.heads = (int)H;
    A.headDim = (int)Hd;
    A.scale = (float)X0.scale;
    A.hasBias = !X0.bias.empty();
    if (A.hasBias) {
        std::vector<float> Bf(X0.bias.begin(), X0.bias.end());
        A.biasOff = addConst(Bf);
    }
    A.hasRtBias = X0.hasRt;
    if (A.hasRtBias) {
        A.rtBias = X0.rtBias;
        A.rtHeadStride = X0.rtHead;
        A.rtScale = (float)X0.rtScale;
    }
    L.out = freshView((int)(H * Hd), true);
    P.flopsPerPosition += 2.0 * (2.0 * 81 * 81 * (double)Hd) * (double)H; // q k^T and probs x v
    Val V;
    if (OutForm == kFormToken) {
        V = runtimeVal(N, ND, kFormToken);
    } else {
        V.runtime = true;
        V.dims = ND;
        V.form = OutForm;
        V.producer = N.Name;
    }
    V.v = L.out;
    emit(L);
    Vals[N.Out[0]] = V;
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
        if (FA != kFormScores) fail(N, "Softmax on " + A.shownStr() + ": only the softmax over the keys of [N,H,81,81] attention scores is supported");
        int64_t Axis = N.attrI("axis", -1);
        if (Axis < 0) Axis += A.bh ? 3 : 4;
        if (A.bh) ++Axis; // the 3-D scores [N*H,81,81]
        if (Axis != 3) fail(N, "Softmax over axis " + std::to_string(N.attrI("axis", -1)) + " of the attention scores: the keys (axis -1) only");
        interior(N, 0);
        return put(A, kFormProbs, A.dims);
    }
    if (Op == "MatMul") {
        if (isAttForm(FA) && isAttForm(FB) && A.bh != B->bh)
            fail(N, "MatMul of " + A.shownStr() + " and " + B->shownStr() + ": one operand is on the (board x head) axis, the other is not");
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
        fail(N, "MatMul of " + A.shownStr() + " and " + B->shownStr() + " is outside the attention pattern (q k^T, then softmax x v; DESIGN.md section 13.3)");
    }
    // Mul / Div / Add with a constant
    const bool AR = isAttForm(FA);
    const Val& T = AR ? A : *B;
    const Val& Cst = AR ? *B : A;
    if (Op == "Add" && T.viaSeq)
        fail(N, "an Add on the attention scores " + T.shownStr() + " of nn.MultiheadAttention's export form: attn_mask, key_padding_mask and is_causal are outside "
                "the stock-module pattern (a mask of -inf entries is no constant bias of the attention launch; DESIGN.md section 13.3)");
    if (Cst.runtime) {
        // one bias computed at run time, a view of a flat or head-row tensor, added to the scores
        if (Op != "Add" || T.form != kFormScores)
            fail(N, "the other operand of " + Op + " on " + dimsStr(T.dims) + " is computed at run time: only constants enter the attention pattern, and one run-time bias its scores");
        if (Cst.form != kFormScoreBias)
            fail(N, "a run-time tensor " + dimsStr(Cst.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)Cst.v.C * 81} : Cst.dims) + " ('" + N.In[AR ? 1 : 0] +
                        "') is added to the attention scores " + dimsStr(T.dims) + ": only a Reshape of a flat or head-row tensor to [N,H,81,81] or [N,1,81,81] is a run-time bias (DESIGN.md section 13.3)");
        if (T.hasRt) fail(N, "a second run-time Add on the attention scores: the pattern takes one run-time bias");
        const int64_t H = T.dims[1], BH = Cst.dims[1];
        if (BH != H && BH != 1)
            fail(N, "the run-time bias " + dimsStr(Cst.dims) + " has " + std::to_string(BH) + " heads, the attention scores " + dimsStr(T.dims) + " have " + std::to_string(H));
        interior(N, 0);
        interior(N, 1);
        if (Cst.v.offset + (BH - 1) * (int64_t)Cst.rtHead + 81 * 81 > Cst.v.stride) fail(N, "internal planner error: the run-time bias does not fit its rows");
        Val V = T;
        V.hasRt = true;
        V.rtBias = Cst.v;
        V.rtHead = Cst.rtHead;
        V.rtScale = 1.0;
        return put(V, kFormScores, T.dims);
    }
    interior(N, AR ? 0 : 1);
    if (Op == "Mul" || Op == "Div") {
        if (Cst.count() != 1) fail(N, "only a scalar constant scales the attention pattern's tensors");
        if (Op == "Div" && !AR) fail(N, "a constant divided by " + dimsStr(T.dims) + " is outside the attention pattern");
        if (T.form != kFormTok4 && T.form != kFormHeads && T.form != kFormHeadsT && T.form != kFormScores)
            fail(N, Op + " on " + dimsStr(T.dims) + " is outside the attention pattern");
        const double S = Op == "Mul" ? Cst.at(0) : 1.0 / Cst.at(0);
        // (a factor <= 0 would turn a run-time -inf, a closed key, into +inf or NaN)
        if (T.hasRt && !(S > 0.0)) fail(N, "a scalar factor of " + std::to_string(S) + " behind the run-time Add on the attention scores: only a positive factor scales a run-time bias");
        Val V = T;
        V.scale *= S;
        for (double& Bv : V.bias) Bv *= S;
        if (V.hasRt) V.rtScale *= S; // a factor in front of the run-time Add leaves that bias alone
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

// ---- Flatten / Reshape / Squeeze / Unsqueeze / Identity between [N,C,9,9], its flattened [N,C*81] and the flat shapes:
// no launch.  An open elementwise group read only here stays open: the reshaped tensor is its new result (a [N,C,9,9]
// group that becomes [N,C*81] is emitted first: the flattened view reads its buffer).
void Planner::viewOp(const Node& N) {
    const std::string& Op = N.Op;
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
        ND = reshapeTarget(N, SD);
    } else {
        std::vector<int64_t> Axes = axes(N, SD.size(), Op == "Unsqueeze");
        ND = SD;
        if (Op == "Unsqueeze") {
            std::sort(Axes.begin(), Axes.end());
            for (int64_t A : Axes) {
                if (A <= 0 || A > (int64_t)ND.size()) fail(N, "cannot unsqueeze the batch axis");
                ND.insert(ND.begin() + A, 1);
            }
        } else {
            std::vector<int64_t> Keep;
            for (size_t J = 0; J < SD.size(); ++J) {
                bool Drop = Axes.empty() ? (J > 0 && SD[J] == 1) : false;
                for (int64_t A : Axes) Drop = Drop || A == (int64_t)J;
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
}

// ---- Expand of a one-channel tensor to the shape its reader would broadcast it to anyway (what the exporter writes for
// gate.expand_as(x)): a view.  The value keeps its one-channel shape and remembers the target (Val::expandTo); the Add,
// Sub, Mul, Div, Max or Min that reads it broadcasts it (kSrcRowOne / kSrcBoardOne) and checks the target against its result.
void Planner::expandView(const Node& N) {
    const Val& X = get(N, 0);
    const std::vector<int64_t> XD = X.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)X.v.C * 81} : X.dims;
    const std::vector<int64_t> Sh = ints(N, 1, "the target shape");
    std::vector<int64_t> T;
    const bool Fits = broadcast(XD, Sh, &T);
    const bool Plain = X.form == kFormPlain && !X.flatOfSpatial;
    const bool View = Fits && (T == XD || (Plain && XD == std::vector<int64_t>{kBatch, 1, 9, 9} && isSpatialDims(T)) ||
                               (Plain && flatC(XD) == 1 && XD.size() == 4 && isSpatialDims(T)) ||
                               (X.form == kFormToken && XD == std::vector<int64_t>{kBatch, 81, 1} && isTokenDims(T)) ||
                               (Plain && flatC(XD) == 1 && XD.size() == T.size() && flatC(T) > 0));
    if (!View)
        fail(N, "Expand of " + dimsStr(XD) + " to " + dimsStr(Sh) + ": only a one-channel tensor expanded over the channels is a view "
                "([N,1,9,9] or [N,1,1,1] to [N,C,9,9], [N,81,1] to [N,81,C], [N,1] to [N,C]); nothing else is expanded");
    const bool MoveGroup = X.group >= 0 && absorbable(N.In[0]);
    Val V = MoveGroup ? X : ready(N.In[0]);
    V.producer = N.Name;
    if (T != XD) V.expandTo = T;
    if (MoveGroup) Groups[(size_t)V.group].out = N.Out[0];
    Vals[N.Out[0]] = V;
}

// ---- Concat along the channels: one kLaunchConcat
void Planner::concat(const Node& N) {
    const Val& X = get(N, 0);
    int64_t Ax = N.attrI("axis", 1);
    const size_t Rank = X.flatOfSpatial ? 2 : X.dims.size();
    if (Ax < 0) Ax += (int64_t)Rank;
    if (Ax != 1) fail(N, "Concat of runtime tensors along axis 1 only");
    if (N.In.size() > (size_t)kMaxCopySegs) fail(N, "more than " + std::to_string(kMaxCopySegs) + " inputs");
    Launch L;
    L.name = N.Name;
    std::vector<CopySeg>& Segs = L.args.emplace<ConcatSegs>().segs;
    int Total = 0;
    bool Sp = false;
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
        Segs.push_back(S);
    }
    L.out = freshView(Total, Sp);
    std::vector<int64_t> ND = Sp ? std::vector<int64_t>{kBatch, Total, 9, 9} : std::vector<int64_t>{kBatch, Total};
    if (!Sp) for (size_t J = 2; J < Rank; ++J) ND.push_back(1);
    Val V = runtimeVal(N, ND);
    V.v = L.out;
    emit(L);
    Vals[N.Out[0]] = V;
}

// ---- Slice along the channels: a view.  With step -1 over a whole board axis: a flip, one launch (planner_gather.cc)
void Planner::slice(const Node& N) {
    const bool WasFlat = get(N, 0).flatOfSpatial; // (the copy below makes it a flat tensor of its own)
    const Val Src = WasFlat ? (plain(N.In[0], N.Name + " (flatten)"), Vals.at(N.In[0])) : ready(N.In[0]);
    const std::vector<int64_t> St = ints(N, 1, "starts"), En = ints(N, 2, "ends");
    std::vector<int64_t> Axes = has(N, 3) ? ints(N, 3, "axes") : std::vector<int64_t>();
    const std::vector<int64_t> Sp = has(N, 4) ? ints(N, 4, "steps") : std::vector<int64_t>(St.size(), 1);
    if (Axes.empty()) for (size_t J = 0; J < St.size(); ++J) Axes.push_back((int64_t)J);
    if (St.size() != En.size() || Axes.size() != St.size() || Sp.size() != St.size()) fail(N, "malformed Slice");
    Val V = Src;
    V.producer = N.Name;
    const int64_t ChanAxis = Src.form == kFormToken ? 2 : 1;
    // step -1 over a whole board axis of a spatial tensor (x.flip(2), x.flip(3)): the squares re-ordered, one launch
    const bool Board = Src.form == kFormPlain && !WasFlat && isSpatialDims(Src.dims);
    bool FlipRanks = false, FlipFiles = false;
    for (size_t J = 0; J < Axes.size(); ++J) {
        int64_t A = Axes[J] < 0 ? Axes[J] + (int64_t)Src.dims.size() : Axes[J];
        if (Sp[J] == -1 && Board && (A == 2 || A == 3)) {
            // ONNX: the start is clamped to [0, 8], the end to [-1, 8]; the whole axis runs from 8 down to and excluding -1
            const int64_t S = std::max<int64_t>(0, std::min<int64_t>(St[J] < 0 ? St[J] + 9 : St[J], 8));
            const int64_t E = std::max<int64_t>(-1, std::min<int64_t>(En[J] < 0 ? En[J] + 9 : En[J], 8));
            if (S == 8 && E == -1 && !(A == 2 ? FlipRanks : FlipFiles)) {
                (A == 2 ? FlipRanks : FlipFiles) = true;
                continue;
            }
        }
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
    if (FlipRanks || FlipFiles) return flipBoard(N, V, FlipRanks, FlipFiles);
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

// ---- the seq-first forms: what the exporter writes for nn.MultiheadAttention, and so for nn.TransformerEncoderLayer
// and nn.TransformerEncoder ("stock transformer modules").  The module works on [81,N,E]; every
// tensor below is a view of the board-major token rows and costs no launch:
//   [N,C,81] -Transpose [2,0,1]-> [81,N,C] <-Transpose [1,0,2]-> tokens [N,81,C];  [81,N,C] <-Reshape-> [N*81,C]
//   a Linear (MatMul (+ Add) or Gemm) on [81,N,C] or [N*81,C] is the token Linear (linear, planner_linear.cc)
//   the packed projection [81,N,3E] -Reshape-> [81,N,3,E] -Unsqueeze 0-> [1,81,N,3,E] -Transpose [3,1,2,0,4]->
//     [3,81,N,1,E] -Squeeze 3-> [3,81,N,E] -Gather k, axis 0-> [81,N,E]: the view at channel k E of the QKV rows
//   [81,N,E] -Reshape-> [81,N*H,d] -Transpose [1,0,2]-> [N*H,81,d]: q, k and v on the (board x head) axis; k^T by
//     Transpose [1,2,0] of [81,N*H,d] or [0,2,1] of [N*H,81,d].  [N*H,81,d] -Reshape-> [N,H,81,d] joins the 4-D forms;
//     without it MatMul, Mul and Softmax work on the 3-D forms (attentionOp, Val::bh)
//   probs x v: [N,H,81,d] -Transpose [2,0,1,3]-> [81,N,H,d], or [N*H,81,d] -Transpose [1,0,2]-> [81,N*H,d]; the
//     Reshape to [N*81,E] (or [81,N,E]) closes the pattern: the one kLaunchAttention
// Returns false when N reads none of these forms and enters none (the caller goes on).
bool Planner::seqView(const Node& N) {
    using Dv = std::vector<int64_t>;
    const std::string& Op = N.Op;
    if (N.In.empty() || N.In[0].empty()) return false;
    auto It = Vals.find(N.In[0]);
    if (It == Vals.end() || !It->second.runtime) return false;
    const Val X0 = It->second;
    const int F = X0.form;
    const bool SeqForm = F >= kFormSeqTok && F <= kFormSeqOut;
    const bool Transpose = Op == "Transpose", Reshape = Op == "Reshape";
    const Dv Perm = Transpose ? N.attrInts("perm", {}) : Dv();
    const bool Enter = Transpose && ((F == kFormChan3 && Perm == Dv{2, 0, 1}) || (F == kFormToken && Perm == Dv{1, 0, 2}) ||
                                     (F == kFormHeadOut && !X0.bh && Perm == Dv{2, 0, 1, 3}));
    if (!SeqForm && !X0.bh && !Enter) return false;
    const bool PackedOp = F == kFormSeqPacked && (Op == "Unsqueeze" || Op == "Squeeze" || Op == "Gather");
    if (!Transpose && !Reshape && !PackedOp) return false; // a Linear, the attention pattern's arithmetic, or refused by the caller
    const std::string Shown = X0.shownStr();
    auto put = [&](Val V, int Form, Dv Dims, bool Chain) {
        V.form = Form;
        V.dims = std::move(Dims);
        V.producer = N.Name;
        if (Chain) V.chain += (V.chain.empty() ? "" : "+") + N.Name;
        else V.chain.clear();
        Vals[N.Out[0]] = V;
        return true;
    };
    // the views on the way back from a Linear keep it open for the residual Add behind them (lateResidual)
    auto passLinear = [&]() {
        auto Open = OpenLinear.find(N.In[0]);
        if (Open == OpenLinear.end()) return;
        if (dataUses(N.In[0]) == 1 && !Outputs.count(N.In[0])) OpenLinear[N.Out[0]] = Open->second;
        OpenLinear.erase(N.In[0]);
    };
    const Dv& D = X0.dims;
    if (Transpose) {
        if (F == kFormChan3) { // (the [0,2,1] Transpose beside this one is formView's)
            if (!seqReaders(N.In[0])) interior(N, 0);
            return put(X0, kFormSeqTok, {81, kBatch, D[1]}, false);
        }
        if (F == kFormToken) return put(ready(N.In[0]), kFormSeqTok, {81, kBatch, D[2]}, false);
        if (F == kFormSeqTok && Perm == Dv{1, 0, 2}) {
            passLinear();
            return put(X0, kFormToken, {kBatch, 81, D[2]}, false);
        }
        if (F != kFormSeqTok && F != kFormSeqRows && F != kFormSeqPacked) interior(N, 0);
        if (F == kFormSeqHeads && Perm == Dv{1, 0, 2}) return put(X0, kFormHeads, {kBatch, D[2], 81, D[3]}, true);
        if (F == kFormSeqHeads && Perm == Dv{1, 2, 0}) return put(X0, kFormHeadsT, {kBatch, D[2], D[3], 81}, true);
        if (F == kFormHeads && X0.bh && Perm == Dv{0, 2, 1}) return put(X0, kFormHeadsT, {kBatch, D[1], D[3], 81}, true);
        if (F == kFormHeadOut && Perm == (X0.bh ? Dv{1, 0, 2} : Dv{2, 0, 1, 3})) return put(X0, kFormSeqOut, {81, kBatch, D[1], D[3]}, true);
        if (F == kFormSeqPacked && D.size() == 5 && D[0] == 1 && Perm == Dv{3, 1, 2, 0, 4}) return put(X0, kFormSeqPacked, {D[3], D[1], D[2], 1, D[4]}, false);
        fail(N, "Transpose of " + Shown + " with perm " + dimsStr(Perm) + " is outside the seq-first forms of nn.MultiheadAttention's export (DESIGN.md section 13.3)");
    }
    if (PackedOp) {
        if (Op == "Unsqueeze" && D.size() == 4 && D[0] == 81 && axes(N, 4, true) == Dv{0}) return put(X0, kFormSeqPacked, {1, D[0], D[1], D[2], D[3]}, false);
        if (Op == "Squeeze" && D.size() == 5 && D[0] == 3 && D[3] == 1 && axes(N, 5) == Dv{3}) return put(X0, kFormSeqPacked, {D[0], D[1], D[2], D[4]}, false);
        if (Op == "Gather" && D.size() == 4 && D[0] == 3 && N.attrI("axis", 0) == 0) {
            const Val& Iv = host(N, 1, "Gather's indices");
            if (Iv.dims.empty() && Iv.count() == 1 && Iv.isInt && Iv.i[0] >= -3 && Iv.i[0] < 3) {
                const int64_t Part = (Iv.i[0] + 3) % 3;
                Val V = X0;
                V.v.offset += (int)(Part * D[3]);
                V.v.C = (int)D[3];
                V.packedPart = true;
                return put(V, kFormSeqTok, {81, kBatch, D[3]}, false);
            }
        }
        fail(N, Op + " of the packed q / k / v projection " + Shown + " is outside the split nn.MultiheadAttention's export writes: Reshape to [81,N,3,E], Unsqueeze 0, "
                    "Transpose [3,1,2,0,4], Squeeze 3, Gather of part 0, 1 or 2 along axis 0 (DESIGN.md section 13.3)");
    }
    // Reshape: the exporter writes every target of these forms in full
    const Dv Sh = ints(N, 1, "the target shape");
    for (int64_t S : Sh)
        if (S == 0 || S == -1) fail(N, "Reshape of " + Shown + " to " + dimsStr(Sh) + ": the target shapes of the seq-first forms are taken only when written in full");
    if (F == kFormSeqTok) {
        const int64_t C = D[2];
        if (Sh == Dv{batchTimes(81), C}) return put(X0, kFormSeqRows, Sh, false);
        // one head: the exporter drops the product N*1, and the head split of a part of the packed projection is the
        // Reshape to its own shape [81,N,E]
        const bool Split1 = Sh == D && X0.packedPart;
        if (Sh == D && !Split1) {
            passLinear();
            return put(X0, kFormSeqTok, D, false);
        }
        if (Sh.size() == 4 && Sh[0] == 81 && Sh[1] == kBatch && Sh[2] == 3 && Sh[3] * 3 == C) return put(X0, kFormSeqPacked, Sh, false);
        const int64_t H = Sh.size() == 3 ? batchFactor(Sh[1]) : 0;
        if (H < 1 || Sh[0] != 81 || Sh[2] <= 0 || H * Sh[2] != C)
            fail(N, "the seq-first tokens " + Shown + " can become [N*81,C], the packed projection [81,N,3,E] or the head split [81,N*H,d], not " + dimsStr(Sh));
        const int64_t Hd = Sh[2];
        if (!X0.packedPart)
            fail(N, "the head split " + dimsStr(Sh) + " of '" + N.In[0] + "', which is no part of a packed q / k / v projection: the stock-module pattern is self-attention "
                        "with one in_proj_weight; separate projections (kdim or vdim other than embed_dim, cross-attention) are outside it (DESIGN.md section 13.3)");
        if (Hd % 4 != 0 || Hd > kMaxHeadDim)
            fail(N, "head dimension " + std::to_string(Hd) + ": the attention kernel takes multiples of 4 up to " + std::to_string(kMaxHeadDim));
        if (X0.v.offset % 4 != 0) fail(N, "'" + N.In[0] + "' starts at channel " + std::to_string(X0.v.offset) + " of its row: the attention kernel reads views at multiples of 4");
        Val V = X0;
        V.scale = 1.0;
        V.packedPart = false;
        V.bh = V.viaSeq = true;
        V.chain.clear();
        return put(V, kFormSeqHeads, {81, kBatch, H, Hd}, true);
    }
    if (F == kFormSeqRows) {
        if (Sh != Dv{81, kBatch, D[1]}) fail(N, "the token rows " + Shown + " can become [81,N," + std::to_string(D[1]) + "] again, not " + dimsStr(Sh));
        passLinear();
        return put(X0, kFormSeqTok, Sh, false);
    }
    interior(N, 0);
    if (F == kFormHeads && X0.bh) {
        if (Sh != D) fail(N, "q, k or v on the (board x head) axis " + Shown + " can become " + dimsStr(D) + ", not " + dimsStr(Sh));
        Val V = X0;
        V.bh = false;
        return put(V, kFormHeads, D, true);
    }
    if (F == kFormSeqOut) { // the Reshape that closes the pattern: one launch
        const int64_t E = D[2] * D[3];
        const bool Rows = Sh == Dv{batchTimes(81), E};
        if (!Rows && Sh != Dv{81, kBatch, E})
            fail(N, "the attention output " + Shown + " is reshaped to " + dimsStr(Sh) + ", not to [N*81," + std::to_string(E) + "] or [81,N," + std::to_string(E) + "]");
        attentionLaunch(N, X0, Sh, Rows ? kFormSeqRows : kFormSeqTok);
        return true;
    }
    fail(N, "Reshape of " + Shown + " to " + dimsStr(Sh) + " is outside the seq-first forms of nn.MultiheadAttention's export (DESIGN.md section 13.3)");
}

// ---- x + (a seq-first Linear seen through its views back to tokens): the exporter's Shape nodes stand between the
// Linear and its residual Add, so the epilogue could not look ahead; the Add joins the launch here, as the residual the
// hand-written form's Linear takes.  Only while the Linear has no residual and no activation, its result has this one
// reader, and the residual was written before the Linear's launch.
bool Planner::lateResidual(const Node& N) {
    if (N.Op != "Add" || N.In.size() != 2 || N.In[0] == N.In[1]) return false;
    for (size_t Side = 0; Side < 2; ++Side) {
        const std::string& T = N.In[Side];
        const std::string& Other = N.In[1 - Side];
        auto Open = OpenLinear.find(T);
        if (Open == OpenLinear.end() || !Vals.count(Other)) continue;
        const Val& A = Vals.at(T);
        const Val& O = Vals.at(Other);
        if (A.form != kFormToken || !O.runtime || O.form != kFormToken || O.dims != A.dims || O.group >= 0 || !O.expandTo.empty()) continue;
        if (dataUses(T) != 1 || Outputs.count(T)) continue;
        const size_t At = Open->second;
        ConvArgs& C = std::get<ConvArgs>(P.launches[At].args);
        if (C.res.buf != kNoRes || C.act != kActNone) continue;
        bool Before = O.v.buf == -1; // the graph input
        for (size_t K = 0; K < At; ++K) Before = Before || P.launches[K].out.buf == O.v.buf;
        if (!Before) continue;
        C.res = O.v;
        P.launches[At].name += "+" + N.Name;
        Val V = A;
        V.producer = N.Name;
        OpenLinear.erase(Open);
        Vals[N.Out[0]] = V;
        return true;
    }
    return false;
}

} // namespace nsg::graph
