// onnx_graph.cc -- see onnx_graph.h and DESIGN.md section 13.  The planner's entry points, the stages of a plan, the
// dispatch of one node, the outputs and the activation buffers; the ops themselves are in planner_*.cc.
#include "planner.h"

namespace nsg::graph {

// ---- the plan: its stages in order -----------------------------------------------------------------------------------
void Planner::run() {
    checkContract();
    Nodes = G.Nodes;
    P.nodes = (int)Nodes.size();
    Skip.assign(Nodes.size(), false);
    rewritePatterns(Nodes, Skip, G.Inits, Outputs);
    countUses();
    loadConstants();
    defineInput();
    for (size_t K = 0; K < Nodes.size(); ++K)
        if (!Skip[K]) lower(Nodes[K], K);
    checkOutputs();
    assignBuffers(P, VirtStride, VirtSpatial, VirtAlsoFlat, Trace);
}

// tensor contract (trt.cc:144-227), and the op set
void Planner::checkContract() {
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

    // (checked on the file's own nodes, before the rewrites name theirs)
    for (const Node& N : G.Nodes)
        if (!opSet().count(N.Op) && N.Op != "Swish" && N.Op != "Gelu") fail(N, "op '" + N.Op + "' is outside the supported op set (DESIGN.md section 13)");
}

// the live consumers of every tensor and the live node that computes it, after the rewrites
void Planner::countUses() {
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
}

void Planner::loadConstants() {
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
}

// the graph input: [N, numChannels, 9, 9] as the plane expansion writes it
void Planner::defineInput() {
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

// ---- one live node: folded on the host, taken by a pattern, or lowered to its launch ----------------------------------
void Planner::lower(const Node& N, size_t K) {
    const std::string& Op = N.Op;
    if (N.Out.empty()) fail(N, "no output");
    if (PendingMix.count(K)) return mixFlush(K); // the last node of a token-mixing pattern: its launch goes here
    // the Div of an F.normalize chain: its launch goes here, or (a chain that does not fit after all) its held-back nodes do
    if (OpenNormalize.count(K) && normalizeClose(N, K)) return;
    if (Op == "Constant") {
        if (!Vals.count(N.Out[0])) fail(N, "unsupported Constant attribute (value tensor or value_float only)");
        return;
    }
    bool AnyRuntime = false;
    for (const std::string& I : N.In)
        if (!I.empty()) {
            auto It = Vals.find(I);
            if (It == Vals.end()) fail(N, "input '" + I + "' is not defined before its use");
            AnyRuntime = AnyRuntime || It->second.runtime;
        }
    // an Expand of a one-channel tensor is a view that keeps the one-channel shape: only the ops that broadcast read it
    for (const std::string& I : N.In)
        if (!I.empty() && Vals.at(I).runtime && !Vals.at(I).expandTo.empty() && !isBinary(Op) && Op != "Max" && Op != "Min")
            fail(N, "input '" + I + "' is " + dimsStr(Vals.at(I).dims) + " behind an Expand to " + dimsStr(Vals.at(I).expandTo) +
                        ": the Expand is a view that only Add, Sub, Mul, Div, Max and Min read, broadcasting it themselves (DESIGN.md section 13.3)");
    if (Op == "Shape" || !AnyRuntime) return hostFold(N);
    // (Mod is in the op set for the host's shape chains alone)
    if (Op == "Mod") fail(N, "op 'Mod' is outside the supported op set (DESIGN.md section 13)");
    const Val& X = get(N, 0);
    double PowOne = 0;
    // a line tensor is read by the ops of planner_lines.cc only
    for (const std::string& I : N.In)
        if (!I.empty() && Vals.at(I).runtime && Vals.at(I).form == kFormLine) return lineOp(N, K);
    if (seqView(N) || formView(N) || attentionOp(N) || normOp(N, K) || lateResidual(N)) return;
    if (bmmOperands(N)) return bmm(N, K);
    if (mixEntry(N)) return tokenMix(N, K);
    // [N,C,81] and the 4-D tensors exist only inside the patterns the calls above follow
    for (size_t J = 0; J < N.In.size(); ++J) {
        if (N.In[J].empty()) continue;
        const Val& I = Vals.at(N.In[J]);
        if (I.runtime && (I.form == kFormGroup3 || I.normG > 0))
            fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " exists only inside the GroupNorm pattern: Reshape, InstanceNormalization, Reshape back to [N,C,9,9] (DESIGN.md section 13.3)");
        if (I.runtime && I.form == kFormChanLast)
            fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " is a channel-last view: only a LayerNorm over its last axis and Transpose [0,3,1,2] read it (DESIGN.md section 13.3)");
        if (I.runtime && I.form == kFormHeadRows) {
            if (Op == "MatMul" && J == 0 && has(N, 1) && !get(N, 1).runtime) return headRowsDense(N, K);
            fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " holds head rows [N,H,K]: only a MatMul with a constant [K,M] or the Reshape to an attention bias [N,H,81,81] reads them (DESIGN.md section 13.3)");
        }
        if (I.runtime && I.form == kFormScoreBias)
            fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " is a run-time attention bias: only the Add into the scores of the attention pattern reads it (DESIGN.md section 13.3)");
        if (I.runtime && (I.form == kFormSeqTok || I.form == kFormSeqRows)) {
            if ((Op == "MatMul" || Op == "Gemm") && J == 0 && has(N, 1) && !get(N, 1).runtime) return linear(N, K);
            fail(N, "input '" + N.In[J] + "' " + dimsStr(I.dims) + " holds the token rows seq-first: only a Linear (MatMul or Gemm with a constant weight), the Reshapes of nn.MultiheadAttention's export and Transpose [1,0,2] read it (DESIGN.md section 13.3)");
        }
        if (I.runtime && I.form >= kFormChan3)
            fail(N, "input '" + N.In[J] + "' " + I.shownStr() + " is consumed outside the token-view and attention patterns (DESIGN.md section 13.3)");
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
        powOne(N);
    } else if (isAct(Op) || isBinary(Op) || isEltExtra(Op) || Op == "BatchNormalization" || Op == "Pow") {
        if (Op == "BatchNormalization" && !X.runtime) fail(N, "expected a runtime input");
        if (isBinary(Op) && !get(N, 0).runtime && !get(N, 1).runtime) fail(N, "constant operands only");
        elementwise(N);
    } else if (Op == "MaxPool" || Op == "AveragePool") {
        pool(N);
    } else if (Op == "Split") {
        split(N);
    } else if (Op == "ReduceMin" || Op == "ReduceSum" || Op == "ReduceL1" || Op == "ReduceL2" || Op == "ReduceSumSquare" ||
               Op == "ReduceLogSumExp" || (Op == "ReduceMax" && channelAxis(N, X)) ||
               (Op == "ReduceMean" && channelAxis(N, X) > 1)) { // (a ReduceMean over the channels of a spatial tensor: refused below, as before)
        reduceChannels(N);
    } else if (Op == "GlobalAveragePool" || Op == "ReduceMean" || Op == "GlobalMaxPool" || Op == "ReduceMax") {
        reduceSquares(N);
    } else if (Op == "Expand") {
        expandView(N);
    } else if (Op == "Gather") {
        gather(N);
    } else if (X.form == kFormToken && Op != "Slice" && Op != "Identity") { // (Split on tokens is taken above)
        fail(N, "op '" + Op + "' is not supported on a token tensor " + dimsStr(X.dims));
    } else if (Op == "Flatten" || Op == "Reshape" || Op == "Squeeze" || Op == "Unsqueeze" || Op == "Identity") {
        viewOp(N);
    } else if (Op == "Concat") {
        concat(N);
    } else if (Op == "Slice") {
        slice(N);
    } else if (Op == "Cast") {
        fail(N, "applied to a runtime tensor (folded on shape values only)");
    } else {
        fail(N, "op '" + Op + "' is not supported on runtime tensors");
    }
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
        if (!It->second.expandTo.empty())
            outFail(O, "is " + dimsStr(It->second.dims) + " behind an Expand to " + dimsStr(It->second.expandTo) + ": the Expand is a view that only a broadcasting op reads");
        if (It->second.form == kFormLine)
            outFail(O, "is a line tensor " + dimsStr(It->second.dims) + ": it exists only between the rank / file pooling and the broadcast back onto the board (DESIGN.md section 13.3)");
        ready(O);
    }
    {
        const Val& V = Vals.at("policy"); // spatial C = 27, read as c * 81 + square, or flat C = 2187
        const int Width = V.flatOfSpatial || isSpatialDims(V.dims) ? V.v.C * 81 : flatC(V.dims);
        if (Width != 2187) outFail("policy", "has " + std::to_string(Width) + " values per position (expected: 2187)");
        P.policy = V.v;
    }
    for (const char* O : {"value", "draw"}) {
        const Val& V = Vals.at(O);
        if (V.flatOfSpatial || isSpatialDims(V.dims) || flatC(V.dims) != 1)
            outFail(O, "must hold one value per position, it is " + dimsStr(V.dims));
        (O[0] == 'v' ? P.value : P.draw) = V.v;
    }
}

// lifetimes -> physical buffers (a launch's output never shares a buffer with its inputs)
void assignBuffers(GraphPlan& P, const std::vector<int>& VirtStride, const std::vector<bool>& VirtSpatial,
                   const std::vector<int>& VirtAlsoFlat, LifetimeTrace* Trace) {
    const size_t NV = VirtStride.size();
    const int NL = (int)P.launches.size();
    std::vector<int> Last(NV, -1); // the last launch that touches each virtual buffer (NL: a graph output)
    for (int I = 0; I <= NL; ++I) {
        auto use = [&](View& V) {
            if (V.buf >= 0) Last[(size_t)V.buf] = std::max(Last[(size_t)V.buf], I);
        };
        if (I < NL) forEachView(P.launches[(size_t)I], use);
        else for (View* V : {&P.policy, &P.value, &P.draw}) use(*V);
    }
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
        // token rows read as flat rows too: a dense launch reads whole groups of 81 boards at that stride
        P.bufFlatStride[(size_t)Best] = std::max(P.bufFlatStride[(size_t)Best], VirtAlsoFlat[(size_t)V]);
        Phys[(size_t)V] = Best;
    };
    for (int I = 0; I < NL; ++I) {
        // (the two poolings of an 18-line block write one virtual buffer: it is taken once)
        if (Phys[(size_t)P.launches[(size_t)I].out.buf] < 0) take(P.launches[(size_t)I].out.buf);
        for (size_t V = 0; V < NV; ++V)
            if (Last[V] == I && Phys[V] >= 0) Free[(size_t)Phys[V]] = true;
    }
    auto rename = [&](View& V) {
        if (V.buf == kPending) throw Error("internal planner error: a launch reads an elementwise result before it is computed");
        if (V.buf >= 0) V.buf = Phys[(size_t)V.buf];
    };
    // the renaming, and beside it the record of what was renamed (LifetimeTrace)
    LifetimeTrace Unkept;
    LifetimeTrace& T = Trace ? *Trace : Unkept;
    T.virtStride = VirtStride;
    T.virtSpatial = VirtSpatial;
    T.virtAlsoFlat = VirtAlsoFlat;
    T.virtPhys = Phys;
    auto traced = [&](std::vector<ViewTrace>& Row, const char* Name, View& V) {
        ViewTrace R;
        R.field = Name;
        R.virt = V.buf;
        rename(V);
        R.v = V;
        Row.push_back(R);
    };
    T.launches.resize(P.launches.size());
    for (size_t I = 0; I < P.launches.size(); ++I)
        forEachNamedView(P.launches[I], [&](const char* Name, View& V) { traced(T.launches[I], Name, V); });
    traced(T.outputs, "policy", P.policy);
    traced(T.outputs, "value", P.value);
    traced(T.outputs, "draw", P.draw);
    size_t Bytes = (size_t)P.planeStride * 81 * 4;
    for (size_t K = 0; K < P.bufSpatialStride.size(); ++K)
        Bytes += 4 * std::max((size_t)P.bufSpatialStride[K] * 81, (size_t)P.bufFlatStride[K]);
    P.activationBytesPerPosition = Bytes;
}

bool buildPlan(const void* Data, size_t Size, int NumChannels, GraphPlan* Plan, std::string* Err) {
    return buildPlanTraced(Data, Size, NumChannels, Plan, nullptr, Err);
}

bool buildPlanTraced(const void* Data, size_t Size, int NumChannels, GraphPlan* Plan, LifetimeTrace* Trace, std::string* Err) {
    try {
        const Graph G = readModel(Span{(const unsigned char*)Data, Size});
        GraphPlan P;
        P.numChannels = NumChannels;
        LifetimeTrace T;
        Planner(G, NumChannels, &P, Trace ? &T : nullptr).run();
        if (Trace) *Trace = std::move(T);
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

} // namespace nsg::graph
