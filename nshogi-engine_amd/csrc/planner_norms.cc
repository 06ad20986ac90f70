// planner_norms.cc -- the planner: the normalisations beyond a folded BatchNorm.
#include "planner.h"

namespace nsg::graph {

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
    L.name = N.Name;
    LayerNormArgs& A = L.args.emplace<LayerNormArgs>();
    A.in = ready(N.In[0]).v;
    L.out = freshView(C, Tok);
    A.wOff = addConst(Gm);
    A.biasOff = addConst(Bt);
    A.eps = (float)N.attrF("epsilon", 1e-5);
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
    L.name = Name;
    GroupNormArgs& Ga = L.args.emplace<GroupNormArgs>();
    Ga.in = In; // a view at any channel offset: the kernel reads it where it lies
    Ga.groups = G;
    Ga.act = Act;
    Ga.eps = (float)Eps;
    Ga.wOff = addConst(std::vector<float>(Gm.begin(), Gm.end()));
    Ga.biasOff = addConst(std::vector<float>(Bt.begin(), Bt.end()));
    L.out = freshView(C, true);
    Val V = runtimeVal(Last, Dims);
    V.v = L.out;
    emit(L);
    Vals[Cur] = V;
}

// ReduceMean over the last axis (given as -1 or as rank - 1) with keepdims = 1
bool Planner::lastAxis(const Node& N, const Val& X) {
    if (has(N, 1) && Vals.count(N.In[1]) && Vals.at(N.In[1]).runtime) return false;
    const std::vector<int64_t> Axes = axes(N, X.dims.size());
    return Axes.size() == 1 && Axes[0] == (int64_t)X.dims.size() - 1 && N.attrI("keepdims", 1) != 0;
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
    L.name = N.Name;
    for (const Node* A : Absorbed) {
        L.name += "+" + A->Name;
        Skip[indexOf(A)] = true;
    }
    const View In = ready(N.In[0]).v;
    L.out = freshView(C, X0.form != kFormPlain);
    const size_t WOff = addConst(Gm);
    if (Mean) L.args = LayerNormArgs{In, WOff, addConst(Bt), (float)Eps};
    else L.args = RmsNormArgs{In, WOff, (float)Eps};
    Val V = runtimeVal(*Y, X0.dims, X0.form);
    V.v = L.out;
    emit(L);
    Vals[Y->Out[0]] = V;
    return true;
}

// ---- F.normalize over the channels, as the exporter writes it:
//   n = ReduceL2(x) or ReduceL1(x) over the channel axis, keepdims 1;  c = Clip(n, min = eps);  [e = Expand(c, Shape(x))];
//   y = Div(x, e or c)
// with a constant scalar eps > 0, no max bound, the same x as the Div's numerator, and n, c, e read by the chain only (x
// may have other readers).  Matched forward from the reduction on the graph's structure; the nodes are held back (the
// Clip and the Expand in Skip) until the Div, where the Expand's target, folded by then, is checked against x's shape:
// one kLaunchNormalize.  A chain that starts like this and deviates is no error: normalizeOpen returns false and every
// node is lowered as it stands, a kLaunchChanReduce and elementwise nodes.
bool Planner::normalizeOpen(const Node& N, size_t Index) {
    const Val& X = get(N, 0);
    if (!channelAxis(N, X) || N.attrI("keepdims", 1) == 0 || !absorbable(N.Out[0])) return false;
    const Node* Cl = onlyConsumer(N.Out[0], Index);
    double Eps = 0;
    if (!Cl || Cl->Op != "Clip" || Cl->In.size() < 2 || Cl->In[0] != N.Out[0] || Cl->In[1].empty() || Cl->In[1] == N.Out[0] ||
        (Cl->In.size() > 2 && !Cl->In[2].empty()) || !scalarAhead(Cl->In[1], &Eps) || !((float)Eps > 0.f) || !absorbable(Cl->Out[0]))
        return false;
    PendingNormalize Pn;
    Pn.reduce = Index;
    Pn.interior = {indexOf(Cl)};
    Pn.p = N.Op == "ReduceL1" ? 1 : 2;
    Pn.eps = (float)Eps;
    const Node* Dv = onlyConsumer(Cl->Out[0], indexOf(Cl));
    if (Dv && Dv->Op == "Expand" && Dv->In.size() == 2 && Dv->In[0] == Cl->Out[0] && Dv->In[1] != Cl->Out[0] && absorbable(Dv->Out[0])) {
        Pn.interior.push_back(indexOf(Dv));
        Dv = onlyConsumer(Dv->Out[0], indexOf(Dv));
    }
    if (!Dv || Dv->Op != "Div" || Dv->In.size() != 2 || Dv->In[0] != N.In[0] || Dv->In[1] != Nodes[Pn.interior.back()].Out[0]) return false;
    for (size_t K : Pn.interior) Skip[K] = true;
    OpenNormalize[indexOf(Dv)] = Pn;
    return true;
}

bool Planner::normalizeClose(const Node& N, size_t Index) {
    const PendingNormalize Pn = OpenNormalize.at(Index);
    OpenNormalize.erase(Index);
    const Node& Rd = Nodes[Pn.reduce];
    const Val& X = get(Rd, 0);
    const int Kind = channelAxis(Rd, X);
    // the Expand is the view expandView would make of it: its target is the shape x has
    bool Fits = Kind != 0;
    if (Fits && Pn.interior.size() == 2) {
        const Node& Ex = Nodes[Pn.interior[1]];
        auto It = Vals.find(Ex.In[1]);
        std::vector<int64_t> One = X.dims, T;
        One[Kind == 2 ? 2 : 1] = 1;
        Fits = It != Vals.end() && !It->second.runtime && It->second.isInt && broadcast(One, It->second.i, &T) && T == X.dims;
    }
    if (!Fits) { // the chain's nodes one by one, here: nothing else reads what they compute
        reduceChannels(Rd);
        for (size_t K : Pn.interior) {
            Skip[K] = false;
            lower(Nodes[K], K);
        }
        return false;
    }
    Launch L;
    L.name = Rd.Name;
    for (size_t K : Pn.interior) L.name += "+" + Nodes[K].Name;
    L.name += "+" + N.Name;
    const int C = Kind == 2 ? (int)X.dims[2] : (int)X.dims[1];
    const std::vector<int64_t> Dims = X.dims;
    const int Form = X.form;
    L.args = NormalizeArgs{ready(Rd.In[0]).v, Pn.p, Pn.eps}; // a view at any channel offset
    L.out = freshView(C, Kind != 3);
    Val V = runtimeVal(N, Dims, Form);
    V.v = L.out;
    emit(L);
    Vals[N.Out[0]] = V;
    return true;
}

// ---- the normalisations beyond BatchNorm and the single LayerNormalization node.  Returns false when N is none.
bool Planner::normOp(const Node& N, size_t Index) {
    if (N.Op == "ReduceL1" || N.Op == "ReduceL2") return normalizeOpen(N, Index);
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

} // namespace nsg::graph
