// planner_elementwise.cc -- the planner: elementwise ops fused into groups.
#include "planner.h"

namespace nsg::graph {

// The program of one elementwise node, behind the programs of the open groups it inlines.
struct EltBuilder {
    Planner& Pl;
    const Node& N;
    std::vector<std::vector<int64_t>> InDims;
    std::vector<int64_t> D; // the result's dims
    bool Tok = false, Spatial = false;
    int Lines = 0; // > 0: the result is a line tensor of that many lines per board
    int C = 0, ChanAxis = 1;
    size_t Arity = 1;
    // what the node adds to the program behind its operands, beyond one instruction and one register: set by budget()
    int XSrcs = 0, XCode = 0, XRegs = 0;
    Group NG;

    EltBuilder(Planner& Pl, const Node& N) : Pl(Pl), N(N) {}
    [[noreturn]] void fail(const std::string& Why) const { Pl.fail(N, Why); }
    void budget(int Srcs, int CodeAndRegs) { XSrcs = Srcs, XCode = XRegs = CodeAndRegs; }
    int instr(int Code, int A, int B) {
        const int R = NG.nregs++;
        NG.code.push_back(EltInstr{(uint8_t)Code, (uint8_t)R, (uint8_t)A, (uint8_t)B});
        return R;
    }
    // a new source, read into a new register
    int load(const EltSrc& S) {
        if (NG.srcs.size() >= (size_t)kMaxEltSrcs) fail("too many inputs for one fused launch");
        NG.srcs.push_back(S);
        return instr(kEltLoad, (int)NG.srcs.size() - 1, 0);
    }
    int scalarReg(double Value) {
        EltSrc S;
        S.mode = kSrcScalar;
        S.scalar = (float)Value;
        return load(S);
    }
    int channelReg(const std::vector<float>& PerChannel) {
        EltSrc S;
        S.mode = kSrcChannel;
        S.constOff = Pl.addConst(PerChannel);
        return load(S);
    }
    double bound(size_t Idx, const char* Attr, const char* What) {
        if (!Pl.has(N, Idx)) return N.attrF(Attr, 0.0);
        const Val& B = Pl.host(N, Idx, What);
        if (B.count() != 1 || (B.isInt && B.i[0] == kBatch)) fail(std::string(What) + " must be a scalar constant");
        return B.at(0);
    }
    int constOperand(size_t K, const Val& V);
    int operand(size_t K);
    int expand(int ActCode, double PowE);
};

// a constant operand: a scalar, one value per channel, or one per (square, channel)
int EltBuilder::constOperand(size_t K, const Val& V) {
    const std::vector<int> Ax = variesAlong(InDims[K], D.size());
    if (Ax.empty()) {
        if (V.count() < 1) fail("empty constant");
        return scalarReg(V.at(0));
    }
    if (Ax.size() == 1 && Ax[0] == ChanAxis && D.size() >= 2) {
        std::vector<float> F((size_t)C);
        for (int Ch = 0; Ch < C; ++Ch) F[(size_t)Ch] = (float)V.at((size_t)Ch);
        return channelReg(F);
    }
    if ((Tok && Ax == std::vector<int>{1, 2}) || (Spatial && Ax == std::vector<int>{1, 2, 3})) {
        // a learned positional embedding, [81,C] on tokens or [C,9,9] on a spatial tensor: stored [square][C]
        if (V.count() != (size_t)C * 81) fail("constant of shape " + dimsStr(InDims[K]) + " does not cover " + dimsStr(D));
        std::vector<float> F((size_t)C * 81);
        for (int Sq = 0; Sq < 81; ++Sq)
            for (int Ch = 0; Ch < C; ++Ch)
                F[(size_t)Sq * C + Ch] = (float)V.at(Tok ? (size_t)Sq * C + Ch : (size_t)Ch * 81 + Sq);
        EltSrc S;
        S.mode = kSrcSquareChannel;
        S.constOff = Pl.addConst(F);
        return load(S);
    }
    if (N.Op != "PRelu" && ((Tok && Ax == std::vector<int>{1}) || (Spatial && Ax == std::vector<int>{2, 3}))) {
        // one value per square, [1,81,1] on tokens or [1,1,9,9] on a spatial tensor (a mask, a promotion-zone bias): 81 floats
        if (V.count() != 81) fail("constant of shape " + dimsStr(InDims[K]) + " does not cover the squares of " + dimsStr(D));
        std::vector<float> F(81);
        for (size_t Sq = 0; Sq < 81; ++Sq) F[Sq] = (float)V.at(Sq);
        EltSrc S;
        S.mode = kSrcSquare;
        S.constOff = Pl.addConst(F);
        return load(S);
    }
    if (Lines)
        fail("constant of shape " + dimsStr(InDims[K]) + " on the line tensor " + dimsStr(D) +
             ": a per-(line, channel) constant is not supported on a line tensor (per-channel and scalar constants only)");
    fail("constant of shape " + dimsStr(InDims[K]) + " broadcast to " + dimsStr(D) +
         " (per-channel, per-square, per-(square, channel) and scalar constants only)");
}

// operand K -> the register that holds it
int EltBuilder::operand(size_t K) {
    const std::string& Name = N.In[K];
    Val& V = Pl.Vals.at(Name);
    if (!V.runtime) return constOperand(K, V);
    // runtime operand: how it varies relative to the output
    const std::vector<int64_t>& Di = InDims[K];
    const bool VLine = V.form == kFormLine;
    bool Same, Board = false;
    int Map = kSrcSame; // what a kSrcSame source of an inlined group becomes, and how the operand itself is loaded
    if (Lines || VLine) {
        // a line operand: of a line result with the same lines, or broadcast back onto the board
        if (Lines && !VLine && !V.flatOfSpatial && Planner::flatC(Di) >= 0)
            fail("a flat operand " + dimsStr(Di) + " ('" + Name + "') in a chain of line tensors " + dimsStr(D) +
                 ": a per-board value is broadcast over the 81 squares of a board only, not over its lines");
        Same = Lines && VLine && Di == D;
        const bool Back = Spatial && VLine && V.v.lines == 9 && Di[1] == C;
        if (!Same && !Back && VLine && Di[1] == 1 && C > 1)
            fail("the one-channel line operand " + dimsStr(Di) + " ('" + Name + "') against " + dimsStr(D) +
                 ": a one-channel tensor is broadcast over the channels of spatial, token and flat rows only, not over the channels of lines");
        if (!Same && !Back) fail("operand " + dimsStr(Di) + " broadcast to " + dimsStr(D) + " is not supported");
        if (Back) Map = Di[3] == 1 ? kSrcRankLine : kSrcFileLine;
    } else {
        Same = Tok ? (V.form == kFormToken && Di == D) : (Di == D || (Planner::flatC(Di) == C && !Spatial && Planner::flatC(D) == C));
        Board = !Tok && Spatial && !V.flatOfSpatial && Planner::flatC(Di) == C && Di.size() == 4;
        // one channel against C > 1: channel 0 of the operand's own row, or of its board's row
        const bool Arith = isBinary(N.Op) || N.Op == "Max" || N.Op == "Min";
        const bool Wide = Arith && C > 1 && !V.flatOfSpatial;
        const bool RowOne = Wide && (Tok ? V.form == kFormToken && Di == std::vector<int64_t>{kBatch, 81, 1}
                                     : Spatial ? V.form == kFormPlain && Di == std::vector<int64_t>{kBatch, 1, 9, 9}
                                               : V.form == kFormPlain && Planner::flatC(Di) == 1 && Planner::flatC(D) == C);
        const bool BoardOne = Wide && !Tok && Spatial && V.form == kFormPlain && Planner::flatC(Di) == 1 && Di.size() == 4;
        if (!Same && !Board && !RowOne && !BoardOne) fail("operand " + dimsStr(Di) + " broadcast to " + dimsStr(D) + " is not supported");
        if (!V.expandTo.empty() && V.expandTo != D)
            fail("'" + Name + "' is " + dimsStr(Di) + " expanded to " + dimsStr(V.expandTo) + ", the other operand makes the result " +
                 dimsStr(D) + ": an Expand is a view only where the broadcast of its reader gives the same shape");
        if (Board) Map = kSrcBoard;
        if (RowOne) Map = kSrcRowOne;
        if (BoardOne) Map = kSrcBoardOne;
    }
    // an open group used only here: inline its program
    const Group* Open = V.group >= 0 ? &Pl.Groups[(size_t)V.group] : nullptr;
    const bool Domain = Open && !V.flatOfSpatial && Open->C == C &&
                        (VLine ? Open->lines == V.v.lines : !Open->lines && (Open->spatial == NG.spatial || (Board && !Open->spatial)));
    if (Domain && Pl.absorbable(Name)) {
        Group& Gr = Pl.Groups[(size_t)V.group];
        // inline it only if the rest of the node still fits behind it: every operand still to come takes at least
        // one source and one register (a constant, or a tensor read from memory), then the node's scalars and its
        // own instruction.  Otherwise the group is launched and read as one source, which cuts the chain here.
        const size_t Rest = Arity - 1 - K;
        if (NG.srcs.size() + Gr.srcs.size() + Rest + XSrcs <= (size_t)kMaxEltSrcs &&
            NG.code.size() + Gr.code.size() + 2 + XCode <= (size_t)kMaxEltCode &&
            NG.nregs + Gr.nregs + (int)Rest + 1 + XRegs <= kMaxEltRegs) {
            const int RB = NG.nregs, SB = (int)NG.srcs.size();
            for (EltSrc S : Gr.srcs) {
                if (Map != kSrcSame && (S.mode == kSrcSame || S.mode == kSrcLine)) S.mode = Map;
                else if (Map == kSrcBoard && S.mode == kSrcRowOne) S.mode = kSrcBoardOne; // [N,1] of a flat group, now per board
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
    EltSrc S;
    S.v = V.flatOfSpatial ? Pl.plain(Name, N.Name + " (flatten)") : Pl.ready(Name).v;
    // (a line view that is not its whole buffer, one half of an 18-line block, is read through its line fields)
    S.mode = Map != kSrcSame ? Map : VLine && (S.v.line0 != 0 || S.v.bufLines != S.v.lines) ? kSrcLine : kSrcSame;
    return load(S);
}

// The node's own instructions behind its operands; returns the register of the result.  Each op states its budget()
// right above what it emits: the sources, and the instructions (= registers), beyond the operands' loads and one
// instruction.  The budget is what operand() holds back when it inlines a group, so the two must agree.
int EltBuilder::expand(int ActCode, double PowE) {
    const std::string& Op = N.Op;
    int Out;
    if (ActCode != kActNone) {
        Out = instr(kEltAct, operand(0), ActCode);
    } else if (isBinary(Op) || Op == "Max" || Op == "Min") {
        const int A = operand(0), B = operand(1);
        Out = instr(Op == "Add" ? kEltAdd : Op == "Sub" ? kEltSub : Op == "Mul" ? kEltMul : Op == "Div" ? kEltDiv : Op == "Max" ? kEltMax : kEltMin, A, B);
    } else if (Op == "Clip") { // min(max(x, lo), hi), either bound optional
        const bool Lo = Pl.has(N, 1) || N.Attrs.count("min"), Hi = Pl.has(N, 2) || N.Attrs.count("max");
        budget(Lo + Hi, 2 * (Lo + Hi)); // per bound: a scalar, its load, the Max or Min
        Out = operand(0);
        if (Lo) Out = instr(kEltMax, Out, scalarReg(bound(1, "min", "Clip's lower bound")));
        if (Hi) Out = instr(kEltMin, Out, scalarReg(bound(2, "max", "Clip's upper bound")));
    } else if (Op == "HardSigmoid") { // min(max(alpha x + beta, 0), 1) at any alpha and beta
        budget(4, 8); // four scalars, each with its load and its instruction
        Out = operand(0);
        Out = instr(kEltMul, Out, scalarReg(N.attrF("alpha", 0.2)));
        Out = instr(kEltAdd, Out, scalarReg(N.attrF("beta", 0.5)));
        Out = instr(kEltMax, Out, scalarReg(0.0));
        Out = instr(kEltMin, Out, scalarReg(1.0));
    } else if (Op == "LeakyRelu") {
        budget(1, 2); // alpha: a scalar and its load, then kEltLeaky
        Out = operand(0);
        Out = instr(kEltLeaky, Out, scalarReg(N.attrF("alpha", 0.01)));
    } else if (Op == "PRelu") { // the slope: a scalar or per-channel constant, loaded like any constant operand
        budget(0, 1); // LeakyRelu's budget; the slope's source and load count as an operand to come
        const int A = operand(0), B = operand(1);
        Out = instr(kEltLeaky, A, B);
    } else if (Op == "Abs" || Op == "Neg") {
        Out = instr(Op == "Abs" ? kEltAbs : kEltNeg, operand(0), 0);
    } else if (Op == "Pow") {
        // Pow(x, c) at a constant scalar c: 2, 3, 4 as products, -0.5 and -2 as a reciprocal behind the square root or
        // the square (0.5 and -1 are activations, 1 never gets here), anything else powf with c as a scalar source
        const bool TwoStep = PowE == 3.0 || PowE == 4.0 || PowE == -0.5 || PowE == -2.0;
        if (TwoStep) budget(0, 1);            // one instruction more
        else if (PowE != 2.0) budget(1, 1);   // the exponent: a scalar and its load
        const int A = operand(0);
        if (PowE == 2.0) Out = instr(kEltMul, A, A);
        else if (PowE == 3.0) Out = instr(kEltMul, instr(kEltMul, A, A), A);
        else if (PowE == 4.0) { const int Sq = instr(kEltMul, A, A); Out = instr(kEltMul, Sq, Sq); }
        else if (PowE == -0.5) Out = instr(kEltAct, instr(kEltAct, A, kActSqrt), kActRecip);
        else if (PowE == -2.0) Out = instr(kEltAct, instr(kEltMul, A, A), kActRecip);
        else Out = instr(kEltPow, A, scalarReg(PowE));
    } else { // BatchNormalization on a runtime tensor: y = x * s + t per channel
        budget(2, 3); // s and t: two sources and their loads, then Mul and Add
        if (N.In.size() < 5) fail("expected scale, bias, mean and variance");
        for (size_t S = 1; S < 5; ++S)
            if (Pl.host(N, S, "a BatchNormalization statistic").count() != (size_t)C) fail("statistic length does not match the channels");
        std::vector<float> Sc((size_t)C), Sh((size_t)C);
        for (int Ch = 0; Ch < C; ++Ch) {
            const Planner::BnChannel B = Pl.bnChannel(N, (size_t)Ch);
            Sc[(size_t)Ch] = (float)B.scale;
            Sh[(size_t)Ch] = (float)(B.beta - B.mean * B.scale);
        }
        const int A = operand(0);
        const size_t SOff = Pl.addConst(Sc), TOff = Pl.addConst(Sh);
        if (NG.srcs.size() + 2 > (size_t)kMaxEltSrcs) fail("too many inputs for one fused launch");
        EltSrc S1, S2;
        S1.mode = S2.mode = kSrcChannel;
        S1.constOff = SOff;
        S2.constOff = TOff;
        const int RS = load(S1), RT = load(S2);
        Out = instr(kEltAdd, instr(kEltMul, A, RS), RT);
    }
    return Out;
}

// ---- elementwise ops: fused into groups ------------------------------------------------------------------------
void Planner::elementwise(const Node& N) {
    EltBuilder B(*this, N);
    const std::string& Op = N.Op;
    const bool MinMax = Op == "Max" || Op == "Min";
    if (MinMax && N.In.size() != 2) fail(N, Op + " of " + std::to_string(N.In.size()) + " operands: two only");
    const int ActCode = nodeAct(N);
    B.Arity = isBinary(Op) || MinMax || Op == "PRelu" ? 2 : 1;
    if (Op == "PRelu") host(N, 1, "the slope");
    double PowE = 0;
    if (Op == "Pow") {
        const Val& E = get(N, 1);
        if (E.runtime || E.count() != 1 || (E.isInt && E.i[0] == kBatch)) fail(N, "the exponent must be a constant scalar");
        PowE = E.at(0);
    }
    std::vector<int64_t>& D = B.D;
    for (size_t K = 0; K < B.Arity; ++K) {
        const Val& V = get(N, K);
        std::vector<int64_t> Di = V.runtime && V.flatOfSpatial ? std::vector<int64_t>{kBatch, (int64_t)V.v.C * 81} : V.dims;
        // a PRelu slope [C] on [N,C,9,9] is read per channel, like [C,1,1]
        if (Op == "PRelu" && K == 1 && Di.size() == 1 && D.size() == 4 && Di[0] == D[1] && Di[0] != D[3]) Di = {Di[0], 1, 1};
        std::vector<int64_t> Bd;
        if (K == 0) D = Di;
        else if (!broadcast(D, Di, &Bd)) fail(N, "shapes " + dimsStr(D) + " and " + dimsStr(Di) + " do not broadcast");
        else D = Bd;
        B.InDims.push_back(Di);
    }
    for (size_t K = 0; K < B.Arity; ++K) B.Tok = B.Tok || (get(N, K).runtime && get(N, K).form == kFormToken); // a token operand makes the result a token tensor
    if (B.Tok && !isTokenDims(D)) fail(N, "a token tensor broadcast to " + dimsStr(D));
    B.Spatial = isSpatialDims(D);
    // line operands: the result is a line tensor of the same lines, or (broadcast back) a spatial tensor
    const Val* Rank = nullptr;
    const Val* File = nullptr;
    bool AnyLine = false;
    for (size_t K = 0; K < B.Arity; ++K) {
        const Val& V = get(N, K);
        if (!V.runtime || V.form != kFormLine) continue;
        AnyLine = true;
        (V.dims[2] == 1 ? File : Rank) = &V;
    }
    if (Rank && File)
        fail(N, "rank lines " + dimsStr(Rank->dims) + " and file lines " + dimsStr(File->dims) + " in one " + Op +
                    ": the two orientations meet only through Transpose [0,1,3,2] or on the board, each broadcast onto [N,C,9,9]");
    if (AnyLine && !B.Spatial) {
        B.Lines = lineCount(D);
        if (!B.Lines) fail(N, "a line tensor broadcast to " + dimsStr(D));
    }
    const int C = B.C = B.Tok ? (int)D[2] : B.Spatial || B.Lines ? (int)D[1] : flatC(D);
    if (C < 0) fail(N, "output shape " + dimsStr(D) + " is neither [N,C,9,9], a token tensor nor flat");
    B.ChanAxis = B.Tok ? 2 : 1;
    Group& NG = B.NG;
    NG.spatial = B.Spatial || B.Tok;
    NG.lines = B.Lines;
    NG.C = C;
    NG.name = N.Name;
    NG.out = N.Out[0];
    NG.outReg = B.expand(ActCode, PowE);
    if (NG.nregs > kMaxEltRegs || NG.code.size() > (size_t)kMaxEltCode) fail(N, "elementwise chain too long for one launch");
    Groups.push_back(NG);
    Val V;
    if (B.Lines) {
        V.runtime = true;
        V.dims = D;
        V.producer = N.Name;
        V.form = kFormLine;
        V.v.lines = V.v.bufLines = B.Lines;
    } else {
        V = runtimeVal(N, D, B.Tok ? kFormToken : kFormPlain);
    }
    V.group = (int)Groups.size() - 1;
    V.v.buf = kPending;
    V.v.C = C;
    V.v.spatial = NG.spatial;
    V.v.stride = roundUp(std::max(C, 1), kChunk);
    Vals[N.Out[0]] = V;
}

// x ** 1 is x: an open elementwise group read only here stays open under the new name
void Planner::powOne(const Node& N) {
    const Val& X = get(N, 0);
    const bool MoveGroup = X.group >= 0 && absorbable(N.In[0]);
    Val V = MoveGroup ? X : ready(N.In[0]);
    V.producer = N.Name;
    if (MoveGroup) Groups[(size_t)V.group].out = N.Out[0];
    Vals[N.Out[0]] = V;
}

} // namespace nsg::graph
