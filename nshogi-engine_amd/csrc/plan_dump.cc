// plan_dump.cc -- prints every field of the GraphPlan the planner returns for each model, as text: the planner's
// output pinned on the CPU (tests/test_plan_snapshot.py compares it with tests/golden/graph_plans.txt).
//   plan_dump [--lifetimes] [--planes N] MODEL.onnx ... [--planes M] MODEL.onnx ...     (N: the input planes, 86 until given)
// --lifetimes: after each plan, the virtual buffers the views had before assignBuffers renamed them (LifetimeTrace), for
// tests/plan_check.py.  Without the flag the output is what it was before the flag existed.
// Uses the public onnx_graph.h, and plan_lifetimes.h for --lifetimes.  The line format is older than the per-kind
// argument records: `Columns` below projects a record onto it, for this tool only.
// Floats print as %a and doubles as %.17g, so every bit shows; no path beyond the
// model's base name and no timing appears: two runs print the same bytes.
#include "onnx_graph.h"
#include "plan_lifetimes.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

using namespace nsg::graph;

namespace {

uint64_t hashFloats(const std::vector<float>& W, size_t Begin, size_t End) { // FNV-1a over the bytes
    uint64_t H = 1469598103934665603ull;
    const unsigned char* P = (const unsigned char*)W.data();
    for (size_t K = Begin * 4; K < End * 4; ++K) H = (H ^ P[K]) * 1099511628211ull;
    return H;
}

void view(const char* Name, const View& V) {
    std::printf(" %s=%d/%d/%d/%d/%c", Name, V.buf, V.stride, V.offset, V.C, V.spatial ? 's' : 'f');
    if (V.lines) std::printf("/L%d@%d/%d", V.lines, V.line0, V.bufLines); // a line view: lines @ first line / lines of the buffer
}

// The snapshot's line format prints these columns for every launch, whatever its kind: a launch whose record has no
// such field prints the default below.  A projection for this tool only: columns(C, record) fills it.
struct Columns {
    View in, res, attK, attV;
    bool dense = false, depthwise = false;
    int taps = 9, kh = 3, kw = 3, dh = 1, dw = 1, cinPad = 0, coutTiles = 0;
    size_t wOff = 0, biasOff = 0;
    int act = kActNone, eltOut = 0, poolMode = kPoolMax;
    float eps = 0.f;
    int groups = 1, heads = 0, headDim = 0;
    float scale = 1.f;
    bool hasBias = false;
};
void columns(Columns& C, const ConvArgs& A) {
    C.in = A.in; C.res = A.res; C.dense = A.dense; C.depthwise = A.depthwise; C.taps = A.taps;
    C.kh = A.kh; C.kw = A.kw; C.dh = A.dh; C.dw = A.dw; C.cinPad = A.cinPad; C.coutTiles = A.coutTiles;
    C.wOff = A.wOff; C.biasOff = A.biasOff; C.act = A.act; C.groups = A.groups;
}
void columns(Columns& C, const EltProgram& A) { C.eltOut = A.eltOut; }
void columns(Columns&, const ConcatSegs&) {}
void columns(Columns& C, const PoolArgs& A) { C.in = A.in; C.kh = A.kh; C.kw = A.kw; C.dh = A.dh; C.dw = A.dw; C.poolMode = A.poolMode; }
void columns(Columns& C, const LinePoolArgs& A) { C.in = A.in; C.poolMode = A.poolMode; }
void columns(Columns& C, const LayerNormArgs& A) { C.in = A.in; C.wOff = A.wOff; C.biasOff = A.biasOff; C.eps = A.eps; }
void columns(Columns& C, const GroupNormArgs& A) {
    C.in = A.in; C.wOff = A.wOff; C.biasOff = A.biasOff; C.eps = A.eps; C.groups = A.groups; C.act = A.act;
}
void columns(Columns& C, const RmsNormArgs& A) { C.in = A.in; C.wOff = A.wOff; C.eps = A.eps; }
void columns(Columns& C, const AttentionArgs& A) {
    C.in = A.in; C.attK = A.attK; C.attV = A.attV; C.heads = A.heads; C.headDim = A.headDim; C.scale = A.scale;
    C.hasBias = A.hasBias; C.biasOff = A.biasOff;
}
// (the snapshot prints the `res` column of a run-time product, a token mix and a gather as "no residual")
void columns(Columns& C, const BmmArgs& A) { C.in = A.in; C.res = noResidual(); C.scale = A.scale; C.act = A.act; }
void columns(Columns& C, const TokenMixArgs& A) { C.in = A.in; C.res = noResidual(); C.wOff = A.wOff; C.act = A.act; }
void columns(Columns& C, const GatherArgs& A) { C.in = A.in; C.res = noResidual(); }
void columns(Columns& C, const ChanReduceArgs& A) { C.in = A.in; C.scale = A.scale; }
void columns(Columns& C, const NormalizeArgs& A) { C.in = A.in; C.eps = A.eps; }
template <class T> void columns(Columns& C, const T& A) { C.in = A.in; } // the records that hold `in` alone

// the fields behind the columns, per record, where they are not the defaults
void tail(const Launch&, const ConvArgs& A) { // a dense launch over head rows or lines; a grouped conv (groups is a column)
    if (A.rowsPerBoard != 1) std::printf(" rowsPerBoard=%d", A.rowsPerBoard);
    if (A.groups > 1) std::printf(" gTabOff=%zu", A.gTabOff);
}
void tail(const Launch&, const AttentionArgs& A) { // a run-time attention bias
    if (!A.hasRtBias) return;
    view("rtBias", A.rtBias);
    std::printf(" rtHeadStride=%d rtScale=%a", A.rtHeadStride, (double)A.rtScale);
}
void tail(const Launch&, const LinePoolArgs& A) { std::printf(" lineFiles=%d", A.lineFiles); }
void tail(const Launch&, const BmmArgs& A) { // A is `in`; scale and act are columns
    view("bmmB", A.bmmB);
    std::printf(" bmmNN=%d bmmK=%d", A.bmmNN, A.bmmK);
}
void tail(const Launch&, const TokenMixArgs& A) { // the first stage's act is a column, the record's hash is among the consts
    std::printf(" mixD=%d mixStages=%d mixAct2=%d", A.mixD, A.mixStages, A.mixAct2);
}
void tail(const Launch& L, const GatherArgs& A) { // the width is out's stride; the two tables' hash is among the consts
    std::printf(" gatherRows=%d gatherBlock=%ld gatherWidth=%d gatherTabOff=%zu", A.gatherRows, A.gatherBlock, L.out.stride, A.gatherTabOff);
}
void tail(const Launch&, const ChanReduceArgs& A) { std::printf(" redMode=%d", A.redMode); } // the mean's factor is the column `scale`
void tail(const Launch&, const NormalizeArgs& A) { std::printf(" normP=%d", A.p); } // eps is a column
template <class T> void tail(const Launch&, const T&) {}

// the offsets into `weights` a record reads its constants at
std::vector<size_t> consts(const ConvArgs& A) {
    std::vector<size_t> R{A.wOff, A.biasOff};
    if (A.groups > 1) R.push_back(A.gTabOff);
    return R;
}
std::vector<size_t> consts(const EltProgram& A) {
    std::vector<size_t> R;
    for (const EltSrc& S : A.srcs)
        if (S.mode == kSrcChannel || S.mode == kSrcSquareChannel || S.mode == kSrcSquare) R.push_back(S.constOff);
    return R;
}
std::vector<size_t> consts(const LayerNormArgs& A) { return {A.wOff, A.biasOff}; }
std::vector<size_t> consts(const GroupNormArgs& A) { return {A.wOff, A.biasOff}; }
std::vector<size_t> consts(const RmsNormArgs& A) { return {A.wOff}; }
std::vector<size_t> consts(const TokenMixArgs& A) { return {A.wOff}; }
std::vector<size_t> consts(const AttentionArgs& A) { return A.hasBias ? std::vector<size_t>{A.biasOff} : std::vector<size_t>{}; }
std::vector<size_t> consts(const GatherArgs& A) { return {A.gatherTabOff}; }
template <class T> std::vector<size_t> consts(const T&) { return {}; }
std::vector<size_t> constsOf(const Launch& L) {
    return std::visit([](const auto& A) { return consts(A); }, L.args);
}

void dump(const GraphPlan& P) {
    std::printf("numChannels=%d planeStride=%d nodes=%d convLaunches=%d attentionLaunches=%d params=%" PRIu64
                " flopsPerPosition=%.17g activationBytesPerPosition=%zu\n",
                P.numChannels, P.planeStride, P.nodes, P.convLaunches, P.attentionLaunches, P.params, P.flopsPerPosition,
                P.activationBytesPerPosition);
    std::printf("weights=%zu hash=%016" PRIx64 "\n", P.weights.size(), hashFloats(P.weights, 0, P.weights.size()));
    std::printf("bufSpatialStride");
    for (int S : P.bufSpatialStride) std::printf(" %d", S);
    std::printf("\nbufFlatStride");
    for (int S : P.bufFlatStride) std::printf(" %d", S);
    std::printf("\nlaunches=%zu\n", P.launches.size());
    // a constant record runs from its offset to the next offset any launch names
    std::vector<size_t> Starts;
    for (const Launch& L : P.launches)
        for (size_t O : constsOf(L)) Starts.push_back(O);
    Starts.push_back(P.weights.size());
    std::sort(Starts.begin(), Starts.end());
    for (size_t I = 0; I < P.launches.size(); ++I) {
        const Launch& L = P.launches[I];
        std::printf("#%zu kind=%d name=%s", I, L.kind(), L.name.c_str());
        Columns C;
        std::visit([&](const auto& A) { columns(C, A); }, L.args);
        view("out", L.out);
        view("in", C.in);
        view("res", C.res);
        std::printf(" dense=%d depthwise=%d taps=%d k=%dx%d d=%dx%d cinPad=%d coutTiles=%d wOff=%zu biasOff=%zu act=%d eltOut=%d"
                    " poolMode=%d eps=%a groups=%d",
                    C.dense, C.depthwise, C.taps, C.kh, C.kw, C.dh, C.dw, C.cinPad, C.coutTiles, C.wOff, C.biasOff, C.act,
                    C.eltOut, C.poolMode, (double)C.eps, C.groups);
        view("attK", C.attK);
        view("attV", C.attV);
        std::printf(" heads=%d headDim=%d scale=%a hasBias=%d", C.heads, C.headDim, (double)C.scale, C.hasBias);
        std::visit([&](const auto& A) { tail(L, A); }, L.args);
        // every line ends with a program and a segment list: empty ones for the kinds that have none
        static const EltProgram NoElt;
        static const ConcatSegs NoSegs;
        const EltProgram& Elt = L.is<EltProgram>() ? std::get<EltProgram>(L.args) : NoElt;
        std::printf(" srcs=%zu", Elt.srcs.size());
        for (const EltSrc& S : Elt.srcs) {
            std::printf(" [mode=%d", S.mode);
            view("v", S.v);
            std::printf(" constOff=%zu scalar=%a]", S.constOff, (double)S.scalar);
        }
        std::printf(" code=%zu", Elt.code.size());
        for (const EltInstr& In : Elt.code) std::printf(" %d:%d,%d,%d", In.op, In.dst, In.a, In.b);
        const std::vector<CopySeg>& Segs = (L.is<ConcatSegs>() ? std::get<ConcatSegs>(L.args) : NoSegs).segs;
        std::printf(" segs=%zu", Segs.size());
        for (const CopySeg& S : Segs) {
            std::printf(" [dstOff=%d", S.dstOff);
            view("v", S.v);
            std::printf("]");
        }
        std::printf(" consts=");
        for (size_t O : constsOf(L)) {
            const size_t End = *std::upper_bound(Starts.begin(), Starts.end(), O);
            std::printf("%zu+%zu:%016" PRIx64 ",", O, End - O, hashFloats(P.weights, O, End));
        }
        std::printf("\n");
    }
    std::printf("outputs");
    view("policy", P.policy);
    view("value", P.value);
    view("draw", P.draw);
    std::printf("\n");
}

// "V<id> stride spatial alsoFlat phys" per virtual buffer, then per launch every view of forEachNamedView as
// field:virtual followed by the renamed view.  The format has the six fields below in every launch's row: a field the
// launch's record does not have is printed as the default view, which names no buffer (tests/plan_check.py skips it).
void dumpLifetimes(const GraphPlan& P, const LifetimeTrace& T) {
    std::printf("lifetimes virtuals=%zu\n", T.virtStride.size());
    for (size_t V = 0; V < T.virtStride.size(); ++V)
        std::printf("V%zu stride=%d spatial=%d alsoFlat=%d phys=%d\n", V, T.virtStride[V], (int)T.virtSpatial[V], T.virtAlsoFlat[V], T.virtPhys[V]);
    auto one = [](const ViewTrace& R) {
        std::printf(" %s:%d", R.field.c_str(), R.virt);
        view("v", R.v);
    };
    for (size_t I = 0; I < T.launches.size(); ++I) {
        std::printf("L%zu", I);
        const std::vector<ViewTrace>& Row = T.launches[I];
        Columns C;
        std::visit([&](const auto& A) { columns(C, A); }, P.launches[I].args);
        size_t Next = 0; // (a record names its views in the order of this list)
        for (const char* Field : {"in", "res", "attK", "attV", "rtBias", "bmmB"}) {
            if (Next < Row.size() && Row[Next].field == Field) {
                one(Row[Next++]);
                continue;
            }
            ViewTrace None;
            None.field = Field;
            None.virt = None.v.buf = std::strcmp(Field, "res") ? -1 : C.res.buf;
            one(None);
        }
        for (; Next < Row.size(); ++Next) one(Row[Next]);
        std::printf("\n");
    }
    std::printf("LO");
    for (const ViewTrace& R : T.outputs) one(R);
    std::printf("\n");
}

} // namespace

int main(int Argc, char** Argv) {
    int Planes = 86;
    bool Lifetimes = false;
    for (int A = 1; A < Argc; ++A) {
        if (!std::strcmp(Argv[A], "--lifetimes")) {
            Lifetimes = true;
            continue;
        }
        if (!std::strcmp(Argv[A], "--planes") && A + 1 < Argc) {
            Planes = std::atoi(Argv[++A]);
            continue;
        }
        const char* Slash = std::strrchr(Argv[A], '/');
        std::printf("== %s planes=%d\n", Slash ? Slash + 1 : Argv[A], Planes);
        std::ifstream F(Argv[A], std::ios::binary);
        if (!F) {
            std::printf("ERROR cannot read the file\n");
            continue;
        }
        const std::string Data((std::istreambuf_iterator<char>(F)), std::istreambuf_iterator<char>());
        GraphPlan P;
        std::string Err;
        LifetimeTrace T;
        if (buildPlanTraced(Data.data(), Data.size(), Planes, &P, Lifetimes ? &T : nullptr, &Err)) {
            dump(P);
            if (Lifetimes) dumpLifetimes(P, T);
        } else std::printf("ERROR %s\n", Err.c_str());
    }
    return 0;
}
