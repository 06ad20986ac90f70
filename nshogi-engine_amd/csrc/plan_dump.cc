// plan_dump.cc -- prints every field of the GraphPlan the planner returns for each model, as text: the planner's
// output pinned on the CPU (tests/test_plan_snapshot.py compares it with tests/golden/graph_plans.txt).
//   plan_dump [--lifetimes] [--planes N] MODEL.onnx ... [--planes M] MODEL.onnx ...     (N: the input planes, 86 until given)
// --lifetimes: after each plan, the virtual buffers the views had before assignBuffers renamed them (LifetimeTrace), for
// tests/plan_check.py.  Without the flag the output is what it was before the flag existed.
// Uses the public onnx_graph.h, and plan_lifetimes.h for --lifetimes.
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

// the offsets into `weights` a launch reads its constants at
std::vector<size_t> constsOf(const Launch& L) {
    std::vector<size_t> R;
    const int K = L.kind;
    if (K == kLaunchConv || K == kLaunchLayerNorm || K == kLaunchGroupNorm) R = {L.wOff, L.biasOff};
    if (K == kLaunchRmsNorm || K == kLaunchTokenMix) R = {L.wOff};
    if (K == kLaunchConv && L.groups > 1) R.push_back(L.gTabOff);
    if (K == kLaunchAttention && L.hasBias) R = {L.biasOff};
    if (K == kLaunchGather) R = {L.gatherTabOff};
    for (const EltSrc& S : L.srcs)
        if (S.mode == kSrcChannel || S.mode == kSrcSquareChannel || S.mode == kSrcSquare) R.push_back(S.constOff);
    return R;
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
        std::printf("#%zu kind=%d name=%s", I, L.kind, L.name.c_str());
        view("out", L.out);
        view("in", L.in);
        view("res", L.res);
        std::printf(" dense=%d depthwise=%d taps=%d k=%dx%d d=%dx%d cinPad=%d coutTiles=%d wOff=%zu biasOff=%zu act=%d eltOut=%d"
                    " poolMode=%d eps=%a groups=%d",
                    L.dense, L.depthwise, L.taps, L.kh, L.kw, L.dh, L.dw, L.cinPad, L.coutTiles, L.wOff, L.biasOff, L.act,
                    L.eltOut, L.poolMode, (double)L.eps, L.groups);
        view("attK", L.attK);
        view("attV", L.attV);
        std::printf(" heads=%d headDim=%d scale=%a hasBias=%d", L.heads, L.headDim, (double)L.scale, L.hasBias);
        // the fields of a run-time attention bias and of a dense launch over head rows, where they are not the defaults
        if (L.hasRtBias) {
            view("rtBias", L.rtBias);
            std::printf(" rtHeadStride=%d rtScale=%a", L.rtHeadStride, (double)L.rtScale);
        }
        if (L.rowsPerBoard != 1) std::printf(" rowsPerBoard=%d", L.rowsPerBoard);
        if (L.kind == kLaunchLinePool) std::printf(" lineFiles=%d", L.lineFiles);
        if (L.kind == kLaunchConv && L.groups > 1) std::printf(" gTabOff=%zu", L.gTabOff); // a grouped conv: groups is printed above
        if (L.kind == kLaunchBmm) { // A is `in`; scale and act are printed above
            view("bmmB", L.bmmB);
            std::printf(" bmmNN=%d bmmK=%d", L.bmmNN, L.bmmK);
        }
        if (L.kind == kLaunchTokenMix) // the input is `in`, the first stage's act is printed above, the record's hash below
            std::printf(" mixD=%d mixStages=%d mixAct2=%d", L.mixD, L.mixStages, L.mixAct2);
        if (L.kind == kLaunchGather) // the source is `in`; the width is out's stride; the two tables' hash is below
            std::printf(" gatherRows=%d gatherBlock=%ld gatherWidth=%d gatherTabOff=%zu", L.gatherRows, L.gatherBlock, L.out.stride, L.gatherTabOff);
        if (L.kind == kLaunchChanReduce) std::printf(" redMode=%d", L.redMode); // the input is `in`; the mean's factor is `scale`, above
        std::printf(" srcs=%zu", L.srcs.size());
        for (const EltSrc& S : L.srcs) {
            std::printf(" [mode=%d", S.mode);
            view("v", S.v);
            std::printf(" constOff=%zu scalar=%a]", S.constOff, (double)S.scalar);
        }
        std::printf(" code=%zu", L.code.size());
        for (const EltInstr& C : L.code) std::printf(" %d:%d,%d,%d", C.op, C.dst, C.a, C.b);
        std::printf(" segs=%zu", L.segs.size());
        for (const CopySeg& S : L.segs) {
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

// "V<id> stride spatial alsoFlat phys" per virtual buffer, then per launch every view of forEachView as
// field:virtual followed by the renamed view
void dumpLifetimes(const LifetimeTrace& T) {
    std::printf("lifetimes virtuals=%zu\n", T.virtStride.size());
    for (size_t V = 0; V < T.virtStride.size(); ++V)
        std::printf("V%zu stride=%d spatial=%d alsoFlat=%d phys=%d\n", V, T.virtStride[V], (int)T.virtSpatial[V], T.virtAlsoFlat[V], T.virtPhys[V]);
    auto row = [](const std::vector<ViewTrace>& Row) {
        for (const ViewTrace& R : Row) {
            std::printf(" %s:%d", R.field.c_str(), R.virt);
            view("v", R.v);
        }
        std::printf("\n");
    };
    for (size_t I = 0; I < T.launches.size(); ++I) {
        std::printf("L%zu", I);
        row(T.launches[I]);
    }
    std::printf("LO");
    row(T.outputs);
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
            if (Lifetimes) dumpLifetimes(T);
        } else std::printf("ERROR %s\n", Err.c_str());
    }
    return 0;
}
