// onnx_graph.h -- the general graph path's host half: reads an ONNX model built from the closed op set of
// DESIGN.md section 13, folds shape chains and BatchNorm, fuses epilogues and elementwise chains, assigns
// activation buffers, and returns an immutable GraphPlan of launches: each a name, an output view and the argument
// record of its kind (ConvArgs, EltProgram, ... below), which also names the device views the launch reads.
// graph_exec.hip runs a launch on the device, one function per record.  Host-only C++: no device code.
//
// Layout of every runtime tensor (the library's board-major, channel-innermost layout):
//   spatial [N,C,9,9]           -> [row = board * 81 + square][stride] floats
//   token [N,81,C]              -> the same rows under another logical shape: a transformer's token tensor over the
//                                  81 squares is the spatial layout, so flatten(2).transpose(1,2) costs no launch
//   flat [N,C] / [N,C,1,1] / [N] -> [row = board][stride] floats
//   head rows [N,H,K]           -> [row = board * H + head][stride] floats, a view of a flat [N,H*K] (K a multiple of 16)
//   lines [N,C,9,1] / [N,C,1,9] / [N,C,18,1] -> [row = board * L + line][stride] floats, L = 9 or 18 lines per board: one
//                                  value per rank (or per file) and channel, in a flat buffer of stride L * stride
// stride = C rounded up to 16 (the conv kernel's K chunk); channels C..stride-1 are written as zero by every kernel.
// A view names a buffer plus a channel offset, so `Slice` and `Split` along the channel axis cost no launch; a view of a
// line tensor names a first line as well, so the two halves of an 18-line block are views too.
// A one-channel tensor ([N,1,9,9], [N,81,1], [N,1]) is an ordinary C = 1 tensor: a row of stride 16 with channel 0 live.
// A reduction over the channels of a row (kLaunchChanReduce) writes one, and the elementwise program broadcasts one over
// the channels of a C-channel output by reading channel 0 of its row (kSrcRowOne, kSrcBoardOne).
#ifndef NSG_ONNX_GRAPH_H
#define NSG_ONNX_GRAPH_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <variant>
#include <vector>

namespace nsg {
namespace graph {

constexpr int kChunk = 16;      // channel granule of every activation stride and of the conv kernel's K chunk
constexpr int kCoutTile = 64;   // output channels per conv workgroup
constexpr int kMaxConvHalo = 4; // squares a conv tap may reach past the board's edge (the LDS image is at most 17 x 17)
constexpr int kMaxEltSrcs = 8;  // inputs of one fused elementwise launch
constexpr int kMaxEltCode = 32; // instructions of one fused elementwise launch
constexpr int kMaxEltRegs = 16;
constexpr int kMaxCopySegs = 8; // sources of one channel concat
constexpr int kGroupTabInts = 12; // ints per 64-output tile in a grouped conv's table (ConvArgs::gTabOff)
constexpr int kMaxMixHidden = 336; // hidden units of a token-mixing MLP: 21 fragments of 16 (an expansion of 4 x 81 = 324 fits)

// kActGelu: exact (erf); kActRelu6 = min(max(x, 0), 6); kActHardSigmoid = min(max(x / 6 + 0.5, 0), 1); kActHardSwish =
// x * that.  All of them are parameter-free: a LeakyRelu, a PRelu, other Clip bounds are elementwise instructions.
// kActRecip = 1 / x; kActMish = x tanh(softplus(x)); kActGeluTanh = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)));
// kActSoftsign = x / (1 + |x|).
enum Act {
    kActNone = 0, kActRelu, kActSigmoid, kActTanh, kActSwish, kActSoftplus, kActErf, kActGelu,
    kActRelu6, kActHardSwish, kActHardSigmoid,
    kActExp, kActLog, kActSqrt, kActRecip, kActMish, kActGeluTanh, kActSoftsign
};

// A runtime tensor as a launch sees it.  buf: -1 = the plane buffer (graph input), >= 0 = activation buffer.
struct View {
    int buf = -1;
    int stride = 0;  // floats per row
    int offset = 0;  // first channel inside the row
    int C = 0;       // channels (a flat tensor: its width)
    bool spatial = false;
    // a line tensor (lines > 0): `lines` rows per board starting at row `line0` of the `bufLines` rows the buffer holds
    // per board; row (board, l) of the view is row board * bufLines + line0 + l of the buffer
    int lines = 0, bufLines = 0, line0 = 0;
};
constexpr int kNoRes = -2; // View::buf of a conv's `res` that has no residual
inline View noResidual() {
    View V;
    V.buf = kNoRes;
    return V;
}

// Elementwise program: registers r0..r15; opcodes below.  LOAD reads source `a` into register `dst`.
// kEltLeaky: dst = a > 0 ? a : a * b (LeakyRelu: b holds alpha; PRelu: b holds the channel's slope); kEltNeg, kEltAbs: of a.
// kEltPow: dst = powf(a, b), b loaded from a scalar source: a Pow whose exponent has no exact form.
enum EltOp {
    kEltLoad = 0, kEltAct, kEltAdd, kEltSub, kEltMul, kEltDiv, kEltMax, kEltMin, kEltLeaky, kEltNeg, kEltAbs, kEltPow
};
struct EltInstr {
    uint8_t op, dst, a, b; // kEltAct: a = source register, b = Act; binary: dst = a (op) b; unary: b unused
};
// How a source is read, relative to the element (row, c) of the output
enum EltMode {
    kSrcSame = 0,   // the view's (row, c): same kind as the output
    kSrcBoard,      // flat view broadcast over squares: (row / 81, c)
    kSrcChannel,    // constant per channel: weights[constOff + c]
    kSrcScalar,     // constant: `scalar`
    kSrcSquareChannel, // constant per (square, channel), a learned positional embedding: weights[constOff + (row % 81) * C + c]
    // line views (View::lines > 0), row = board * bufLines + line0 + l
    kSrcRankLine,   // broadcast over the files of a spatial output: l = (row % 81) / 9
    kSrcFileLine,   // broadcast over the ranks of a spatial output: l = (row % 81) % 9
    kSrcLine,       // a line output reading a line view of as many lines: l = row % lines (kSrcSame when the view is its whole buffer)
    // one-channel sources broadcast over the channels of the output
    kSrcRowOne,     // a view with C == 1 of the output's kind (spatial or token rows, or flat against flat): p[row * stride + offset]
    kSrcBoardOne,   // a flat view with C == 1 ([N,1], [N,1,1,1]) against a spatial output: p[(row / 81) * stride + offset]
    kSrcSquare,     // constant per square ([1,1,9,9] on a spatial tensor, [1,81,1] on tokens), 81 floats: weights[constOff + row % 81]
};
struct EltSrc {
    int mode = kSrcScalar;
    View v;
    size_t constOff = 0;
    float scalar = 0.f;
};

// The numeric values are printed by plan_dump (kind=%d): they do not change.
enum LaunchKind {
    kLaunchConv = 0, kLaunchElt, kLaunchMean, kLaunchConcat, kLaunchFlatten, kLaunchLayerNorm, kLaunchAttention,
    kLaunchPool, kLaunchMax, kLaunchGroupNorm, kLaunchRmsNorm, kLaunchBmm, kLaunchLinePool, kLaunchTokenMix, kLaunchGather,
    kLaunchChanReduce, kLaunchNormalize
};
// PoolArgs: the max, or the mean over kh x kw taps with the zero halo counted (count_include_pad = 1) or left out
enum PoolMode { kPoolMax = 0, kPoolAvgInclude, kPoolAvgExclude };
// ChanReduceArgs: what is taken over the channels of a row.  kRedL1 = sum |x|, kRedSumSq = sum x^2, kRedL2 = its square
// root, kRedLogSumExp = log sum exp(x) through the row's max.  plan_dump prints the values (redMode=%d): they do not change.
enum RedMode { kRedMax = 0, kRedMin, kRedSum, kRedL1, kRedSumSq, kRedL2, kRedLogSumExp };
constexpr int kMaxHeadDim = 64; // channels per attention head (a multiple of 4)
struct CopySeg { View v; int dstOff = 0; };

// ---- The argument records: one per launch kind (or family of kinds), holding that kind's fields only.  A Launch is a
// name, the output view and one record; its kind is read off the record (kind()), so a kind and another kind's fields
// cannot meet.  views(F) calls F(name, View&) for every device view the record reads: the one place a view field is
// named for the lifetime pass and the buffer renaming (forEachNamedView, planner.h).  `out` is the Launch's own.

// kLaunchConv: an implicit-GEMM conv (taps = kh x kw, row-major over (ky, kx)), a dense layer (taps 1, rows =
// boards) or a depthwise conv.  A tap reads the square (ky - (kh-1)/2) * dh rows and (kx - (kw-1)/2) * dw columns
// away; the halo dh * (kh-1)/2 by dw * (kw-1)/2 is at most kMaxConvHalo each way.  Which kernel runs it: kernel().
struct ConvArgs {
    View in, res = noResidual();
    bool dense = false;
    bool depthwise = false; // group = Cin = Cout: per-channel taps, no sum over channels
    int taps = 9;
    int kh = 3, kw = 3, dh = 1, dw = 1;
    int cinPad = 0;  // K = taps x cinPad
    int coutTiles = 0;  // depthwise: unused (0)
    size_t wOff = 0;    // packed weights [coutTiles][cinPad / 16][taps][16][64]; depthwise: [cinPad / 16][taps][16]
    size_t biasOff = 0; // [coutTiles * 64]; depthwise: [cinPad]
    // A grouped conv (1 < group < Cin, Cin / group a multiple of 4) has `groups` > 1.  Its packed weights are [tile]
    // [chunk of the tile's range][tap][16][64]: a tile of 64 outputs holds only the 16-channel input chunks that the
    // groups of its outputs read, with exact zeros where input and output channel lie in different groups.  gTabOff:
    // kGroupTabInts ints per tile, stored bit for bit in the float blob: first chunk, chunk count, the tile's weight
    // offset in floats from wOff, 0, then (first chunk, chunk count) of each of the four waves' 16 outputs (a sub-range
    // of the tile's; count 0: no output).
    int groups = 1;
    size_t gTabOff = 0;
    int act = kActNone;
    // dense: the rows of a board.  1: flat [N,K]; H: head rows [N,H,K], rows of (board, head) at stride in.stride, H of
    // them contiguous per board (the virtual buffer is flat with stride H * in.stride); L: a line tensor's (board, line)
    // rows, a 1x1 conv over them.
    int rowsPerBoard = 1;

    // The kernel of graph_kernels.h that runs the conv: depthwise on graphDepthwise, a grouped conv of any geometry on
    // graphConvGrouped, 1x1 and 3x3 at dilation 1 (and every dense layer) on graphConv<1> / graphConv<9>, every other
    // dense geometry on graphConvGeo.
    enum Kernel { kDepthwise, kGrouped, kTile, kGeo };
    Kernel kernel() const {
        if (depthwise) return kDepthwise;
        if (groups > 1) return kGrouped;
        return kh == kw && (kh == 1 || kh == 3) && dh == 1 && dw == 1 ? kTile : kGeo;
    }
    static constexpr int kind() { return kLaunchConv; }
    template <class Fn> void views(Fn F) { F("in", in); F("res", res); }
};

// kLaunchElt: the fused elementwise program over the rows of `out` (the device-side marshaled form is EltArgs,
// graph_kernels.h)
struct EltProgram {
    std::vector<EltSrc> srcs;
    std::vector<EltInstr> code;
    int eltOut = 0;  // the register stored
    static constexpr int kind() { return kLaunchElt; }
    template <class Fn> void views(Fn F) { // a source that reads a device view is named by its mode
        static const char* const Name[] = {"srcSame", "srcBoard", "", "", "", "srcRankLine", "srcFileLine", "srcLine", "srcRowOne", "srcBoardOne", ""};
        for (EltSrc& S : srcs)
            if (S.mode == kSrcSame || S.mode == kSrcBoard || (S.mode >= kSrcRankLine && S.mode != kSrcSquare)) F(Name[S.mode], S.v);
    }
};

// kLaunchMean / kLaunchMax: the mean or the max (`max`) over the 81 squares of `in` -> a flat out
struct SquareReduceArgs {
    View in;
    bool max = false;
    int kind() const { return max ? kLaunchMax : kLaunchMean; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchConcat: the segments side by side along the channels (one segment: a plain copy)
struct ConcatSegs {
    std::vector<CopySeg> segs;
    static constexpr int kind() { return kLaunchConcat; }
    template <class Fn> void views(Fn F) {
        for (CopySeg& S : segs) F("seg", S.v);
    }
};

// kLaunchFlatten: a spatial `in` -> the flat [N,C*81] in ONNX order
struct FlattenArgs {
    View in;
    static constexpr int kind() { return kLaunchFlatten; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchPool: `in` (a spatial view at any channel offset) -> out, kh x kw taps at dilations dh, dw under the conv's
// halo rule, stride 1: the board stays 9x9
struct PoolArgs {
    View in;
    int kh = 3, kw = 3, dh = 1, dw = 1;
    int poolMode = kPoolMax;
    static constexpr int kind() { return kLaunchPool; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchLinePool: `in` (a spatial view at any channel offset) -> out, a 9-line view: the max (kPoolMax) or the mean
// (kPoolAvgInclude) of each rank over its files (lineFiles false, [N,C,9,1]) or of each file over its ranks (true,
// [N,C,1,9]).  out.line0 / out.bufLines place the nine lines inside an 18-line block.
struct LinePoolArgs {
    View in;
    bool lineFiles = false;
    int poolMode = kPoolMax;
    static constexpr int kind() { return kLaunchLinePool; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchLayerNorm: over the channels of each row of `in` (token rows or boards); gamma at wOff, beta at biasOff
struct LayerNormArgs {
    View in;
    size_t wOff = 0, biasOff = 0;
    float eps = 0.f;
    static constexpr int kind() { return kLaunchLayerNorm; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchGroupNorm: `in` (a spatial view at any channel offset) normalised per (board, group of C / groups consecutive
// channels), then gamma at wOff, beta at biasOff (both [C], the pattern's constants folded in double) and `act`
struct GroupNormArgs {
    View in;
    size_t wOff = 0, biasOff = 0;
    float eps = 0.f;
    int groups = 1;
    int act = kActNone;
    static constexpr int kind() { return kLaunchGroupNorm; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchRmsNorm: x / sqrt(mean(x^2) + eps) * gamma over the channels of each row of `in`; gamma at wOff
struct RmsNormArgs {
    View in;
    size_t wOff = 0;
    float eps = 0.f;
    static constexpr int kind() { return kLaunchRmsNorm; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchAttention: softmax(scale * q k^T + bias) v per (board, head) over the 81 squares.  q = `in`, k, v: token
// views of heads * headDim channels; bias (hasBias): [heads][81][81] at biasOff; out: token rows, head h at
// channels h * headDim
struct AttentionArgs {
    View in, attK, attV;
    int heads = 0, headDim = 0;
    float scale = 1.f;
    bool hasBias = false;
    size_t biasOff = 0;
    // ... plus rtScale times a bias computed at run time (hasRtBias): rtBias is a flat view whose stride is the floats
    // from one board to the next; head h, query q, key j at offset + h * rtHeadStride + q * 81 + j of the board's row.
    // rtHeadStride 0: one bias for all heads ([N,1,81,81]); 6561: a flat [N,H*6561]; 6576: head rows [N,H,6561].
    // Per score: acc * scale, then + bias, then + rtScale * rtBias, whatever order the graph wrote them in.
    View rtBias;
    int rtHeadStride = 0;
    float rtScale = 1.f;
    bool hasRtBias = false;
    static constexpr int kind() { return kLaunchAttention; }
    template <class Fn> void views(Fn F) {
        F("in", in); F("attK", attK); F("attV", attV);
        if (hasRtBias) F("rtBias", rtBias);
    }
};

// kLaunchBmm: the product of two run-time token tensors per board, out = act(scale * sum), the sum first, then the
// scalar, then `act` (a parameter-free Act).  A = `in`, B = `bmmB`, both token views at offsets that are multiples of 4.
// NT (bmmNN false): A [N,81,bmmK], B [N,81,bmmK] (the rows of the graph's [N,K,81] operand), out[n,i,j] = sum_k
// A[n,i,k] B[n,j,k], a token tensor of 81 channels.  NN: A [N,81,81], B [N,81,M], out[n,i,c] = sum_j A[n,i,j] B[n,j,c],
// bmmK = 81.
struct BmmArgs {
    View in, bmmB;
    bool bmmNN = false;
    int bmmK = 0;
    float scale = 1.f;
    int act = kActNone;
    static constexpr int kind() { return kLaunchBmm; }
    template <class Fn> void views(Fn F) { F("in", in); F("bmmB", bmmB); }
};

// kLaunchTokenMix: a Linear over the 81 squares of every channel of `in` (a spatial view of C channels at an offset
// that is a multiple of 4), one stage or two: out[n,j,c] = act2(sum_d W2[d][j] h[n,d,c] + b2[j]) with h[n,d,c] =
// act(sum_s W1[s][d] in[n,s,c] + b1[d]), mixD hidden units (mixStages 2); or out = h with mixD = 81 (mixStages 1).
// One constant record at wOff, with Dp = mixD rounded up to 16: W1 transposed [Dp][84], b1 [Dp], then for two
// stages W2 transposed [96][Dp] and b2 [96], every pad zero.  act, mixAct2: parameter-free Acts.
struct TokenMixArgs {
    View in;
    size_t wOff = 0;
    int mixD = 0;
    int mixStages = 0;
    int act = kActNone;
    int mixAct2 = kActNone;
    static constexpr int kind() { return kLaunchTokenMix; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchGather: a Gather with constant indices, or a board flip.  Per board the output has gatherRows rows (81: spatial
// or token rows; 1: a flat row) of out.stride floats, and the source is a block of gatherBlock floats (81 * in.stride for
// spatial or token rows, in.stride for a flat row) in `in`'s buffer.  Output element (r, c), c < out.C, is
// src[board * gatherBlock + rowTab[r] + colTab[c]] (in.offset is inside colTab); elements c >= out.C are zero.  The
// two int tables lie at gatherTabOff, stored bit for bit in the float blob as a grouped conv's table is: rowTab
// [gatherRows], then colTab[out.stride] with pad entries 0, each 16-byte aligned.  The planner checks every entry:
// max(rowTab) + max(colTab) < gatherBlock, none negative.  The device checks nothing.
struct GatherArgs {
    View in;
    int gatherRows = 0;
    long gatherBlock = 0;
    size_t gatherTabOff = 0;
    static constexpr int kind() { return kLaunchGather; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchChanReduce: the max, min, sum, L1 norm, sum of squares, L2 norm or log-sum-exp (redMode) over the in.C channels
// of every row of `in` (spatial or token rows, or flat rows; a view at any channel offset) -> out, a one-channel tensor
// of the same rows: channel 0 holds the result, channels 1..15 zeros.  A sum is multiplied by `scale` after its last
// add: 1 for ReduceSum, the f32 constant 1/C for a ReduceMean.
struct ChanReduceArgs {
    View in;
    int redMode = kRedMax;
    float scale = 1.f;
    static constexpr int kind() { return kLaunchChanReduce; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

// kLaunchNormalize: F.normalize over the channels, x / max(norm_p(x), eps) on every row of `in` (spatial or token rows,
// or flat rows; a view at any channel offset) -> out, a tensor of in.C channels of the same rows.  p: 1 or 2; eps > 0.
// The norm has the bits of kLaunchChanReduce's kRedL1 / kRedL2.  `out` is never `in`'s buffer: a row is read twice.
struct NormalizeArgs {
    View in;
    int p = 2;
    float eps = 0.f;
    static constexpr int kind() { return kLaunchNormalize; }
    template <class Fn> void views(Fn F) { F("in", in); }
};

using LaunchArgs = std::variant<ConvArgs, EltProgram, SquareReduceArgs, ConcatSegs, FlattenArgs, LayerNormArgs, AttentionArgs,
                                PoolArgs, GroupNormArgs, RmsNormArgs, BmmArgs, LinePoolArgs, TokenMixArgs, GatherArgs,
                                ChanReduceArgs, NormalizeArgs>;

struct Launch {
    std::string name; // the ONNX node(s) it runs
    View out;
    LaunchArgs args;
    int kind() const { // a LaunchKind
        return std::visit([](const auto& A) -> int { return A.kind(); }, args);
    }
    template <class T> bool is() const { return std::holds_alternative<T>(args); }
};

struct GraphPlan {
    int numChannels = 0;
    int planeStride = 0;           // the plane buffer's stride (numChannels rounded up to 16)
    std::vector<float> weights;    // every constant a launch reads, uploaded once per device
    // activation buffers: the widest spatial and flat strides each one holds (bytes for B boards: bufferFloats)
    std::vector<int> bufSpatialStride, bufFlatStride;
    std::vector<Launch> launches;  // in order; the plane expansion before and the output scatter after are implicit
    View policy, value, draw;      // policy: spatial C = 27 (read as c * 81 + square) or flat C = 2187
    // reported by nsg_get_graph_info / nsg_inspect_onnx
    int nodes = 0;
    int convLaunches = 0;
    int attentionLaunches = 0;
    uint64_t params = 0;
    double flopsPerPosition = 0.0;
    size_t activationBytesPerPosition = 0;
};

// Plans `data` (an ONNX ModelProto) for `numChannels` input planes.  Returns false and a message naming the node
// on anything outside the op set or the tensor contract.
bool buildPlan(const void* data, size_t size, int numChannels, GraphPlan* plan, std::string* error);

// Nodes of an ONNX model's graph (0 when it cannot be read).
int countNodes(const void* data, size_t size);

// Floats activation buffer `i` needs for `batch` boards: a flat tensor is read by the conv kernel (a dense layer) in
// groups of 81 rows, so its rows are padded to a multiple of 81.
inline size_t bufferFloats(const GraphPlan& P, size_t i, int batch) {
    const size_t s = (size_t)P.bufSpatialStride[i] * 81 * (size_t)batch;
    const size_t f = (size_t)P.bufFlatStride[i] * (((size_t)batch + 80) / 81 * 81);
    return s > f ? s : f;
}

} // namespace graph
} // namespace nsg

#endif
