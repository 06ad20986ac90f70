// graph_kernels.h -- launch interface of the general graph path's kernels (graph_conv.hip, graph_pool.hip,
// graph_ops.hip, graph_attention.hip, graph_norm.hip, graph_bmm.hip, graph_linepool.hip, graph_gconv.hip, graph_tokenmix.hip,
// graph_gather.hip, graph_chanreduce.hip, graph_normalize.hip).  Their one caller for a plan's launches is ../graph_exec.hip, which marshals
// each argument record of onnx_graph.h (ConvArgs, EltProgram, ...) into the call below that runs it; nsg_capi.hip calls
// launchGraphOutputs only.
//
// Every tensor is f32 in the layout of onnx_graph.h: rows (board x square, or board) of `stride` floats, channel
// innermost, channels C..stride-1 written as zero.  A view (ptr, stride, offset) reads channels offset..offset+C-1.
#ifndef NSG_GRAPH_KERNELS_H
#define NSG_GRAPH_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../onnx_graph.h"

namespace nsg {
namespace graph {

struct DevView {
    const float* p = nullptr;
    int stride = 0, offset = 0, C = 0;
};

// Implicit-GEMM convolution on the f32 MFMA (v_mfma_f32_16x16x4_f32): M = groups x 81 rows, N = output channels,
// K = taps x cinPad.  taps 9: a 3x3 conv (dilation 1) of `groups` boards; taps 1: a 1x1 conv, or a dense layer when the rows are
// boards (then `groups` = ceil(boards / 81) and `rows` masks the last group).  w: packed [coutTiles][cinPad/16][taps]
// [16][64]; bias [coutTiles * 64].  y = act(acc + bias[c] (+ res)), written for rows < `rows`, channels < out stride.
hipError_t launchGraphConv(const float* in, int inStride, const float* w, const float* bias, DevView res,
                           float* out, int outStride, int cout, int cinPad, int coutTiles, int taps, int groups,
                           long rows, int act, hipStream_t stream);

// The same conv for every other geometry: kh x kw taps (odd, at most 9), dilations dh, dw, a halo dh (kh-1)/2 by
// dw (kw-1)/2 of at most kMaxConvHalo squares; `boards` boards of 81 rows.  w: packed [coutTiles][cinPad/16][kh * kw]
// [16][64], taps row-major over (ky, kx).  The sum of an output element runs in launchGraphConv's order (chunk, tap,
// channel): a 5x5 kernel whose outer ring is zero gives the bits of the 3x3 kernel at its centre.
hipError_t launchGraphConvGeo(const float* in, int inStride, const float* w, const float* bias, DevView res,
                              float* out, int outStride, int cout, int cinPad, int coutTiles, int kh, int kw, int dh,
                              int dw, int boards, int act, hipStream_t stream);

// Depthwise conv of the same geometries on the VALU: y[c] = act(sum over taps of x[c] w[c][tap] + bias[c] (+ res)), one
// fmaf chain per (square, channel) in row-major tap order.  w: [outStride/16][kh * kw][16]; bias [outStride];
// outStride = C rounded up to 16, the input's rows at least as wide.
hipError_t launchGraphDepthwise(const float* in, int inStride, const float* w, const float* bias, DevView res,
                                float* out, int outStride, int C, int kh, int kw, int dh, int dw, int boards, int act,
                                hipStream_t stream);

// Grouped conv (1 < group < Cin, Cin / group a multiple of 4) of the same geometries on the f32 MFMA (graph_gconv.hip):
// graphConvGeo's work split, but a tile of 64 outputs stages only the 16-channel input chunks its outputs' groups read
// and each wave issues MFMAs only for the chunks of its own 16 outputs.  w: packed [tile][chunk of the tile's range]
// [kh * kw][16][64], zeros across groups; tables: kGroupTabInts ints per tile (ConvArgs::gTabOff); bias [tiles * 64];
// tiles = ceil(cout / 64); inStride and outStride multiples of 16.  An output element is one f32 chain over (chunk
// ascending, tap row-major, the chunk's four k-steps ascending): launchGraphConv's chain restricted to the group's
// chunks, so with Cin / group a multiple of 16 it gives the bits of a group-1 conv on the group's channel slice.  A wave
// never reads a chunk outside its sub-range into an MFMA.
hipError_t launchGraphConvGrouped(const float* in, int inStride, const float* w, const float* bias, const int* tables,
                                  DevView res, float* out, int outStride, int cout, int kh, int kw, int dh, int dw,
                                  int boards, int act, hipStream_t stream);

// Fused elementwise chain (onnx_graph.h's EltProgram, marshaled for the device) over `rows` rows.
struct EltArgs {
    const float* src[kMaxEltSrcs];
    int stride[kMaxEltSrcs];
    int offset[kMaxEltSrcs];
    int mode[kMaxEltSrcs];  // EltMode; kSrcChannel, kSrcSquareChannel and kSrcSquare read constants at src
    int bufLines[kMaxEltSrcs], line0[kMaxEltSrcs]; // kSrcRankLine, kSrcFileLine, kSrcLine: the view's line fields
    float scalar[kMaxEltSrcs];
    uint32_t code[kMaxEltCode]; // op | dst << 8 | a << 16 | b << 24
    int ncode;
    int outReg;
    float* out;
    int outStride;
    int C;
    long rows;
    int outLines; // kSrcLine: the lines per board of the output (and of every such source)
};
hipError_t launchGraphElt(const EltArgs& a, hipStream_t stream);

// Mean over the 81 squares: [B*81][in] -> [B][outStride]
hipError_t launchGraphMean(DevView in, float* out, int outStride, int boards, hipStream_t stream);

// Max over the 81 squares, the same shapes; pad channels zero
hipError_t launchGraphMax(DevView in, float* out, int outStride, int boards, hipStream_t stream);

// MaxPool / AveragePool of kh x kw taps (odd, at most 9) at dilations dh, dw, stride 1, under the conv's halo rule: the
// board stays 9x9.  mode: PoolMode.  `in` may start at any channel of its rows (an offset that is no multiple of 4 is
// read with scalar loads); out: rows of outStride = C rounded up to 16, pad channels zero.  An average is the f32 sum
// of the window in row-major tap order, the halo as zeros, then one division by kh * kw (kPoolAvgInclude) or by the
// number of taps on the board (kPoolAvgExclude).
hipError_t launchGraphPool(DevView in, float* out, int outStride, int kh, int kw, int dh, int dw, int mode, int boards,
                           hipStream_t stream);

// Rank and file pooling: the max (kPoolMax) or the mean (kPoolAvgInclude) of each of a board's nine ranks over its files
// (files = 0) or of each of its nine files over its ranks (files = 1).  `in`: a spatial view at any channel offset (an
// offset that is no multiple of 4 is read with scalar loads).  out: line rows, row (board, l) at out + ((size_t)board *
// bufLines + line0 + l) * outStride with 9 <= line0 + 9 <= bufLines; outStride = C rounded up to 16, pad channels zero.
// The mean is the f32 sum of the line's nine elements in ascending square order, then one division by 9.
hipError_t launchGraphLinePool(DevView in, float* out, int outStride, int bufLines, int line0, int files, int mode,
                               int boards, hipStream_t stream);

// Channel concat (also a plain copy of one view): up to kMaxCopySegs views placed at channel dstOff[i]
struct ConcatArgs {
    const float* src[kMaxCopySegs];
    int stride[kMaxCopySegs];
    int offset[kMaxCopySegs];
    int count[kMaxCopySegs];
    int dstOff[kMaxCopySegs];
    int nseg;
    float* out;
    int outStride;
    long rows;
};
hipError_t launchGraphConcat(const ConcatArgs& a, hipStream_t stream);

// LayerNorm over the channels of each row (token rows or boards): y = (x - mean) / sqrt(var + eps) * gamma + beta, the
// biased variance, channels in.C..outStride-1 written as zero.  One wave per row.
hipError_t launchGraphLayerNorm(DevView in, const float* gamma, const float* beta, float eps, float* out,
                                int outStride, long rows, hipStream_t stream);

// GroupNorm on spatial rows: group g is the C / groups consecutive channels from g C / groups (groups = C: instance norm;
// groups = 1: one group), any group width.  Per (board, group) over its 81 C / groups elements: the mean, the biased
// variance as the mean of squared deviations in a second pass, y = act((x - mean) / sqrt(var + eps) * gamma[c] + beta[c]),
// act a parameter-free Act.  gamma, beta: [C].  `in` may start at any channel of its rows; out: rows of outStride = C
// rounded up to 16, pad channels zero.  Every statistic is summed in an order fixed by (C, groups): see graph_norm.hip.
hipError_t launchGraphGroupNorm(DevView in, int groups, const float* gamma, const float* beta, float eps, int act,
                                float* out, int outStride, int boards, hipStream_t stream);

// RMSNorm over the channels of each row (token rows or boards): y = x / sqrt(mean(x^2) + eps) * gamma[c], channels
// in.C..outStride-1 written as zero.  One wave per row; `in` may start at any channel.
hipError_t launchGraphRmsNorm(DevView in, const float* gamma, float eps, float* out, int outStride, long rows,
                              hipStream_t stream);

// Attention over the 81 squares, one workgroup per (board, head): out[:, h*d .. h*d+d-1] = softmax(scale * q_h k_h^T +
// bias[h]) v_h.  q, k, v: token views of heads * headDim channels at offsets that are multiples of 4; headDim a
// multiple of 4, at most kMaxHeadDim; bias: [heads][81][81] or null.
// rt (p null: none): a bias computed at run time, the element of (board, head, query, key) at p[board * boardStride +
// head * headStride + query * 81 + key]; headStride 0 broadcasts one bias over the heads, 6561 is a flat [N,H*6561]
// tensor, 6576 head rows [N,H,6561].  Per score: acc * scale, then + bias, then + rt.scale * rt; with rt.scale > 0
// (the planner refuses any other factor; the launch rejects it) an element of -inf gives probability exactly 0.  The
// loads are clamped to query 80 and key 80 of the (board, head) block: nothing outside it is read.
struct RtBias {
    const float* p = nullptr;
    long boardStride = 0;
    int headStride = 0;
    float scale = 1.f;
};
hipError_t launchGraphAttention(DevView q, DevView k, DevView v, const float* bias, float scale, RtBias rt, float* out,
                                int outStride, int heads, int headDim, int boards, hipStream_t stream);

// The product of two run-time token tensors per board (graph_bmm.hip), out = act(scale * sum): the sum is one f32 chain
// over k ascending that depends on (K, M) only, then one multiplication by `scale`, then a parameter-free Act.  Views
// at offsets that are multiples of 4, of any width >= 1; pad channels of `out` are written as zeros.
// NT: a, b [boards*81][K] -> out[n,i,j] = sum_k a[n,i,k] b[n,j,k], 81 channels at outStride = 96.
hipError_t launchGraphBmmNT(DevView a, DevView b, float scale, int act, float* out, int outStride, int boards,
                            hipStream_t stream);
// NN: p [boards*81][81], v [boards*81][M] -> out[n,i,c] = sum_j p[n,i,j] v[n,j,c], outStride = M rounded up to 16.
hipError_t launchGraphBmmNN(DevView p, DevView v, float scale, int act, float* out, int outStride, int boards,
                            hipStream_t stream);

// A Linear over the 81 squares of every channel, one stage or two in one launch (graph_tokenmix.hip): with Dp = D rounded
// up to 16 and the constant record consts = W1^T [Dp][84], b1 [Dp], W2^T [96][Dp], b2 [96] (the last two for two stages
// only; every pad zero),
//   h[n,d,c] = act1(sum_s W1^T[d][s] in[n,s,c] + b1[d]),   out[n,j,c] = act2(sum_d W2^T[j][d] h[n,d,c] + b2[j])
// and with one stage (D = 81) out = h.  `in`: a view at an offset that is a multiple of 4, of any width C >= 1; outStride =
// C rounded up to 16, pad channels written as zeros.  Every sum is one f32 chain whose order depends on D only; h never
// leaves the registers of the wave that computed it.
hipError_t launchGraphTokenMix(DevView in, const float* consts, int D, int stages, int act1, int act2, float* out,
                               int outStride, int boards, hipStream_t stream);

// A Gather with constant indices or a board flip (graph_gather.hip): per board, out[r][c] = src[board * blockFloats +
// rowTab[r] + colTab[c]] for r < rowsPerBoard, c < C, zeros for C <= c < outStride.  rowTab[rowsPerBoard] and
// colTab[outStride] (16-byte aligned, pad entries 0) are the planner's, which has checked that no entry is negative
// and that max(rowTab) + max(colTab) < blockFloats: the kernel reads nothing outside the board's block and checks
// nothing itself.  outStride a multiple of 16.  The output holds the source's bits.
hipError_t launchGraphGather(const float* src, long blockFloats, const int* rowTab, const int* colTab, float* out,
                             int outStride, int C, int rowsPerBoard, int boards, hipStream_t stream);

// The max (kRedMax), min (kRedMin) or sum (kRedSum) over the in.C channels of each of `rows` rows (graph_chanreduce.hip):
// out[row][0] = the result, a sum multiplied by `scale` once after its last add; out[row][1 .. outStride-1] = 0.  `in`
// may start at any channel of its rows (the ragged ends of an offset that is no multiple of 4 are read with scalar
// loads); nothing outside [offset, offset + C) is read.  in.stride a multiple of 4, in.p 16-byte aligned.  The order of a
// sum depends on (C, offset) only.  Max and min are fmaxf / fminf folds from -inf / +inf: a NaN element is skipped.
// kRedL1: the sum of fabsf(x); kRedSumSq: the sum of x * x as an fmaf chain; kRedL2: sqrtf of that, no rescaling (x * x
// overflows where it does in f32); kRedLogSumExp: m + logf(sum expf(x - m)) with m the row's max in a first pass, m
// itself where m is +inf or -inf (a row of -inf gives -inf).  The same lanes, fold order and butterfly for every mode.
hipError_t launchGraphChanReduce(DevView in, int mode, float scale, float* out, int outStride, long rows, hipStream_t stream);

// The L1 (p = 1) or L2 (p = 2) normalisation over the in.C channels of each of `rows` rows (graph_normalize.hip):
// out[row][c] = x[c] / fmaxf(n, eps) with n the row's norm exactly as launchGraphChanReduce's kRedL1 / kRedL2 computes
// it, eps > 0, the division correctly rounded; out[row][in.C .. outStride-1] = 0.  `in` may start at any channel of its
// rows and nothing outside [offset, offset + C) is read; in.stride and outStride multiples of 4, outStride >= in.C,
// in.p and out 16-byte aligned.  `out` must not overlap the rows of `in`: a row is read twice.
hipError_t launchGraphNormalize(DevView in, int p, float eps, float* out, int outStride, long rows, hipStream_t stream);

// [B*81][C] spatial view -> [B][outStride] flat in ONNX order (index c * 81 + square)
hipError_t launchGraphFlatten(DevView in, float* out, int outStride, int boards, hipStream_t stream);

// The evaluator's outputs: policy [B][2187] (from a spatial view read as c * 81 + square, or a flat view), value and
// draw [B] (flat views of one channel)
hipError_t launchGraphOutputs(DevView policy, bool policySpatial, DevView value, DevView draw, float* dstPolicy,
                              float* dstValue, float* dstDraw, int boards, hipStream_t stream);

} // namespace graph
} // namespace nsg

#endif
