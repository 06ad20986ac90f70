// graph_chanreduce.hip -- the general graph path's reduction over the channels of a row (kLaunchChanReduce): the max, the
// min, the sum, the L1 norm, the sum of squares, the L2 norm or the log-sum-exp of the C contiguous floats at channel
// `offset` of every row, written as a one-channel row (channel 0 the result, channels 1..outStride-1 zeros).  The gate of
// an sSE / CBAM block, a token score's amax or sum, the norm of an embedding, the normaliser of a softmax over channels.
//
// A streaming kernel: 16 lanes take one row, so a wave64 holds four rows and a workgroup of 256 threads sixteen.  The
// row's range [offset, offset + C) is cut, by (C, offset) alone, into
//   head   the 0..3 elements in front of the first 16-byte boundary    lane l < head reads element l          (scalar loads)
//   body   (C - head) / 4 float4s                                     lane l reads float4s l, l + 16, ...   (16-byte loads)
//   tail   the (C - head) % 4 elements behind the last float4         lane l < tail reads element l of them (scalar loads)
// Each lane folds its elements into one accumulator in that order (head, body ascending with x y z w of each float4 in
// turn, tail), starting from the identity (0, -inf, +inf), and the sixteen accumulators meet in a butterfly over lane
// distances 8, 4, 2, 1 (__shfl_xor inside the group of 16).  The order of every add is therefore a function of (C, offset)
// only, never of the batch or of the row's place in it: a board's bits do not depend on its neighbours.  Nothing outside
// [offset, offset + C) is read: a neighbouring channel of the view's buffer may hold an infinity.  The split and the
// fold are rowFold (graph_rowfold.h), which the fused normalise launch shares.
//
// A sum is multiplied by `scale` once, after the butterfly's last add (1 for ReduceSum: exact; the f32 constant 1/C for a
// ReduceMean).  Max and min go through fmaxf / fminf and give what those give: a NaN operand is dropped where the other
// operand is a number, so a row with some NaN elements gives the max / min of the others, and a row of nothing but NaN
// gives the identity the fold started from (-inf for a max, +inf for a min).  A sum propagates NaN.
//
// kRedL1 folds acc + fabsf(x) and kRedSumSq fmaf(x, x, acc), both from 0; the lanes' accumulators meet by addition.
// kRedL2 is sqrtf (correctly rounded) of the kRedSumSq result, once, after the butterfly.  There is no rescaling: x * x
// overflows where it overflows in f32, so a row with an element beyond 1.8e19 has the L2 norm +inf, and squares below
// the smallest denormal count as 0.
//
// kRedLogSumExp runs two passes over the row.  Pass 1 is the max fold and gives m.  If m is +inf or -inf the result is
// m: a row of nothing but -inf gives -inf, never NaN, and a row with a +inf gives +inf.  Otherwise pass 2 folds
// acc + expf(x - m) from 0 in the same lane and butterfly order (the row comes from cache) and the result is
// m + logf(s), s >= 1 up to rounding.  An element of -inf adds exactly 0.  A NaN element is dropped by the max and then
// propagates through the sum; a row of nothing but NaN has m = -inf and gives -inf, as the max does.
#include "graph_rowfold.h"

namespace nsg {
namespace graph {

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / kRowGroup;

template <int Mode>
__global__ __launch_bounds__(kThreads) void graphChanReduce(const float* __restrict__ in, int inStride, int inOff, int C,
                                                            float* __restrict__ out, int outStride, long rows, float scale) {
    const int lane = threadIdx.x % kRowGroup;
    const long row = (long)blockIdx.x * kRowsPerBlock + threadIdx.x / kRowGroup;
    const bool live = row < rows; // a dead group loads and stores nothing, but stays in the wave's shuffles
    const float* p = in + (size_t)(live ? row : 0) * inStride + inOff;
    float acc;
    if (Mode == kRedLogSumExp) {
        const float m = rowFold<kRedMax>(p, inOff, C, lane, live);
        // (every lane of a group holds the same m; the groups of a wave that skip pass 2 stay in its shuffles)
        const float s = rowFold<kFoldExpSum>(p, inOff, C, lane, live && fabsf(m) != INFINITY, m);
        acc = fabsf(m) != INFINITY ? m + logf(s) : m;
    } else if (Mode == kRedL2) {
        acc = sqrtf(rowFold<kRedSumSq>(p, inOff, C, lane, live));
    } else {
        acc = rowFold<Mode>(p, inOff, C, lane, live);
    }
    if (!live) return;
    if (Mode == kRedSum) acc *= scale;
    float* o = out + (size_t)row * outStride;
    for (int c = lane; c < outStride; c += kRowGroup) o[c] = c == 0 ? acc : 0.f;
}

template <int Mode>
void launchMode(dim3 grid, DevView in, float scale, float* out, int outStride, long rows, hipStream_t stream) {
    hipLaunchKernelGGL(graphChanReduce<Mode>, grid, dim3(kThreads), 0, stream, in.p, in.stride, in.offset, in.C, out, outStride, rows, scale);
}

} // namespace

hipError_t launchGraphChanReduce(DevView in, int mode, float scale, float* out, int outStride, long rows, hipStream_t stream) {
    if (rows <= 0 || in.C < 1 || in.offset < 0 || in.offset + in.C > in.stride || in.stride % 4 != 0 || outStride < 1 ||
        ((uintptr_t)in.p & 15) != 0 || !out)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock));
    switch (mode) {
    case kRedMax: launchMode<kRedMax>(grid, in, scale, out, outStride, rows, stream); break;
    case kRedMin: launchMode<kRedMin>(grid, in, scale, out, outStride, rows, stream); break;
    case kRedSum: launchMode<kRedSum>(grid, in, scale, out, outStride, rows, stream); break;
    case kRedL1: launchMode<kRedL1>(grid, in, scale, out, outStride, rows, stream); break;
    case kRedSumSq: launchMode<kRedSumSq>(grid, in, scale, out, outStride, rows, stream); break;
    case kRedL2: launchMode<kRedL2>(grid, in, scale, out, outStride, rows, stream); break;
    case kRedLogSumExp: launchMode<kRedLogSumExp>(grid, in, scale, out, outStride, rows, stream); break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
