// graph_normalize.hip -- the general graph path's fused L1 / L2 normalisation over the channels of a row
// (kLaunchNormalize): what F.normalize(x, p, dim = channels, eps) exports as ReduceL1 / ReduceL2 -> Clip(min = eps) ->
// [Expand] -> Div, in one launch that reads x from memory once.  For each of `rows` rows of the view:
//   n      the L1 norm (fold acc + fabsf(x) from 0) or the L2 norm (fold fmaf(x, x, acc) from 0, then one correctly
//          rounded sqrtf), by rowFold (graph_rowfold.h): the lane split, the fold order and the butterfly of
//          graph_chanreduce.hip's kRedL1 / kRedL2, so n has the bits of the stand-alone reduction;
//   d      fmaxf(n, eps), eps > 0: what the elementwise launch computes for the Clip (a NaN norm gives eps);
//   out[c] x[c] / d for c < C, the correctly rounded division the elementwise Div uses; 0 for C <= c < outStride.
// So the launch gives, bit for bit, what kLaunchChanReduce and the elementwise Clip and Div give in two launches.  No
// rescaling in the L2 norm: x * x overflows where it overflows in f32 (then n = +inf and the row is 0, or NaN where x is inf).
//
// A streaming kernel, wave64, no LDS, no atomics: 16 lanes take one row, as in graphChanReduce, whatever the rows are
// (board x square rows of a spatial or token tensor, or the boards of a flat one).  The row is read twice by the same 16
// lanes, once for the norm and once for the division: the second read comes from cache.  The second pass walks the
// output's float4s (lane l writes float4s l, l + 16, ...), reading the input with 16-byte loads where the view's offset
// is a multiple of 4 and the float4 lies inside [offset, offset + C), with scalar loads of the elements inside it
// otherwise: nothing outside the view's range is read.  A dead row group loads and stores nothing, but stays in the
// wave's shuffles.
#include "graph_rowfold.h"

namespace nsg {
namespace graph {

namespace {

constexpr int kThreads = 256;
constexpr int kRowsPerBlock = kThreads / kRowGroup;

template <int P>
__global__ __launch_bounds__(kThreads) void graphNormalize(const float* __restrict__ in, int inStride, int inOff, int C, float eps,
                                                           float* __restrict__ out, int outStride, long rows) {
    const int lane = threadIdx.x % kRowGroup;
    const long row = (long)blockIdx.x * kRowsPerBlock + threadIdx.x / kRowGroup;
    const bool live = row < rows;
    const float* p = in + (size_t)(live ? row : 0) * inStride + inOff;
    const float n = P == 1 ? rowFold<kRedL1>(p, inOff, C, lane, live) : sqrtf(rowFold<kRedSumSq>(p, inOff, C, lane, live));
    if (!live) return;
    const float d = fmaxf(n, eps);
    const bool aligned = (inOff & 3) == 0; // then p + 4 j is 16-byte aligned: rows are
    float4* o = reinterpret_cast<float4*>(out + (size_t)row * outStride);
    for (int j = lane; j < outStride >> 2; j += kRowGroup) {
        const int c = 4 * j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (aligned && c + 4 <= C) {
            v = *reinterpret_cast<const float4*>(p + c);
        } else {
            if (c < C) v.x = p[c];
            if (c + 1 < C) v.y = p[c + 1];
            if (c + 2 < C) v.z = p[c + 2];
            if (c + 3 < C) v.w = p[c + 3];
        }
        float4 y;
        y.x = c < C ? v.x / d : 0.f;
        y.y = c + 1 < C ? v.y / d : 0.f;
        y.z = c + 2 < C ? v.z / d : 0.f;
        y.w = c + 3 < C ? v.w / d : 0.f;
        o[j] = y;
    }
}

} // namespace

hipError_t launchGraphNormalize(DevView in, int p, float eps, float* out, int outStride, long rows, hipStream_t stream) {
    if (rows <= 0 || in.C < 1 || in.offset < 0 || in.offset + in.C > in.stride || in.stride % 4 != 0 || outStride % 4 != 0 ||
        outStride < in.C || ((uintptr_t)in.p & 15) != 0 || !out || ((uintptr_t)out & 15) != 0 || !(eps > 0.f) || (p != 1 && p != 2))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)), block(kThreads);
    if (p == 1) hipLaunchKernelGGL(graphNormalize<1>, grid, block, 0, stream, in.p, in.stride, in.offset, in.C, eps, out, outStride, rows);
    else hipLaunchKernelGGL(graphNormalize<2>, grid, block, 0, stream, in.p, in.stride, in.offset, in.C, eps, out, outStride, rows);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
