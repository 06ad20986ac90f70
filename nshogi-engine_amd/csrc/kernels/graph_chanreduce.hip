// graph_chanreduce.hip -- the general graph path's reduction over the channels of a row (kLaunchChanReduce): the max, the
// min or the sum of the C contiguous floats at channel `offset` of every row, written as a one-channel row (channel 0
// the result, channels 1..outStride-1 zeros).  The gate of an sSE / CBAM block, a token score's amax or sum.
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
// [offset, offset + C) is read: a neighbouring channel of the view's buffer may hold an infinity.
//
// A sum is multiplied by `scale` once, after the butterfly's last add (1 for ReduceSum: exact; the f32 constant 1/C for a
// ReduceMean).  Max and min go through fmaxf / fminf and give what those give: a NaN operand is dropped where the other
// operand is a number, so a row with some NaN elements gives the max / min of the others, and a row of nothing but NaN
// gives the identity the fold started from (-inf for a max, +inf for a min).  A sum propagates NaN.
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

constexpr int kThreads = 256;
constexpr int kGroup = 16;                   // lanes per row
constexpr int kRowsPerBlock = kThreads / kGroup;

template <int Mode> __device__ __forceinline__ float fold(float a, float b) {
    return Mode == kRedMax ? fmaxf(a, b) : Mode == kRedMin ? fminf(a, b) : a + b;
}

template <int Mode>
__global__ __launch_bounds__(kThreads) void graphChanReduce(const float* __restrict__ in, int inStride, int inOff, int C,
                                                            float* __restrict__ out, int outStride, long rows, float scale) {
    const int lane = threadIdx.x % kGroup;
    const long row = (long)blockIdx.x * kRowsPerBlock + threadIdx.x / kGroup;
    const bool live = row < rows; // a dead group loads and stores nothing, but stays in the wave's shuffles
    float acc = Mode == kRedMax ? -INFINITY : Mode == kRedMin ? INFINITY : 0.f;
    if (live) {
        const float* p = in + (size_t)row * inStride + inOff;
        const int lead = (4 - (inOff & 3)) & 3;
        const int head = lead < C ? lead : C;
        const int body = (C - head) >> 2, tail = (C - head) & 3;
        if (lane < head) acc = fold<Mode>(acc, p[lane]);
        const float4* q = reinterpret_cast<const float4*>(p + head); // 16-byte aligned: rows are, and inOff + head is a multiple of 4
        for (int i = lane; i < body; i += kGroup) {
            const float4 v = q[i];
            acc = fold<Mode>(fold<Mode>(fold<Mode>(fold<Mode>(acc, v.x), v.y), v.z), v.w);
        }
        if (lane < tail) acc = fold<Mode>(acc, p[head + 4 * body + lane]);
    }
    for (int d = kGroup / 2; d > 0; d >>= 1) acc = fold<Mode>(acc, __shfl_xor(acc, d, kGroup));
    if (!live) return;
    if (Mode == kRedSum) acc *= scale;
    float* o = out + (size_t)row * outStride;
    for (int c = lane; c < outStride; c += kGroup) o[c] = c == 0 ? acc : 0.f;
}

} // namespace

hipError_t launchGraphChanReduce(DevView in, int mode, float scale, float* out, int outStride, long rows, hipStream_t stream) {
    if (rows <= 0 || in.C < 1 || in.offset < 0 || in.offset + in.C > in.stride || in.stride % 4 != 0 || outStride < 1 ||
        ((uintptr_t)in.p & 15) != 0 || !out)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock)), block(kThreads);
    switch (mode) {
    case kRedMax:
        hipLaunchKernelGGL(graphChanReduce<kRedMax>, grid, block, 0, stream, in.p, in.stride, in.offset, in.C, out, outStride, rows, scale);
        break;
    case kRedMin:
        hipLaunchKernelGGL(graphChanReduce<kRedMin>, grid, block, 0, stream, in.p, in.stride, in.offset, in.C, out, outStride, rows, scale);
        break;
    case kRedSum:
        hipLaunchKernelGGL(graphChanReduce<kRedSum>, grid, block, 0, stream, in.p, in.stride, in.offset, in.C, out, outStride, rows, scale);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
