// graph_linepool.hip -- rank and file pooling of the general graph path: the max or the mean of a spatial tensor
// along one board axis.  Rank lines ([N,C,9,1]) hold one value per rank, reduced over the nine files of that rank;
// file lines ([N,C,1,9]) one value per file, reduced over its nine ranks.  The nine lines of a board come out of one
// launch; orientation and mode are launch arguments.
//
//   * a thread owns a (board, line, 4-channel group): nine channel-contiguous loads, one 16-byte store.  There is
//     nothing to share between threads (every input element is read once), so there is no LDS and no barrier; the
//     lanes of a wave walk consecutive 16-byte pieces of a row, then the next line;
//   * pieces of a view whose offset is a multiple of 4 are read as float4; any other offset, and the piece that holds
//     the view's last channels when C is no multiple of 4, is read with scalar loads of the channels below C.  Nothing
//     outside the board's 81 rows or the view's channels is read;
//   * the output row of (board, line) is row board * bufLines + line0 + line, so the nine lines can land in either
//     half of an 18-line block (the Concat of two rank-line tensors costs no launch of its own).
//
// Order contract.  The max is exact: fmaxf from -inf over the line's squares in ascending order, graphPool's sequence
// for a 1x9 or 9x1 window that holds the whole line.  The mean is the f32 sum of the line's nine elements in ascending
// square order, starting from the first element, followed by ONE division by 9.  No atomics; no element reads another
// board, line or channel, so nothing depends on the batch or the grid.  Channels C..outStride-1 are written as zero.
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

constexpr int kLineThreads = 256;

__global__ __launch_bounds__(kLineThreads) void graphLinePool(const float* __restrict__ in, int inStride, int inOff, int C,
                                                              float* __restrict__ out, int outStride, int bufLines,
                                                              int line0, int files, int mode, int boards) {
    const int q4 = outStride >> 2;
    const long idx = (long)blockIdx.x * kLineThreads + threadIdx.x;
    if (idx >= (long)boards * 9 * q4) return;
    const long bl = idx / q4;
    const int c0 = (int)(idx - bl * q4) * 4;
    const long b = bl / 9;
    const int line = (int)(bl - b * 9);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < C) {
        // rank lines: squares line * 9 + 0..8; file lines: squares line + 9 * (0..8)
        const int sq0 = files ? line : line * 9, step = files ? 9 : 1;
        const float* src = in + (size_t)(b * 81 + sq0) * inStride + inOff + c0;
        const bool vec = (inOff & 3) == 0 && c0 + 4 <= C;
        const bool max = mode == kPoolMax;
        if (max) s = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float* p = src + (size_t)(k * step) * inStride;
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (vec) {
                t = *(const float4*)p;
            } else {
                t.x = p[0];
                if (c0 + 1 < C) t.y = p[1];
                if (c0 + 2 < C) t.z = p[2];
                if (c0 + 3 < C) t.w = p[3];
            }
            if (max) {
                s.x = fmaxf(s.x, t.x); s.y = fmaxf(s.y, t.y); s.z = fmaxf(s.z, t.z); s.w = fmaxf(s.w, t.w);
            } else if (k == 0) {
                s = t;
            } else {
                s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
            }
        }
        if (!max) { s.x /= 9.f; s.y /= 9.f; s.z /= 9.f; s.w /= 9.f; }
        if (c0 + 1 >= C) s.y = 0.f;
        if (c0 + 2 >= C) s.z = 0.f;
        if (c0 + 3 >= C) s.w = 0.f;
    }
    *(float4*)(out + ((size_t)b * bufLines + line0 + line) * outStride + c0) = s;
}

} // namespace

hipError_t launchGraphLinePool(DevView in, float* out, int outStride, int bufLines, int line0, int files, int mode,
                               int boards, hipStream_t stream) {
    if (boards <= 0 || (mode != kPoolMax && mode != kPoolAvgInclude) || in.C <= 0 || in.offset < 0 ||
        in.offset + in.C > in.stride || in.stride % 4 != 0 || outStride % 16 != 0 || outStride < in.C ||
        outStride - in.C >= 16 || line0 < 0 || line0 + 9 > bufLines)
        return hipErrorInvalidValue;
    const long items = (long)boards * 9 * (outStride / 4);
    hipLaunchKernelGGL(graphLinePool, dim3((unsigned)((items + kLineThreads - 1) / kLineThreads)), dim3(kLineThreads), 0,
                       stream, in.p, in.stride, in.offset, in.C, out, outStride, bufLines, line0, files ? 1 : 0, mode, boards);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
