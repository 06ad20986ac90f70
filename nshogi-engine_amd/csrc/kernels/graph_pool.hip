// graph_pool.hip -- MaxPool and AveragePool of the general graph path: kh x kw taps (odd, at most 9) at dilations dh,
// dw, stride 1, a halo of at most kMaxConvHalo squares, so the board stays 9x9.  A VALU kernel on graphDepthwise's
// haloed LDS image, without weights to stage:
//
//   * the grid is (board, group of up to four 16-channel chunks): a board of 256 channels is four workgroups, not one
//     that walks sixteen chunks one after another;
//   * a workgroup of 192 threads stages the group's image once -- (9 + 2 hy) x (9 + 2 hx) positions of 16 g channels,
//     16-byte channel-contiguous global reads, the halo filled with -inf (max: every window holds its own centre, so
//     the halo never wins) or 0 (the averages) -- and then a thread owns a (square, 4-channel group): 324 g items,
//     1296 at g = 4, which is 6.75 passes of 192 threads (an image of 16 g floats per position needs no padding: the
//     lanes of a wave read consecutive 16-byte pieces along a board row);
//   * the image is dynamic LDS, sized by the geometry: 30 976 B for a 3x3 window at g = 4; a 17 x 17 image takes g = 3
//     (55 488 B) to stay under 64 KB.
//
// Order contract.  Max is exact in any order.  An average is the f32 sum of the window's taps in row-major order
// (ky outer, kx inner), a tap in the halo adding 0, followed by ONE division: by kh * kw (count_include_pad = 1) or by
// the number of the square's taps that lie on the board (count_include_pad = 0), which depends on (y, x) only.  No
// element reads another board or another channel, so a board does not depend on its batch or on the grouping.
//
// The input is a view: it may start at any channel of its rows.  Pieces of a view whose offset is a multiple of 4 are
// read as float4; any other offset, and the piece that holds the view's last channels when C is no multiple of 4, is
// read with scalar loads of the channels below C (nothing past the view is read).  Channels C..outStride-1 are
// written as zero.
#include <algorithm>

#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

constexpr int kPoolThreads = 192;
constexpr int kPoolChunks = 4;        // 16-channel chunks per workgroup, fewer when the image would not fit
constexpr int kPoolLdsBytes = 65536;  // the dynamic LDS a launch may ask for without opting in

__global__ __launch_bounds__(kPoolThreads) void graphPool(const float* __restrict__ in, int inStride, int inOff, int C,
                                                          float* __restrict__ out, int outStride, int kh, int kw,
                                                          int dh, int dw, int mode, int group) {
    extern __shared__ __attribute__((aligned(16))) float sImg[];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int chunk0 = blockIdx.y * group;
    const int g = min(group, outStride / 16 - chunk0);
    const int hy = dh * (kh - 1) / 2, hx = dw * (kw - 1) / 2, W = 9 + 2 * hx, H = 9 + 2 * hy;
    const int q4 = g * 4, ls = g * 16; // 16-byte pieces and floats per position
    const float fill = mode == kPoolMax ? -INFINITY : 0.f;
    const bool vec = (inOff & 3) == 0;

    for (int i = tid; i < H * W * q4; i += kPoolThreads) {
        const int p = i / q4, q = i - p * q4;
        const int y = p / W - hy, x = p % W - hx;
        const int c0 = chunk0 * 16 + q * 4;
        float4 v = make_float4(fill, fill, fill, fill);
        if (y >= 0 && y < 9 && x >= 0 && x < 9 && c0 < C) {
            const float* src = in + (size_t)(b * 81 + y * 9 + x) * inStride + inOff + c0;
            if (vec && c0 + 4 <= C) {
                v = *(const float4*)src;
            } else {
                v.x = src[0];
                if (c0 + 1 < C) v.y = src[1];
                if (c0 + 2 < C) v.z = src[2];
                if (c0 + 3 < C) v.w = src[3];
            }
        }
        *(float4*)(sImg + p * ls + q * 4) = v;
    }
    __syncthreads();
    for (int i = tid; i < 81 * q4; i += kPoolThreads) {
        const int sq = i / q4, q = i - sq * q4;
        const int y = sq / 9, x = sq - y * 9;
        const float* a = sImg + (y * W + x) * ls + q * 4;
        float4 s;
        if (mode == kPoolMax) {
            s = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx) {
                    const float4 t = *(const float4*)(a + (ky * dh * W + kx * dw) * ls);
                    s.x = fmaxf(s.x, t.x); s.y = fmaxf(s.y, t.y); s.z = fmaxf(s.z, t.z); s.w = fmaxf(s.w, t.w);
                }
        } else {
            s = make_float4(0.f, 0.f, 0.f, 0.f);
            int ny = 0, nx = 0; // taps on the board along each axis
            for (int ky = 0; ky < kh; ++ky) {
                const int yy = y - hy + ky * dh;
                ny += yy >= 0 && yy < 9;
                for (int kx = 0; kx < kw; ++kx) {
                    const float4 t = *(const float4*)(a + (ky * dh * W + kx * dw) * ls);
                    s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
                }
            }
            for (int kx = 0; kx < kw; ++kx) {
                const int xx = x - hx + kx * dw;
                nx += xx >= 0 && xx < 9;
            }
            const float div = mode == kPoolAvgInclude ? (float)(kh * kw) : (float)(ny * nx);
            s.x /= div; s.y /= div; s.z /= div; s.w /= div;
        }
        const int c0 = chunk0 * 16 + q * 4;
        if (c0 + 0 >= C) s.x = 0.f;
        if (c0 + 1 >= C) s.y = 0.f;
        if (c0 + 2 >= C) s.z = 0.f;
        if (c0 + 3 >= C) s.w = 0.f;
        *(float4*)(out + ((size_t)b * 81 + sq) * outStride + c0) = s;
    }
}

} // namespace

hipError_t launchGraphPool(DevView in, float* out, int outStride, int kh, int kw, int dh, int dw, int mode, int boards,
                           hipStream_t stream) {
    const bool geometry = kh >= 1 && kw >= 1 && kh <= 9 && kw <= 9 && (kh & 1) && (kw & 1) && dh >= 1 && dw >= 1 &&
                          dh * (kh - 1) / 2 <= kMaxConvHalo && dw * (kw - 1) / 2 <= kMaxConvHalo;
    if (boards <= 0 || !geometry || mode < kPoolMax || mode > kPoolAvgExclude || in.C <= 0 || in.offset < 0 ||
        in.offset + in.C > in.stride || in.stride % 4 != 0 || outStride % 16 != 0 || outStride < in.C ||
        outStride - in.C >= 16)
        return hipErrorInvalidValue;
    const int positions = (9 + 2 * (dh * (kh - 1) / 2)) * (9 + 2 * (dw * (kw - 1) / 2));
    const int chunks = outStride / 16;
    const int group = std::min(std::min(kPoolChunks, chunks), kPoolLdsBytes / (positions * 64));
    const size_t lds = (size_t)positions * group * 64;
    hipLaunchKernelGGL(graphPool, dim3((unsigned)boards, (unsigned)((chunks + group - 1) / group)), dim3(kPoolThreads), lds,
                       stream, in.p, in.stride, in.offset, in.C, out, outStride, kh, kw, dh, dw, mode, group);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
