// graph_norm.hip -- the normalisations of the general graph path that need no batch statistics.
//
// graphGroupNorm: GroupNorm / InstanceNorm on spatial rows (board x square, channel innermost).  Group g holds the
// Cg = C / G consecutive channels g Cg .. g Cg + Cg - 1 (Cg = 1: instance norm; Cg = C: one group; any value between,
// multiples of 4 or not, groups that straddle a 16-channel chunk included).  Per (board, group), over its n = 81 Cg
// elements: mean = sum(x) / n; var = sum((x - mean)^2) / n in a second pass (the biased variance, not E[x^2] - mean^2);
// inv = 1.f / sqrtf(var + eps); y = act((x - mean) inv gamma[c] + beta[c]).  Channels C..outStride-1 are written as
// zero.
//
//   * Work split.  A workgroup of 256 threads owns `gpw` whole groups of one board, so no statistic crosses a
//     workgroup; the grid is (board, ceil(G / gpw)).  gpw = min(G, max(1, 64 / Cg)): slabs of up to 64 channels, so
//     256 channels in 32 groups are four workgroups per board (as graphPool splits a board), G = 1 is one.
//   * Teams.  gpw >= 4: a wave owns the groups w, w + 4, ... of the slab, one after another.  gpw < 4 (wide groups):
//     all four waves work on each group in turn, and the four wave sums are added as ((w0 + w1) + w2) + w3.
//   * Order.  A team of T lanes (64 or 256) walks a group's elements e = sq Cg + c in index order: lane t adds
//     e = t, t + T, t + 2T, ... into one f32 partial, the 64 partials of a wave are added by the xor butterfly
//     32, 16, 8, 4, 2, 1.  gpw and T depend on (C, G) only: never on the batch, the grid or the input's offset.  No
//     atomics, no element of another board is read, so a board's output bits do not depend on its batch.
//   * Memory.  The input is a view at any channel offset of its rows, read where it lies: 16-byte pieces when the
//     slab's first channel falls on a multiple of 4 floats, scalar loads otherwise and for the slab's last 1..3
//     channels; nothing outside the slab is read.  A slab whose 81 rows of W channels, at an odd row stride, fit 64 KB
//     of LDS together with the kernel's 528 bytes of static LDS (W <= 199: 81 x 199 x 4 + 528 = 65 004 bytes; the odd
//     stride keeps the lanes of an instance norm, which walk one channel down the squares, on distinct banks) is read
//     from global memory once and the three passes run on LDS.  A wider slab -- one group of 200 channels or more:
//     G = 1 at C = 256 -- is not staged: the second and third pass re-read it (65 KB and more per board, which comes
//     from L2).  Static and dynamic LDS together never exceed 64 KB, so no attribute is needed.
//
// graphRmsNorm: one wave per row (token rows or boards), the shape of graphLayerNorm: ms = waveSum(x^2) / C with lane
// t adding channels t, t + 64, ... and the same butterfly, inv = 1.f / sqrtf(ms + eps), y = x inv gamma[c]; channels
// C..outStride-1 zero.  The input is a view at any offset.
#include <algorithm>

#include "graph_act.h"
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

constexpr int kNormThreads = 256;
constexpr int kNormSlab = 64;          // channels a workgroup aims for
constexpr int kNormStaticLds = (4 + 2 * kNormSlab) * 4; // sX, sMean, sInv below
constexpr int kNormMaxLdsW = 199;      // the widest slab held in LDS: 81 x 199 x 4 = 64 476 bytes beside the static 528
static_assert(81 * (kNormMaxLdsW | 1) * 4 + kNormStaticLds <= 65536 && 81 * ((kNormMaxLdsW + 1) | 1) * 4 + kNormStaticLds > 65536,
              "the widest staged slab and the static LDS fit the 64 KB a launch gets without opting in; the next does not");

__device__ inline float waveSum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the sum over a team: a wave, or (block) the four waves of the workgroup in the order ((w0 + w1) + w2) + w3
__device__ inline float teamSum(float v, bool block, float* sX) {
    v = waveSum(v);
    if (!block) return v;
    __syncthreads(); // the previous exchange has been read
    if ((threadIdx.x & 63) == 0) sX[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sX[0] + sX[1]) + sX[2]) + sX[3];
}

__global__ __launch_bounds__(kNormThreads) void graphGroupNorm(const float* __restrict__ in, int inStride, int inOff, int C,
                                                               int G, int gpw, int useLds, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, int act,
                                                               float* __restrict__ out, int outStride) {
    extern __shared__ __attribute__((aligned(16))) float sImg[];
    __shared__ float sX[4];
    __shared__ float sMean[kNormSlab], sInv[kNormSlab];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long b = blockIdx.x;
    const int Cg = C / G;
    const int g0 = blockIdx.y * gpw;
    const int ng = min(gpw, G - g0);     // groups of this workgroup
    const int cA = g0 * Cg, W = ng * Cg; // its slab: channels cA .. cA + W - 1
    const int Ws = W | 1;                // LDS floats per square
    const float* src = in + (size_t)b * 81 * inStride + inOff + cA;
    const bool block = gpw < 4;

    if (useLds) {
        const int Q = (W + 3) >> 2;
        const bool vec = ((inOff + cA) & 3) == 0;
        for (int i = tid; i < 81 * Q; i += kNormThreads) {
            const int sq = i / Q, c0 = (i - sq * Q) * 4;
            const float* p = src + (size_t)sq * inStride + c0;
            float* d = sImg + sq * Ws + c0;
            if (vec && c0 + 4 <= W) {
                const float4 v = *(const float4*)p;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            } else {
                d[0] = p[0];
                if (c0 + 1 < W) d[1] = p[1];
                if (c0 + 2 < W) d[2] = p[2];
                if (c0 + 3 < W) d[3] = p[3];
            }
        }
        __syncthreads();
    }
    // element (sq, c) of the slab
    auto ld = [&](int sq, int c) -> float { return useLds ? sImg[sq * Ws + c] : src[(size_t)sq * inStride + c]; };

    const int n = 81 * Cg;
    const int T = block ? kNormThreads : 64, t = block ? tid : lane;
    // block: every thread takes every group (the exchange in teamSum is a workgroup barrier); else a wave its own
    // lane t walks e = t, t + T, ... as (square, channel): one division here, then a carry per step
    const int sq0 = t / Cg, ch0 = t - sq0 * Cg, dsq = T / Cg, dc = T - dsq * Cg;
    for (int j = block ? 0 : wave; j < ng; j += block ? 1 : 4) {
        const int cj = j * Cg;
        float s = 0.f;
        for (int e = t, sq = sq0, c = ch0; e < n; e += T) {
            s += ld(sq, cj + c);
            sq += dsq; c += dc;
            if (c >= Cg) { c -= Cg; ++sq; }
        }
        const float mean = teamSum(s, block, sX) / (float)n;
        float q = 0.f;
        for (int e = t, sq = sq0, c = ch0; e < n; e += T) {
            const float dv = ld(sq, cj + c) - mean;
            q += dv * dv;
            sq += dsq; c += dc;
            if (c >= Cg) { c -= Cg; ++sq; }
        }
        const float inv = 1.f / sqrtf(teamSum(q, block, sX) / (float)n + eps);
        if (t == 0) { sMean[j] = mean; sInv[j] = inv; }
    }
    __syncthreads();

    // y: the slab, and behind the last group the pad channels C..outStride-1 as zero
    const int Wo = g0 + ng == G ? outStride - cA : W;
    const int Qo = (Wo + 3) >> 2;
    const bool vecOut = (cA & 3) == 0;
    float* dst = out + (size_t)b * 81 * outStride + cA;
    for (int i = tid; i < 81 * Qo; i += kNormThreads) {
        const int sq = i / Qo, c0 = (i - sq * Qo) * 4;
        float y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k;
            y[k] = 0.f;
            if (c < W) {
                const int j = c / Cg;
                y[k] = applyAct((ld(sq, c) - sMean[j]) * sInv[j] * gamma[cA + c] + beta[cA + c], act);
            }
        }
        float* p = dst + (size_t)sq * outStride + c0;
        if (vecOut && c0 + 4 <= Wo) {
            *(float4*)p = make_float4(y[0], y[1], y[2], y[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < Wo) p[k] = y[k];
        }
    }
}

__global__ __launch_bounds__(kNormThreads) void graphRmsNorm(const float* __restrict__ in, int inStride, int inOff, int C,
                                                             const float* __restrict__ gamma, float eps,
                                                             float* __restrict__ out, int outStride, long rows) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (kNormThreads / 64) + (threadIdx.x >> 6);
    if (row >= rows) return; // whole waves leave: the shuffles below see all 64 lanes
    const float* x = in + (size_t)row * inStride + inOff;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += x[c] * x[c];
    const float inv = 1.f / sqrtf(waveSum(s) / (float)C + eps);
    float* y = out + (size_t)row * outStride;
    for (int c = lane; c < outStride; c += 64) y[c] = c < C ? x[c] * inv * gamma[c] : 0.f;
}

} // namespace

hipError_t launchGraphGroupNorm(DevView in, int groups, const float* gamma, const float* beta, float eps, int act,
                                float* out, int outStride, int boards, hipStream_t stream) {
    if (boards <= 0 || in.C <= 0 || groups <= 0 || in.C % groups != 0 || in.offset < 0 || in.offset + in.C > in.stride ||
        in.stride % 4 != 0 || outStride % 16 != 0 || outStride < in.C || outStride - in.C >= 16)
        return hipErrorInvalidValue;
    const int Cg = in.C / groups;
    const int gpw = std::min(groups, std::max(1, kNormSlab / Cg));
    const int W = gpw * Cg; // the widest slab of the launch
    const int useLds = W <= kNormMaxLdsW;
    const size_t lds = useLds ? (size_t)81 * (W | 1) * sizeof(float) : 0;
    hipLaunchKernelGGL(graphGroupNorm, dim3((unsigned)boards, (unsigned)((groups + gpw - 1) / gpw)), dim3(kNormThreads), lds,
                       stream, in.p, in.stride, in.offset, in.C, groups, gpw, useLds, gamma, beta, eps, act, out, outStride);
    return hipGetLastError();
}

hipError_t launchGraphRmsNorm(DevView in, const float* gamma, float eps, float* out, int outStride, long rows,
                              hipStream_t stream) {
    if (rows <= 0 || in.C <= 0 || in.C > outStride || in.offset < 0 || in.offset + in.C > in.stride) return hipErrorInvalidValue;
    const long blocks = (rows + kNormThreads / 64 - 1) / (kNormThreads / 64);
    hipLaunchKernelGGL(graphRmsNorm, dim3((unsigned)blocks), dim3(kNormThreads), 0, stream, in.p, in.stride, in.offset, in.C,
                       gamma, eps, out, outStride, rows);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
