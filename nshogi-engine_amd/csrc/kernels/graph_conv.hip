// graph_conv.hip -- the general graph path's convolution (and dense layer) kernel, exact f32 on the MFMA.
//
// A workgroup owns one group of 81 rows -- one board of a conv, or 81 boards of a dense layer -- and 64 output
// channels; its four waves take 16 channels each and all six 16-row fragments of the group (rows 81..95 repeat row
// 80 and are never stored).  Per 16-channel input chunk the group's rows are staged in LDS as an 11 x 11 image with
// a zero halo (the im2col-free image of DESIGN.md 4.2: a 3x3 tap is an offset into it), beside the chunk's packed
// weights; every tap then runs four k-steps of v_mfma_f32_16x16x4_f32 per fragment.  The result of a row is a
// k-ordered f32 chain over (chunk, tap, channel) that no other row touches: it does not depend on the batch it
// came with.  No split-K, no atomics.
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kHalo = 121;    // 11 x 11 positions
constexpr int kInStride = 17; // LDS floats per position: 16 channels + 1 (consecutive rows fall on distinct banks)
constexpr int kWStride = 80;  // LDS floats per (tap, k) row of 64 outputs: the four k rows of a step on distinct banks

__device__ inline float applyAct(float v, int act) {
    switch (act) {
    case kActRelu: return v > 0.f ? v : 0.f;
    case kActSigmoid: return 1.f / (1.f + expf(-v));
    case kActTanh: return tanhf(v);
    case kActSwish: return v / (1.f + expf(-v));
    case kActSoftplus: return v > 20.f ? v : log1pf(expf(v)); // torch's threshold
    case kActErf: return erff(v);
    case kActGelu: return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); // exact GELU
    default: return v;
    }
}

template <int TAPS>
__global__ __launch_bounds__(kThreads) void graphConv(const float* __restrict__ in, int inStride,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ res, int resStride, int resOff,
                                                      float* __restrict__ out, int outStride, int cout, int cinPad,
                                                      long rows, int act) {
    __shared__ float sIn[kHalo * kInStride];
    __shared__ __attribute__((aligned(16))) float sW[TAPS * 16 * kWStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x;
    const int tile = blockIdx.y;
    const int chunks = cinPad / 16;
    const float* wt = w + (size_t)tile * chunks * TAPS * 16 * 64;
    const int kq = lane >> 4, col = lane & 15;
    int pos[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int r = min(f * 16 + col, 80);
        pos[f] = (r / 9 + 1) * 11 + (r % 9 + 1);
    }
    f32x4 acc[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < chunks; ++ch) {
        __syncthreads();
        for (int i = tid; i < kHalo * 4; i += kThreads) {
            const int p = i >> 2, q = i & 3;
            const int y = p / 11 - 1, x = p % 11 - 1;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (y >= 0 && y < 9 && x >= 0 && x < 9)
                v = *(const float4*)(in + (size_t)(g * 81 + y * 9 + x) * inStride + ch * 16 + q * 4);
            float* d = sIn + p * kInStride + q * 4;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
        const float* wc = wt + (size_t)ch * TAPS * 16 * 64;
        for (int i = tid; i < TAPS * 16 * 16; i += kThreads) {
            const int row = i >> 4, q = i & 15;
            *(float4*)(sW + row * kWStride + q * 4) = *(const float4*)(wc + row * 64 + q * 4);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TAPS; ++t) {
            const int off = TAPS == 9 ? (t / 3 - 1) * 11 + (t % 3 - 1) : 0;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const int k = k4 * 4 + kq;
                const float b = sW[(t * 16 + k) * kWStride + wave * 16 + col];
#pragma unroll
                for (int f = 0; f < 6; ++f) {
                    const float a = sIn[(pos[f] + off) * kInStride + k];
                    acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[f], 0, 0, 0);
                }
            }
        }
    }
    // acc[f][i] = C[row f*16 + 4*kq + i][channel col] of this wave's 16 channels
    const int cl = tile * 64 + wave * 16 + col;
    if (cl >= outStride) return;
    const float bc = bias[cl];
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = f * 16 + 4 * kq + i;
            const long row = g * 81 + r;
            if (r >= 81 || row >= rows) continue;
            float v = 0.f;
            if (cl < cout) {
                v = acc[f][i] + bc;
                if (res) v += res[(size_t)row * resStride + resOff + cl];
                v = applyAct(v, act);
            }
            out[(size_t)row * outStride + cl] = v;
        }
}

} // namespace

hipError_t launchGraphConv(const float* in, int inStride, const float* w, const float* bias, DevView res,
                           float* out, int outStride, int cout, int cinPad, int coutTiles, int taps, int groups,
                           long rows, int act, hipStream_t stream) {
    if (groups <= 0 || cinPad % 16 != 0 || inStride % 4 != 0 || inStride < cinPad || coutTiles * 64 < cout)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)groups, (unsigned)coutTiles);
    if (taps == 9)
        hipLaunchKernelGGL(graphConv<9>, grid, dim3(kThreads), 0, stream, in, inStride, w, bias, res.p, res.stride,
                           res.offset, out, outStride, cout, cinPad, rows, act);
    else if (taps == 1)
        hipLaunchKernelGGL(graphConv<1>, grid, dim3(kThreads), 0, stream, in, inStride, w, bias, res.p, res.stride,
                           res.offset, out, outStride, cout, cinPad, rows, act);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
