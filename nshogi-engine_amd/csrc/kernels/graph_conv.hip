// graph_conv.hip -- the general graph path's convolution (and dense layer) kernel, exact f32 on the MFMA.
//
// A workgroup owns one group of 81 rows -- one board of a conv, or 81 boards of a dense layer -- and 64 output
// channels; its four waves take 16 channels each and all six 16-row fragments of the group (rows 81..95 repeat row
// 80 and are never stored).  Per 16-channel input chunk the group's rows are staged in LDS as an 11 x 11 image with
// a zero halo (the im2col-free image of DESIGN.md 4.2: a 3x3 tap is an offset into it), beside the chunk's packed
// weights; every tap then runs four k-steps of v_mfma_f32_16x16x4_f32 per fragment.  The result of a row is a
// k-ordered f32 chain over (chunk, tap, channel) that no other row touches: it does not depend on the batch it
// came with.  No split-K, no atomics.
//
// graphConvGeo is the same kernel for every other geometry (kh x kw taps, dilations, a halo of up to 4 squares): the
// image grows to (9 + 2 hy) x (9 + 2 hx) positions and the chunk's weights are staged in groups of up to 8 taps.  Its
// sum runs in graphConv's order -- chunk, tap (row-major), channel -- whatever the grouping.  graphDepthwise is the
// per-channel conv on the VALU: the same image, one fmaf chain per (square, channel) in row-major tap order.
#include "graph_act.h"
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kHalo = 121;    // 11 x 11 positions
constexpr int kInStride = 17; // LDS floats per position: 16 channels + 1 (consecutive rows fall on distinct banks)
constexpr int kWStride = 80;  // LDS floats per (tap, k) row of 64 outputs: the four k rows of a step on distinct banks

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

// ---- every other geometry ---------------------------------------------------------------------------------------
constexpr int kGeoSide = 9 + 2 * kMaxConvHalo;
constexpr int kGeoPos = kGeoSide * kGeoSide; // 17 x 17 positions: 19 652 B at kInStride floats each
constexpr int kGeoTapGroup = 8;              // taps of weights in LDS at a time: 8 x 5 120 B beside the image, under 64 KB
constexpr int kGeoStage = (kGeoPos * 4 + kThreads - 1) / kThreads; // 16-byte pieces of the image a thread stages

// What the float4 piece i of the haloed image shows: a square of the board (0..80), -1 in the halo, -2 past the image
__device__ inline int imageSource(int i, int hy, int hx) {
    const int W = 9 + 2 * hx, p = i >> 2;
    if (p >= (9 + 2 * hy) * W) return -2;
    const int y = p / W - hy, x = p % W - hx;
    return y >= 0 && y < 9 && x >= 0 && x < 9 ? y * 9 + x : -1;
}

__global__ __launch_bounds__(kThreads) void graphConvGeo(const float* __restrict__ in, int inStride,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         const float* __restrict__ res, int resStride, int resOff,
                                                         float* __restrict__ out, int outStride, int cout, int cinPad,
                                                         long rows, int act, int kh, int kw, int dh, int dw,
                                                         int tapGroup) {
    __shared__ float sIn[kGeoPos * kInStride];
    __shared__ __attribute__((aligned(16))) float sW[kGeoTapGroup * 16 * kWStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long g = blockIdx.x;
    const int tile = blockIdx.y;
    const int chunks = cinPad / 16, taps = kh * kw;
    const int hy = dh * (kh - 1) / 2, hx = dw * (kw - 1) / 2, W = 9 + 2 * hx;
    const float* wt = w + (size_t)tile * chunks * taps * 16 * 64;
    const int kq = lane >> 4, col = lane & 15;
    // a row's square sits at (y + hy, x + hx) of the image and tap (ky, kx) reads (y + ky dh, x + kx dw)
    int aBase[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int r = min(f * 16 + col, 80);
        aBase[f] = ((r / 9) * W + r % 9) * kInStride + kq;
    }
    int src[kGeoStage];
#pragma unroll
    for (int j = 0; j < kGeoStage; ++j) src[j] = imageSource(tid + j * kThreads, hy, hx);
    f32x4 acc[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < chunks; ++ch) {
        const float* wc = wt + (size_t)ch * taps * 16 * 64;
        int ky = 0, kx = 0;
        for (int t0 = 0; t0 < taps; t0 += tapGroup) {
            const int n = min(tapGroup, taps - t0);
            __syncthreads();
            if (t0 == 0) {
#pragma unroll
                for (int j = 0; j < kGeoStage; ++j) {
                    if (src[j] == -2) continue;
                    const int i = tid + j * kThreads, p = i >> 2, q = i & 3;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (src[j] >= 0) v = *(const float4*)(in + (size_t)(g * 81 + src[j]) * inStride + ch * 16 + q * 4);
                    float* d = sIn + p * kInStride + q * 4;
                    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                }
            }
            for (int i = tid; i < n * 16 * 16; i += kThreads) {
                const int row = i >> 4, q = i & 15;
                *(float4*)(sW + row * kWStride + q * 4) = *(const float4*)(wc + (size_t)(t0 * 16 + row) * 64 + q * 4);
            }
            __syncthreads();
            for (int t = 0; t < n; ++t) {
                const int off = (ky * dh * W + kx * dw) * kInStride;
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    const int k = k4 * 4 + kq;
                    const float b = sW[(t * 16 + k) * kWStride + wave * 16 + col];
#pragma unroll
                    for (int f = 0; f < 6; ++f) {
                        const float a = sIn[aBase[f] + off + k4 * 4];
                        acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[f], 0, 0, 0);
                    }
                }
                if (++kx == kw) { kx = 0; ++ky; }
            }
        }
    }
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

// ---- depthwise ---------------------------------------------------------------------------------------------------
constexpr int kDwStride = 20; // LDS floats per position: 16 channels + 4, so that a thread's 16-byte read stays aligned

__global__ __launch_bounds__(kThreads) void graphDepthwise(const float* __restrict__ in, int inStride,
                                                           const float* __restrict__ w, const float* __restrict__ bias,
                                                           const float* __restrict__ res, int resStride, int resOff,
                                                           float* __restrict__ out, int outStride, int C, int act,
                                                           int kh, int kw, int dh, int dw) {
    __shared__ __attribute__((aligned(16))) float sIn[kGeoPos * kDwStride];
    __shared__ __attribute__((aligned(16))) float sW[81 * 16];
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const int chunks = outStride / 16, taps = kh * kw;
    const int hy = dh * (kh - 1) / 2, hx = dw * (kw - 1) / 2, W = 9 + 2 * hx;
    const bool resVec = res && ((resStride | resOff) & 3) == 0;
    int src[kGeoStage];
#pragma unroll
    for (int j = 0; j < kGeoStage; ++j) src[j] = imageSource(tid + j * kThreads, hy, hx);

    for (int ch = 0; ch < chunks; ++ch) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kGeoStage; ++j) {
            if (src[j] == -2) continue;
            const int i = tid + j * kThreads, p = i >> 2, q = i & 3;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (src[j] >= 0) v = *(const float4*)(in + (size_t)(g * 81 + src[j]) * inStride + ch * 16 + q * 4);
            *(float4*)(sIn + p * kDwStride + q * 4) = v;
        }
        for (int i = tid; i < taps * 4; i += kThreads)
            *(float4*)(sW + i * 4) = *(const float4*)(w + (size_t)ch * taps * 16 + i * 4);
        __syncthreads();
        for (int i = tid; i < 81 * 4; i += kThreads) {
            const int sq = i >> 2, q = i & 3;
            const float* a = sIn + ((sq / 9) * W + sq % 9) * kDwStride + q * 4;
            const float* b = sW + q * 4;
            float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx) {
                    const float4 x = *(const float4*)(a + (ky * dh * W + kx * dw) * kDwStride);
                    const float4 t = *(const float4*)(b + (ky * kw + kx) * 16);
                    s.x = fmaf(x.x, t.x, s.x); s.y = fmaf(x.y, t.y, s.y);
                    s.z = fmaf(x.z, t.z, s.z); s.w = fmaf(x.w, t.w, s.w);
                }
            const int c0 = ch * 16 + q * 4;
            const size_t row = (size_t)g * 81 + sq;
            const float4 bc = *(const float4*)(bias + c0);
            float v[4] = {s.x + bc.x, s.y + bc.y, s.z + bc.z, s.w + bc.w};
            if (resVec) {
                const float4 r = *(const float4*)(res + row * resStride + resOff + c0);
                v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
            } else if (res) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c0 + j < C) v[j] += res[row * resStride + resOff + c0 + j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = c0 + j < C ? applyAct(v[j], act) : 0.f;
            *(float4*)(out + row * outStride + c0) = make_float4(v[0], v[1], v[2], v[3]);
        }
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

static bool geometryOk(int kh, int kw, int dh, int dw) {
    return kh >= 1 && kw >= 1 && kh <= 9 && kw <= 9 && (kh & 1) && (kw & 1) && dh >= 1 && dw >= 1 &&
           dh * (kh - 1) / 2 <= kMaxConvHalo && dw * (kw - 1) / 2 <= kMaxConvHalo;
}

hipError_t launchGraphConvGeo(const float* in, int inStride, const float* w, const float* bias, DevView res,
                              float* out, int outStride, int cout, int cinPad, int coutTiles, int kh, int kw, int dh,
                              int dw, int boards, int act, hipStream_t stream) {
    if (boards <= 0 || cinPad % 16 != 0 || inStride % 4 != 0 || inStride < cinPad || coutTiles * 64 < cout ||
        !geometryOk(kh, kw, dh, dw))
        return hipErrorInvalidValue;
    // the fewest groups of at most kGeoTapGroup taps, evened out: 25 taps go as 7 + 7 + 7 + 4, not 8 + 8 + 8 + 1
    const int taps = kh * kw, groups = (taps + kGeoTapGroup - 1) / kGeoTapGroup;
    const int tapGroup = (taps + groups - 1) / groups;
    hipLaunchKernelGGL(graphConvGeo, dim3((unsigned)boards, (unsigned)coutTiles), dim3(kThreads), 0, stream, in,
                       inStride, w, bias, res.p, res.stride, res.offset, out, outStride, cout, cinPad,
                       (long)boards * 81, act, kh, kw, dh, dw, tapGroup);
    return hipGetLastError();
}

hipError_t launchGraphDepthwise(const float* in, int inStride, const float* w, const float* bias, DevView res,
                                float* out, int outStride, int C, int kh, int kw, int dh, int dw, int boards, int act,
                                hipStream_t stream) {
    if (boards <= 0 || outStride % 16 != 0 || inStride % 4 != 0 || inStride < outStride || outStride < C ||
        outStride - C >= 16 || !geometryOk(kh, kw, dh, dw))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(graphDepthwise, dim3((unsigned)boards), dim3(kThreads), 0, stream, in, inStride, w, bias, res.p,
                       res.stride, res.offset, out, outStride, C, act, kh, kw, dh, dw);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
