// graph_attention.hip -- the general graph path's attention core and LayerNorm, exact f32.
//
// graphAttention: a workgroup owns one (board, head).  K is staged in LDS as a 96-row image (rows 81..95 zero), Q is
// read from global memory straight into the A operand registers, and S = scale * Q K^T (+ bias) (+ a run-time bias) goes as six by six
// 16 x 16 fragments of v_mfma_f32_16x16x4_f32 into a 96 x 96 score image in LDS.  A row softmax in a fixed order
// follows -- max, expf, sum, divide, one wave per row, keys 81..95 left out of the max and the sum and given
// probability 0 -- while V is staged over K's image; then O = P V on the MFMA, stored as token rows at channels
// h * d .. h * d + d - 1.  Query rows 81..95 are computed and never stored.  No atomics and no split over the keys: a
// board's result is one fixed chain and does not depend on the batch it came with.
//
// graphLayerNorm: one wave per row, two passes (the mean, then the sum of squared deviations), butterfly reductions
// in a fixed order, 1 / sqrtf(var + eps).
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kRows = 96;     // 81 squares rounded up to six 16-row fragments
constexpr int kSStride = 100; // LDS floats per score row: a fragment's four row groups and a row's four k lanes fall on distinct banks

// the same value in every lane, summed / maximised in one fixed order
__device__ inline float waveSum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ inline float waveMax(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// D16: the head dimension d rounded up to 16, in units of 16 (d itself is a multiple of 4, at most 64).
// LDS: (96 x (16 D16 + 4) + 96 x 100) floats = 64512 bytes at D16 = 4, under the 64 KB static limit.
// RT: a bias computed at run time is added to the scores: rt[board * rtBoard + head * rtHead + query * 81 + key], times
// rtScale (rtHead 0: one bias for every head).  Per score: acc * scale, then + bias, then + rtScale * rt.  Without RT
// the arguments are unused and the kernel is the one it was.
template <int D16, bool RT>
__global__ __launch_bounds__(kThreads) void graphAttention(const float* __restrict__ q, int qStride, int qOff,
                                                           const float* __restrict__ k, int kStride, int kOff,
                                                           const float* __restrict__ v, int vStride, int vOff,
                                                           const float* __restrict__ bias, float scale,
                                                           float* __restrict__ out, int outStride, int heads, int d,
                                                           const float* __restrict__ rt, long rtBoard, int rtHead,
                                                           float rtScale) {
    constexpr int DP = 16 * D16;
    constexpr int KS = DP + 4; // floats per K / V row: 4 x odd, so sixteen rows x four k lanes hit 64 distinct banks
    __shared__ __attribute__((aligned(16))) float sKV[kRows * KS];
    __shared__ float sS[kRows * kSStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4, col = lane & 15;
    const long b = blockIdx.x;
    const int h = blockIdx.y;
    const int dq = d >> 2; // k-steps of the score product

    // K image: rows 81..95 and channels d..DP-1 zero
    for (int i = tid; i < kRows * (DP / 4); i += kThreads) {
        const int r = i / (DP / 4), c4 = i - r * (DP / 4);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < 81 && c4 < dq) x = *(const float4*)(k + (size_t)(b * 81 + r) * kStride + kOff + h * d + c4 * 4);
        *(float4*)(sKV + r * KS + c4 * 4) = x;
    }
    __syncthreads();

    // S = scale * Q K^T + bias: 36 fragments, nine per wave; a wave keeps the A operands of its current 16 query rows
    float aQ[4 * D16];
    // The run-time bias of a fragment, four values per lane, is requested one fragment ahead (the first before the loop),
    // behind the Q loads of the iteration that issues it, and used after the next fragment's MFMA chain: a whole
    // iteration -- chain, epilogue and LDS stores -- lies between request and use.  The four loads are unconditional, at
    // addresses clamped to query 80 and key 80 (inside the (board, head) block, so nothing outside it is read), and a
    // select puts 0 where the query or the key is past 80; the 16 lanes of a col group read 16 consecutive floats.
    float rbNext[4] = {0.f, 0.f, 0.f, 0.f};
    const float* rtBase = nullptr;
    if constexpr (RT) rtBase = rt + (size_t)b * (size_t)rtBoard + (size_t)h * (size_t)rtHead;
    auto requestBias = [&](int id) {
        const int rf = id / 6, cf = id - rf * 6;
        const int key = cf * 16 + col;
        const float* rp = rtBase + min(key, 80);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rf * 16 + 4 * kq + i;
            const float x = rp[min(r, 80) * 81];
            rbNext[i] = (r < 81 && key < 81) ? x : 0.f;
        }
    };
    if constexpr (RT) requestBias(wave * 9);
    for (int j = 0; j < 9; ++j) {
        const int id = wave * 9 + j;
        const int rf = id / 6, cf = id - rf * 6;
        if (j == 0 || cf == 0) {
            const int r = rf * 16 + col;
            const float* qr = q + (size_t)(b * 81 + min(r, 80)) * qStride + qOff + h * d;
#pragma unroll
            for (int k4 = 0; k4 < 4 * D16; ++k4) aQ[k4] = (r < 81 && k4 < dq) ? qr[k4 * 4 + kq] : 0.f;
        }
        float rb[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (RT) {
#pragma unroll
            for (int i = 0; i < 4; ++i) rb[i] = rbNext[i];
            if (j + 1 < 9) requestBias(id + 1);
        }
        // acc[i] = S[query rf*16 + 4*kq + i][key cf*16 + col]
        const int key = cf * 16 + col;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* kr = sKV + (cf * 16 + col) * KS + kq;
#pragma unroll
        for (int k4 = 0; k4 < 4 * D16; ++k4)
            if (k4 < dq) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aQ[k4], kr[k4 * 4], acc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rf * 16 + 4 * kq + i;
            float s = acc[i] * scale;
            if (bias && r < 81 && key < 81) s += bias[((size_t)h * 81 + r) * 81 + key];
            if constexpr (RT) s += rtScale * rb[i]; // rb is 0 past query or key 80
            sS[r * kSStride + key] = s;
        }
    }
    __syncthreads(); // every wave is done with K: V takes its place

    for (int i = tid; i < kRows * (DP / 4); i += kThreads) {
        const int r = i / (DP / 4), c4 = i - r * (DP / 4);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < 81 && c4 < dq) x = *(const float4*)(v + (size_t)(b * 81 + r) * vStride + vOff + h * d + c4 * 4);
        *(float4*)(sKV + r * KS + c4 * 4) = x;
    }
    // the softmax of a row over keys 0..80, one wave per row; keys 81..95 get probability 0
    for (int r = wave; r < kRows; r += 4) {
        float* row = sS + r * kSStride;
        const bool two = lane + 64 < 81;
        const float s0 = row[lane], s1 = two ? row[lane + 64] : -INFINITY;
        const float m = waveMax(fmaxf(s0, s1));
        const float e0 = expf(s0 - m), e1 = two ? expf(s1 - m) : 0.f;
        const float sum = waveSum(e0 + e1);
        row[lane] = e0 / sum;
        if (lane + 64 < kRows) row[lane + 64] = two ? e1 / sum : 0.f;
    }
    __syncthreads();

    // O = P V: 6 x D16 fragments; the keys in 21 k-steps (keys 81..83 carry probability 0 and zero V rows)
    for (int id = wave; id < 6 * D16; id += 4) {
        const int rf = id / D16, cf = id - rf * D16;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        const float* pr = sS + (rf * 16 + col) * kSStride + kq;
        const float* vr = sKV + kq * KS + cf * 16 + col;
#pragma unroll
        for (int k4 = 0; k4 < 21; ++k4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[k4 * 4], vr[k4 * 4 * KS], acc, 0, 0, 0);
        const int c = cf * 16 + col;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rf * 16 + 4 * kq + i;
            if (r < 81 && c < d) out[(size_t)(b * 81 + r) * outStride + h * d + c] = acc[i];
        }
    }
    // the channels between heads * d and the row stride are zero, as everywhere on this path
    const int C = heads * d, pad = outStride - C;
    if (h == heads - 1 && pad > 0)
        for (int i = tid; i < 81 * pad; i += kThreads) {
            const int r = i / pad;
            out[(size_t)(b * 81 + r) * outStride + C + (i - r * pad)] = 0.f;
        }
}

__global__ __launch_bounds__(kThreads) void graphLayerNorm(const float* __restrict__ in, int inStride, int inOff, int C,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, float* __restrict__ out, int outStride, long rows) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (row >= rows) return; // whole waves leave: the shuffles below see all 64 lanes
    const float* x = in + (size_t)row * inStride + inOff;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += x[c];
    const float mean = waveSum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float dv = x[c] - mean;
        q += dv * dv;
    }
    const float inv = 1.f / sqrtf(waveSum(q) / (float)C + eps);
    float* y = out + (size_t)row * outStride;
    for (int c = lane; c < outStride; c += 64) y[c] = c < C ? (x[c] - mean) * inv * gamma[c] + beta[c] : 0.f;
}

} // namespace

hipError_t launchGraphAttention(DevView q, DevView k, DevView v, const float* bias, float scale, RtBias rt, float* out,
                                int outStride, int heads, int headDim, int boards, hipStream_t stream) {
    const int C = heads * headDim;
    if (boards <= 0 || heads <= 0 || headDim <= 0 || headDim % 4 != 0 || headDim > kMaxHeadDim || outStride < C)
        return hipErrorInvalidValue;
    for (const DevView* x : {&q, &k, &v})
        if (x->C != C || x->offset % 4 != 0 || x->stride % 4 != 0 || x->offset + C > x->stride) return hipErrorInvalidValue;
    // the last element a workgroup reads, (head heads-1, query 80, key 80), lies inside its board's row
    if (rt.p && (!(rt.scale > 0.f) || rt.headStride < 0 || rt.boardStride <= 0 || (long)(heads - 1) * rt.headStride + 81 * 81 > rt.boardStride))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)boards, (unsigned)heads);
#define NSG_ATT(D16)                                                                                                    \
    do {                                                                                                                \
        if (rt.p)                                                                                                       \
            hipLaunchKernelGGL((graphAttention<D16, true>), grid, dim3(kThreads), 0, stream, q.p, q.stride, q.offset,  \
                               k.p, k.stride, k.offset, v.p, v.stride, v.offset, bias, scale, out, outStride, heads,   \
                               headDim, rt.p, rt.boardStride, rt.headStride, rt.scale);                                \
        else                                                                                                            \
            hipLaunchKernelGGL((graphAttention<D16, false>), grid, dim3(kThreads), 0, stream, q.p, q.stride, q.offset, \
                               k.p, k.stride, k.offset, v.p, v.stride, v.offset, bias, scale, out, outStride, heads,   \
                               headDim, (const float*)nullptr, 0L, 0, 0.f);                                            \
    } while (0)
    switch ((headDim + 15) / 16) {
    case 1: NSG_ATT(1); break;
    case 2: NSG_ATT(2); break;
    case 3: NSG_ATT(3); break;
    default: NSG_ATT(4); break;
    }
#undef NSG_ATT
    return hipGetLastError();
}

hipError_t launchGraphLayerNorm(DevView in, const float* gamma, const float* beta, float eps, float* out,
                                int outStride, long rows, hipStream_t stream) {
    if (rows <= 0 || in.C <= 0 || in.C > outStride || in.offset + in.C > in.stride) return hipErrorInvalidValue;
    const long blocks = (rows + kThreads / 64 - 1) / (kThreads / 64);
    hipLaunchKernelGGL(graphLayerNorm, dim3((unsigned)blocks), dim3(kThreads), 0, stream, in.p, in.stride, in.offset, in.C,
                       gamma, beta, eps, out, outStride, rows);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
