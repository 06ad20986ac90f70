// graph_bmm.hip -- the general graph path's product of two run-time token tensors, exact f32 on the MFMA
// (v_mfma_f32_16x16x4_f32), in the style of graphAttention's two products.
//
// graphBmmNT: out[n,i,j] = act(scale * sum_k A[n,i,k] B[n,j,k]), A and B token views [N,81,K], out [N,81,81] at stride
// 96.  One workgroup of four waves per board.  Per 16-channel chunk A's and B's 81 rows are staged in LDS as 96-row
// images (rows 81..95 zero, channels past K zero), and the 36 output fragments go nine to a wave, four k-steps each.
//
// graphBmmNN: out[n,i,c] = act(scale * sum_j P[n,i,j] V[n,j,c]), P a token view [N,81,81], V a token view [N,81,M].
// A workgroup owns one board and 64 output channels; P is staged whole (96 rows, keys 81..83 zero), V's 64 channels
// beside it (rows 81..83 zero); a wave takes 16 channels and all six row fragments, as graphConv's waves do, over 21
// k-steps.
//
// The order contract.  An output element is one f32 chain over k ascending: chunk by chunk and four k-steps per chunk
// (NT), 21 k-steps (NN), every step one MFMA into the same accumulator.  No atomics and no split over k.  The chain
// depends on (K, M) only -- a partial last chunk adds exact zeros -- and never on the batch, the grid or a view's offset.
// Then the sum is multiplied by `scale` (one rounding) and goes through applyAct.
//
// A board reads its own 81 rows and nothing else: rows 81..95 of an image are written as zeros, never loaded (the last
// board of a batch has nothing behind it, and a neighbour's inf times a pad 0 would be NaN), and a view's channels past
// K are replaced by zeros with a select, not a product.  Output rows 81..95 are computed and never stored; output pad
// channels are stored as zeros, not as what the pad columns computed, and never go through applyAct.
#include "graph_act.h"
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kRows = 96;    // 81 squares rounded up to six 16-row fragments
constexpr int kKS = 20;      // NT: LDS floats per 16-channel row, 4 x odd: sixteen rows x four k lanes on 64 distinct banks
constexpr int kPS = 100;     // NN: LDS floats per row of P (84 keys used), the same property
constexpr int kVS = 80;      // NN: LDS floats per row of V's 64 channels: the four key rows of a step on distinct banks
constexpr int kKeys = 84;    // NN: 21 k-steps

// the float4 at p with the elements from `valid` on replaced by zeros (valid >= 1)
__device__ inline float4 loadMasked(const float* p, int valid) {
    float4 x = *(const float4*)p;
    if (valid < 2) x.y = 0.f;
    if (valid < 3) x.z = 0.f;
    if (valid < 4) x.w = 0.f;
    return x;
}

__global__ __launch_bounds__(kThreads) void graphBmmNT(const float* __restrict__ a, int aStride, int aOff,
                                                       const float* __restrict__ b, int bStride, int bOff, int K,
                                                       float scale, int act, float* __restrict__ out, int outStride) {
    __shared__ __attribute__((aligned(16))) float sA[kRows * kKS];
    __shared__ __attribute__((aligned(16))) float sB[kRows * kKS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4, col = lane & 15;
    const long board = blockIdx.x;
    const float* ab = a + (size_t)board * 81 * aStride + aOff;
    const float* bb = b + (size_t)board * 81 * bStride + bOff;

    for (int i = tid; i < (kRows - 81) * kKS; i += kThreads) {
        sA[81 * kKS + i] = 0.f;
        sB[81 * kKS + i] = 0.f;
    }
    // the fragments of this wave: ids wave * 9 .. wave * 9 + 8, row fragment id / 6, column fragment id % 6
    int aRow[9], bRow[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int id = wave * 9 + j, rf = id / 6, cf = id - rf * 6;
        aRow[j] = (rf * 16 + col) * kKS + kq;
        bRow[j] = (cf * 16 + col) * kKS + kq;
    }
    f32x4 acc[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int chunks = (K + 15) / 16;
    for (int ch = 0; ch < chunks; ++ch) {
        __syncthreads(); // the previous chunk is read (first pass: nothing to wait for but the zero rows' writers)
        for (int i = tid; i < 81 * 4; i += kThreads) {
            const int r = i >> 2, k0 = ch * 16 + (i & 3) * 4;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
            if (k0 < K) {
                x = loadMasked(ab + (size_t)r * aStride + k0, K - k0);
                y = loadMasked(bb + (size_t)r * bStride + k0, K - k0);
            }
            *(float4*)(sA + r * kKS + (i & 3) * 4) = x;
            *(float4*)(sB + r * kKS + (i & 3) * 4) = y;
        }
        __syncthreads();
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
            for (int j = 0; j < 9; ++j)
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(sA[aRow[j] + k4 * 4], sB[bRow[j] + k4 * 4], acc[j], 0, 0, 0);
    }
    // acc[j][i] = sum[row rf*16 + 4*kq + i][column cf*16 + col]
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const int id = wave * 9 + j, rf = id / 6, cf = id - rf * 6;
        const int c = cf * 16 + col;
        if (c >= outStride) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rf * 16 + 4 * kq + i;
            if (r >= 81) continue;
            out[(size_t)(board * 81 + r) * outStride + c] = c < 81 ? applyAct(acc[j][i] * scale, act) : 0.f;
        }
    }
}

__global__ __launch_bounds__(kThreads) void graphBmmNN(const float* __restrict__ p, int pStride, int pOff,
                                                       const float* __restrict__ v, int vStride, int vOff, int M,
                                                       float scale, int act, float* __restrict__ out, int outStride) {
    __shared__ __attribute__((aligned(16))) float sP[kRows * kPS];
    __shared__ __attribute__((aligned(16))) float sV[kKeys * kVS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4, col = lane & 15;
    const long board = blockIdx.x;
    const int c0 = blockIdx.y * 64;
    const float* pb = p + (size_t)board * 81 * pStride + pOff;
    const float* vb = v + (size_t)board * 81 * vStride + vOff;

    // P: rows 81..95 and keys 81..83 zero
    for (int i = tid; i < kRows * (kKeys / 4); i += kThreads) {
        const int r = i / (kKeys / 4), k0 = (i - r * (kKeys / 4)) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < 81) x = loadMasked(pb + (size_t)r * pStride + k0, 81 - k0);
        *(float4*)(sP + r * kPS + k0) = x;
    }
    // V: this workgroup's 64 channels, rows 81..83 and channels from M on zero
    for (int i = tid; i < kKeys * 16; i += kThreads) {
        const int r = i >> 4, c = c0 + (i & 15) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < 81 && c < M) x = loadMasked(vb + (size_t)r * vStride + c, M - c);
        *(float4*)(sV + r * kVS + (i & 15) * 4) = x;
    }
    __syncthreads();
    const int cl = c0 + wave * 16 + col;
    if (c0 + wave * 16 >= outStride) return; // a whole wave past the row: nothing to store, no barrier follows

    f32x4 acc[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* pr = sP + col * kPS + kq;
    const float* vr = sV + kq * kVS + wave * 16 + col;
#pragma unroll
    for (int k4 = 0; k4 < kKeys / 4; ++k4) {
        const float bv = vr[k4 * 4 * kVS];
#pragma unroll
        for (int f = 0; f < 6; ++f)
            acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[f * 16 * kPS + k4 * 4], bv, acc[f], 0, 0, 0);
    }
    // acc[f][i] = sum[row f*16 + 4*kq + i][channel cl]
    if (cl >= outStride) return;
#pragma unroll
    for (int f = 0; f < 6; ++f)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = f * 16 + 4 * kq + i;
            if (r >= 81) continue;
            out[(size_t)(board * 81 + r) * outStride + cl] = cl < M ? applyAct(acc[f][i] * scale, act) : 0.f;
        }
}

bool viewOk(const DevView& x) {
    return x.p && x.C >= 1 && x.offset >= 0 && x.offset % 4 == 0 && x.stride % 4 == 0 && x.offset + x.C <= x.stride;
}

} // namespace

hipError_t launchGraphBmmNT(DevView a, DevView b, float scale, int act, float* out, int outStride, int boards,
                            hipStream_t stream) {
    if (boards <= 0 || !viewOk(a) || !viewOk(b) || a.C != b.C || outStride != kRows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(graphBmmNT, dim3((unsigned)boards), dim3(kThreads), 0, stream, a.p, a.stride, a.offset, b.p, b.stride,
                       b.offset, a.C, scale, act, out, outStride);
    return hipGetLastError();
}

hipError_t launchGraphBmmNN(DevView p, DevView v, float scale, int act, float* out, int outStride, int boards,
                            hipStream_t stream) {
    if (boards <= 0 || !viewOk(p) || !viewOk(v) || p.C != 81 || outStride % kChunk != 0 || outStride < v.C || outStride - v.C >= kChunk)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(graphBmmNN, dim3((unsigned)boards, (unsigned)((outStride + 63) / 64)), dim3(kThreads), 0, stream, p.p,
                       p.stride, p.offset, v.p, v.stride, v.offset, v.C, scale, act, out, outStride);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
