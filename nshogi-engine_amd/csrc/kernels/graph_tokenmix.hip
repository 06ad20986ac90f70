// graph_tokenmix.hip -- the general graph path's Linear over the 81 squares (MLP-Mixer's token MLP, ResMLP's cross-patch
// layer, gMLP's spatial gating projection), exact f32 on the MFMA (v_mfma_f32_16x16x4_f32), with graphBmmNN's work split.
//
//   h[n,d,c]   = act1(sum_s W1^T[d][s] x[n,s,c] + b1[d])      d < D hidden units (one stage: D = 81 and out = h)
//   out[n,j,c] = act2(sum_d W2^T[j][d] h[n,d,c] + b2[j])      j < 81
//
// In board-major rows a product over the squares is a left multiplication of a board's 81 x C block by a constant matrix:
// the constants are the A operand, the board's rows the B operand, and an MFMA column is a channel.  A workgroup owns one
// board and a slab of 64 channels, a wave 16 of them.  The slab's 81 rows are staged once in LDS (rows 81..83 zero) and
// each wave then holds its 16 channels of all 84 squares in 21 registers for the whole launch.
//
// The hidden values never leave the wave.  A stage-1 accumulator of hidden fragment f holds, in lane (kq, col), the units
// f*16 + 4*kq + i (i = 0..3) of channel col -- which is the B-operand layout of the stage-2 k-step that covers the units
// {f*16 + i + 4*q : q = 0..3}.  So each hidden fragment gets its bias and activation and goes straight into four stage-2
// k-steps; the matching A operand is one float4 of W2^T in natural order.  Nothing of h is kept: 4 registers, no LDS.
//
// The order contract.  An element of h is one f32 chain over 21 k-steps (step 4*g + e covers the squares 16*g + 4*q + e,
// g < 5; step 20 the squares 80..83), then + b1[d], then applyAct.  An element of out is one chain over the hidden
// fragments ascending and i = 0..3 within a fragment, then + b2[j], then applyAct.  The chains depend on D only, never on
// the batch, the grid, the slab or the view's offset.  No atomics, no split over k.
//
// A workgroup reads its own board's 81 rows and nothing else: rows 81..83 of the image are written as zeros, never loaded,
// and channels from C on are replaced by zeros with a select.  Zero pads alone would not do (Reciprocal of a pad is inf
// and inf * 0 is NaN): hidden units from D up to the padded count, and every hidden unit of a pad channel, are set to
// zero after the activation; output rows 81..95 are computed and never stored; output channels from C up to the stride
// are stored as zeros, not as what their lanes computed.  Every global load is 16 bytes wide.
#include "graph_act.h"
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kSq = 84;      // 81 squares in 21 k-steps: the row length of W1^T
constexpr int kOutRows = 96; // 81 output squares in six 16-row fragments: the rows of W2^T
constexpr int kXS = 68;      // LDS floats per row of the slab's 64 channels: the four rows of a k-step 16 banks apart

// the float4 at p with the elements from `valid` on replaced by zeros (valid >= 1)
__device__ inline float4 loadMasked(const float* p, int valid) {
    float4 x = *(const float4*)p;
    if (valid < 2) x.y = 0.f;
    if (valid < 3) x.z = 0.f;
    if (valid < 4) x.w = 0.f;
    return x;
}

template <bool Two>
__global__ __launch_bounds__(kThreads) void graphTokenMix(const float* __restrict__ in, int inStride, int inOff, int C,
                                                          const float* __restrict__ consts, int D, int act1, int act2,
                                                          float* __restrict__ out, int outStride) {
    __shared__ __attribute__((aligned(16))) float sX[kSq * kXS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kq = lane >> 4, col = lane & 15;
    const long board = blockIdx.x;
    const int c0 = blockIdx.y * 64;
    const float* xb = in + (size_t)board * 81 * inStride + inOff;

    // the slab: 81 rows of 64 channels, rows 81..83 and channels from C on zero
    for (int i = tid; i < kSq * 16; i += kThreads) {
        const int r = i >> 4, c = c0 + (i & 15) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < 81 && c < C) x = loadMasked(xb + (size_t)r * inStride + c, C - c);
        *(float4*)(sX + r * kXS + (i & 15) * 4) = x;
    }
    __syncthreads();
    if (c0 + wave * 16 >= outStride) return; // a whole wave past the row: nothing to store, no barrier follows
    const int cl = c0 + wave * 16 + col;

    // the B operand of stage 1, for every hidden fragment alike
    float xv[21];
    const float* xr = sX + 4 * kq * kXS + wave * 16 + col;
#pragma unroll
    for (int g = 0; g < 5; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) xv[g * 4 + e] = xr[(16 * g + e) * kXS];
    xv[20] = sX[(80 + kq) * kXS + wave * 16 + col];

    const int Dp = (D + 15) & ~15;
    const float* w1 = consts;
    const float* b1 = w1 + (size_t)Dp * kSq;
    const float* w2 = b1 + Dp;
    const float* b2 = w2 + (size_t)kOutRows * Dp;

    f32x4 acc2[6];
#pragma unroll
    for (int jf = 0; jf < 6; ++jf) acc2[jf] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int f = 0; f < Dp / 16; ++f) {
        // W1^T row f*16 + col: lane kq takes the squares 16*g + 4*kq + e of group g, and square 80 + kq of the last step
        const float* wr = w1 + (size_t)(f * 16 + col) * kSq;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 5; ++g) {
            const float4 a = *(const float4*)(wr + 16 * g + 4 * kq);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, xv[g * 4 + 0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, xv[g * 4 + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, xv[g * 4 + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, xv[g * 4 + 3], acc, 0, 0, 0);
        }
        {
            const float4 a = *(const float4*)(wr + 80);
            const float t = kq == 0 ? a.x : kq == 1 ? a.y : kq == 2 ? a.z : a.w;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(t, xv[20], acc, 0, 0, 0);
        }
        // acc[i] = sum[unit f*16 + 4*kq + i][channel cl]
        const int d0 = f * 16 + 4 * kq;
        const float4 bb = *(const float4*)(b1 + d0);
        float h[4] = {acc[0] + bb.x, acc[1] + bb.y, acc[2] + bb.z, acc[3] + bb.w};
        if (!Two) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (d0 + i < 81) out[(size_t)(board * 81 + d0 + i) * outStride + cl] = cl < C ? applyAct(h[i], act1) : 0.f;
            continue;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) h[i] = d0 + i < D && cl < C ? applyAct(h[i], act1) : 0.f;
        const float* vr = w2 + (size_t)col * Dp + d0;
#pragma unroll
        for (int jf = 0; jf < 6; ++jf) {
            const float4 a = *(const float4*)(vr + (size_t)jf * 16 * Dp);
            acc2[jf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, h[0], acc2[jf], 0, 0, 0);
            acc2[jf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, h[1], acc2[jf], 0, 0, 0);
            acc2[jf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, h[2], acc2[jf], 0, 0, 0);
            acc2[jf] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, h[3], acc2[jf], 0, 0, 0);
        }
    }
    if (!Two) return;
    // acc2[jf][i] = sum[square jf*16 + 4*kq + i][channel cl]
#pragma unroll
    for (int jf = 0; jf < 6; ++jf)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = jf * 16 + 4 * kq + i;
            if (j >= 81) continue;
            out[(size_t)(board * 81 + j) * outStride + cl] = cl < C ? applyAct(acc2[jf][i] + b2[j], act2) : 0.f;
        }
}

} // namespace

hipError_t launchGraphTokenMix(DevView in, const float* consts, int D, int stages, int act1, int act2, float* out,
                               int outStride, int boards, hipStream_t stream) {
    const bool viewOk = in.p && in.C >= 1 && in.offset >= 0 && in.offset % 4 == 0 && in.stride % 4 == 0 && in.offset + in.C <= in.stride;
    if (boards <= 0 || !viewOk || !consts || !out || (stages != 1 && stages != 2) || D < 1 || D > kMaxMixHidden ||
        (stages == 1 && D != 81) || outStride % kChunk != 0 || outStride < in.C || outStride - in.C >= kChunk)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)boards, (unsigned)((outStride + 63) / 64));
    if (stages == 2)
        hipLaunchKernelGGL(graphTokenMix<true>, grid, dim3(kThreads), 0, stream, in.p, in.stride, in.offset, in.C, consts, D,
                           act1, act2, out, outStride);
    else
        hipLaunchKernelGGL(graphTokenMix<false>, grid, dim3(kThreads), 0, stream, in.p, in.stride, in.offset, in.C, consts, D,
                           act1, act2, out, outStride);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
