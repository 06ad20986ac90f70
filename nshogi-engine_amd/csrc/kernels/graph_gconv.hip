// graph_gconv.hip -- the general graph path's grouped convolution (1 < group < Cin), exact f32 on the MFMA.
//
// graphConvGeo's work split and order (graph_conv.hip): a workgroup owns one board and 64 output channels, its four
// waves 16 channels each and all six 16-row fragments; per 16-channel input chunk the board is staged in LDS as a haloed
// image of up to 17 x 17 positions beside the chunk's weights in groups of at most 8 taps, and every tap runs four
// k-steps of v_mfma_f32_16x16x4_f32 per fragment.  The geometry (kh x kw taps, dilations) is a set of launch arguments.
//
// What is new is the k range.  The 64 outputs of a tile belong to a few groups, and those groups read a few input
// channels: the tile's chunk range is the 16-channel chunks that intersect them, and each wave has a sub-range of it
// for its own 16 outputs (the planner's packGrouped builds both, one row of kGroupTabInts ints per tile).  The
// workgroup stages only the chunks of the tile's range; a wave issues MFMAs only for the chunks of its sub-range -- the
// test is wave-uniform, and every wave still takes part in every barrier.  The packed weights are [tile][chunk of the
// tile's range][tap][16][64] with exact zeros where input and output channel lie in different groups, so weight bytes
// and MFMA count are about 1 / group of the dense conv's, rounded up to chunks.
//
// Order: an output element is one f32 chain -- chunks ascending, taps row-major over (ky, kx), the four k-steps of a
// chunk ascending -- that is graphConv's chain restricted to the group's chunks.  No split-K, no atomics, nothing
// depends on the batch or the grid.  A zero weight inside a shared chunk adds an exact 0 to a finite chain.
// Isolation, at chunk granularity: a wave never reads a chunk outside its sub-range into an MFMA, so a non-finite value
// in a channel of another group that shares no chunk with the wave's inputs cannot reach its outputs; inside a shared
// chunk 0 * inf is NaN, as in every dense kernel here.
#include "graph_act.h"
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kInStride = 17; // LDS floats per position: 16 channels + 1 (consecutive rows fall on distinct banks)
constexpr int kWStride = 80;  // LDS floats per (tap, k) row of 64 outputs: the four k rows of a step on distinct banks
constexpr int kSide = 9 + 2 * kMaxConvHalo;
constexpr int kPos = kSide * kSide; // 17 x 17 positions: 19 652 B at kInStride floats each
constexpr int kTapGroup = 8;        // taps of weights in LDS at a time: 8 x 5 120 B beside the image, under 64 KB
constexpr int kStage = (kPos * 4 + kThreads - 1) / kThreads; // 16-byte pieces of the image a thread stages

// What the float4 piece i of the haloed image shows: a square of the board (0..80), -1 in the halo, -2 past the image
__device__ inline int imageSource(int i, int hy, int hx) {
    const int W = 9 + 2 * hx, p = i >> 2;
    if (p >= (9 + 2 * hy) * W) return -2;
    const int y = p / W - hy, x = p % W - hx;
    return y >= 0 && y < 9 && x >= 0 && x < 9 ? y * 9 + x : -1;
}

__global__ __launch_bounds__(kThreads) void graphConvGrouped(const float* __restrict__ in, int inStride,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const int* __restrict__ tables,
                                                             const float* __restrict__ res, int resStride, int resOff,
                                                             float* __restrict__ out, int outStride, int cout,
                                                             long rows, int act, int kh, int kw, int dh, int dw,
                                                             int tapGroup) {
    __shared__ float sIn[kPos * kInStride];
    __shared__ __attribute__((aligned(16))) float sW[kTapGroup * 16 * kWStride];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long g = blockIdx.x;
    const int tile = blockIdx.y;
    const int taps = kh * kw;
    const int hy = dh * (kh - 1) / 2, hx = dw * (kw - 1) / 2, W = 9 + 2 * hx;
    // the tile's chunk range, clamped to the chunks the input's rows hold: nothing is read past a row
    const int* tab = tables + tile * kGroupTabInts;
    const int first = max(tab[0], 0), count = min(tab[1], inStride / 16 - first);
    const float* wt = w + (size_t)tab[2];
    const int myFirst = tab[4 + 2 * wave], myEnd = myFirst + tab[5 + 2 * wave]; // the wave's sub-range
    const int kq = lane >> 4, col = lane & 15;
    // a row's square sits at (y + hy, x + hx) of the image and tap (ky, kx) reads (y + ky dh, x + kx dw)
    int aBase[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int r = min(f * 16 + col, 80);
        aBase[f] = ((r / 9) * W + r % 9) * kInStride + kq;
    }
    int src[kStage];
#pragma unroll
    for (int j = 0; j < kStage; ++j) src[j] = imageSource(tid + j * kThreads, hy, hx);
    f32x4 acc[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) acc[f] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ci = 0; ci < count; ++ci) {
        const int ch = first + ci;
        const bool mine = ch >= myFirst && ch < myEnd; // wave-uniform
        const float* wc = wt + (size_t)ci * taps * 16 * 64;
        int ky = 0, kx = 0;
        for (int t0 = 0; t0 < taps; t0 += tapGroup) {
            const int n = min(tapGroup, taps - t0);
            __syncthreads();
            if (t0 == 0) {
#pragma unroll
                for (int j = 0; j < kStage; ++j) {
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
            if (mine) {
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

hipError_t launchGraphConvGrouped(const float* in, int inStride, const float* w, const float* bias, const int* tables,
                                  DevView res, float* out, int outStride, int cout, int kh, int kw, int dh, int dw,
                                  int boards, int act, hipStream_t stream) {
    const bool geometry = kh >= 1 && kw >= 1 && kh <= 9 && kw <= 9 && (kh & 1) && (kw & 1) && dh >= 1 && dw >= 1 &&
                          dh * (kh - 1) / 2 <= kMaxConvHalo && dw * (kw - 1) / 2 <= kMaxConvHalo;
    if (boards <= 0 || cout <= 0 || inStride % 16 != 0 || outStride % 16 != 0 || outStride < cout ||
        outStride > (cout + kCoutTile - 1) / kCoutTile * kCoutTile || !tables || !geometry)
        return hipErrorInvalidValue;
    // the fewest groups of at most kTapGroup taps, evened out, as launchGraphConvGeo does
    const int taps = kh * kw, tapGroups = (taps + kTapGroup - 1) / kTapGroup;
    const int tapGroup = (taps + tapGroups - 1) / tapGroups;
    const int tiles = (cout + kCoutTile - 1) / kCoutTile;
    hipLaunchKernelGGL(graphConvGrouped, dim3((unsigned)boards, (unsigned)tiles), dim3(kThreads), 0, stream, in, inStride,
                       w, bias, tables, res.p, res.stride, res.offset, out, outStride, cout, (long)boards * 81, act, kh, kw,
                       dh, dw, tapGroup);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
