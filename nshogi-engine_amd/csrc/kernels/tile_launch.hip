// tile_launch.hip -- host side of the MFMA tile kernels: precision dispatch, the small
// value-output kernel and the legal-move gather (the weights are packed by net_prepare.cc).
#include "mfma_tile.h"

#include <algorithm>
#include <cmath>
#include <stdlib.h>
#include <string.h>

namespace nsg {

ConvTuning readConvTuning() {
    ConvTuning t;
    if (const char* e = getenv("NSG_CONV_NB")) t.nb = atoi(e);
    if (const char* e = getenv("NSG_CONV_NWAVES")) t.nwaves = atoi(e);
    if (const char* e = getenv("NSG_CONV_NFRAG")) t.nfrag = atoi(e);
    if (const char* e = getenv("NSG_CONV_MSPLIT")) t.msplit = atoi(e);
    if (const char* e = getenv("NSG_ROWSPLIT8_MAX_BATCH")) t.rowsplit8Max = atoi(e);
    if (const char* e = getenv("NSG_SPLIT_BATCH")) t.splitBatch = atoi(e);
    if (const char* e = getenv("NSG_SPLIT_BATCH_MAX")) t.splitBatchMax3 = atoi(e);
    if (const char* e = getenv("NSG_SLAB_SPLIT")) t.slabSplit = atoi(e);
    if (const char* e = getenv("NSG_KSPLIT3")) t.ksplit3 = atoi(e);
    return t;
}

hipError_t launchConv3x3(const void* x, const void* wfrag, const float* bias,
                         const void* residual, void* y, int batch, int cin,
                         int cout, int relu, float accScale, int prec,
                         const ConvPlan& plan, hipStream_t stream,
                         unsigned long long* stamps, bool outF16x3) {
    if (batch <= 0 || cin % inputChannelGranule(prec) != 0 || cout % 64 != 0)
        return hipErrorInvalidValue;
    tile::Args a{};
    a.x = (const unsigned char*)x;
    a.w = (const tile::u32x4*)wfrag;
    a.bias = bias;
    a.res = (const unsigned char*)residual;
    a.y = (unsigned char*)y;
    a.kdim = cin;
    a.cout = cout;
    a.totalRows = batch * 81;
    a.relu = relu;
    a.accScale = accScale;
    a.stamps = stamps;
    a.outF16x3 = outF16x3 ? 1 : 0;
    switch (prec) {
    case kF16m8: return tile::launchConvF16m8(a, batch, plan, stream);
    case kF16m6: return tile::launchConvF16m6(a, batch, plan, stream);
    case kFp32: return tile::launchConvFp32(a, batch, plan, stream);
    case kFp16: return tile::launchConvFp16(a, batch, plan, stream);
    case kBf16: return tile::launchConvBf16(a, batch, plan, stream);
    case kF16x3: return tile::launchConvF16x3(a, batch, plan, stream);
    }
    return hipErrorInvalidValue;
}

size_t trunkLayerBytes() { return sizeof(tile::Args); }
size_t trunkLayerStampsOffset() { return offsetof(tile::Args, stamps); }

void fillTrunkLayer(void* hostLayers, int index, const void* x, const void* wfrag,
                    const float* bias, const void* residual, void* y, int cin,
                    int cout, int relu, float accScale, bool outF16x3) {
    tile::Args a{};
    a.outF16x3 = outF16x3 ? 1 : 0;
    a.x = (const unsigned char*)x;
    a.w = (const tile::u32x4*)wfrag;
    a.bias = bias;
    a.res = (const unsigned char*)residual;
    a.y = (unsigned char*)y;
    a.kdim = cin;
    a.cout = cout;
    a.relu = relu;
    a.accScale = accScale;
    memcpy((unsigned char*)hostLayers + (size_t)index * sizeof(tile::Args), &a, sizeof(a));
}

hipError_t launchTrunk(const void* devLayers, int nLayers, int batch, int prec,
                       const ConvPlan& plan, hipStream_t stream) {
    if (batch <= 0 || nLayers <= 0) return hipErrorInvalidValue;
    const tile::Args* L = (const tile::Args*)devLayers;
    switch (prec) {
    case kFp32: return tile::launchTrunkFp32(L, nLayers, batch, plan, stream);
    case kFp16: return tile::launchTrunkFp16(L, nLayers, batch, plan, stream);
    case kBf16: return tile::launchTrunkBf16(L, nLayers, batch, plan, stream);
    case kF16x3: return tile::launchTrunkF16x3(L, nLayers, batch, plan, stream);
    case kF16m8: return tile::launchTrunkF16m8(L, nLayers, batch, plan, stream);
    case kF16m6: return tile::launchTrunkF16m6(L, nLayers, batch, plan, stream);
    }
    return hipErrorInvalidValue;
}

bool coopSameXcd() { return tile::kCoopSameXcd; }

hipError_t launchCoopTrunk(const void* devLayers, int nLayers, int batch, int cout, int prec, const ConvPlan& plan,
                           unsigned* flags, unsigned flagBase, int* status, hipStream_t stream, int faultBoard) {
    if (batch <= 0 || nLayers <= 0 || !flags || !status || prec != kF16m6 || flagBase + (unsigned)nLayers + 1 >= (1u << 24))
        return hipErrorInvalidValue;
    return tile::launchCoopTrunkF16m6((const tile::Args*)devLayers, nLayers, batch, cout, plan, flags, flagBase, status, stream, faultBoard);
}

hipError_t launchHeads(const void* x, const void* wfrag, const float* bias,
                       float* policy, void* vfeat, int batch, int channels,
                       int coutPadded, int valueChannels, int vfeatStride,
                       float accScale, int prec, hipStream_t stream) {
    if (batch <= 0 || (channels * elemSize(prec)) % 128 != 0 || coutPadded % 64 != 0 ||
        valueChannels + 27 > coutPadded || vfeatStride < 81 * valueChannels)
        return hipErrorInvalidValue;
    tile::Args a{};
    a.x = (const unsigned char*)x;
    a.w = (const tile::u32x4*)wfrag;
    a.bias = bias;
    a.policy = policy;
    a.vfeat = (unsigned char*)vfeat;
    a.kdim = channels;
    a.cout = coutPadded;
    a.totalRows = batch * 81;
    a.valueChannels = valueChannels;
    a.vfeatStride = vfeatStride;
    a.accScale = accScale;
    switch (prec) {
    case kFp32: return tile::launchHeadsFp32(a, stream);
    case kFp16: return tile::launchHeadsFp16(a, stream);
    case kBf16: return tile::launchHeadsBf16(a, stream);
    case kF16x3: return tile::launchHeadsF16x3(a, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launchDense(const void* x, const void* wfrag, const float* bias,
                       float* y, int rows, int kdim, int cout, size_t partStride,
                       float accScale, int prec, hipStream_t stream) {
    if (rows <= 0 || (kdim * elemSize(prec)) % 128 != 0 || cout % 64 != 0)
        return hipErrorInvalidValue;
    tile::Args a{};
    a.x = (const unsigned char*)x;
    a.w = (const tile::u32x4*)wfrag;
    a.bias = bias;
    a.y = (unsigned char*)y;
    a.kdim = kdim;
    a.cout = cout;
    a.totalRows = rows;
    a.relu = 0;
    a.accScale = accScale;
    a.kSplits = denseSplits(kdim, prec);
    a.partStride = partStride;
    switch (prec) {
    case kFp32: return tile::launchDenseFp32(a, stream);
    case kFp16: return tile::launchDenseFp16(a, stream);
    case kBf16: return tile::launchDenseBf16(a, stream);
    case kF16x3: return tile::launchDenseF16x3(a, stream);
    }
    return hipErrorInvalidValue;
}

// ---------------------------------------------------------------------------
// Value MLP layer 2: one wave per board, 64-lane shuffle reduction.
// ---------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void valueOutKernel(
    const float* __restrict__ h, const float* __restrict__ b1, int nsplit, size_t partStride,
    const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ value,
    float* __restrict__ draw, int batch, int hidden) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    float s0 = 0.f, s1 = 0.f;
    for (int j = lane; j < hidden; j += 64) {
        // layer 1: the K splits' partial sums in a fixed order, + bias, ReLU (all slices
        // requested before the first is added: one memory round trip, not nsplit)
        float part[9];
#pragma unroll
        for (int z = 0; z < 9; ++z) part[z] = z < nsplit ? h[(size_t)z * partStride + (size_t)b * hidden + j] : 0.f;
        float hv = b1[j];
#pragma unroll
        for (int z = 0; z < 9; ++z) hv += part[z];
        hv = fmaxf(hv, 0.f);
        s0 = fmaf(hv, w2[j], s0);
        s1 = fmaf(hv, w2[hidden + j], s1);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s0 += __shfl_xor(s0, off);
        s1 += __shfl_xor(s1, off);
    }
    if (lane == 0) {
        const float o0 = s0 + b2[0];
        const float o1 = s1 + b2[1];
        value[b] = 0.5f * (tanhf(o0) + 1.0f);
        draw[b] = 1.0f / (1.0f + expf(-o1));
    }
}
} // namespace

hipError_t launchValueOut(const float* h, const float* b1, int nsplit, size_t partStride,
                          const float* w2, const float* b2,
                          float* value, float* draw, int batch, int hidden,
                          hipStream_t stream) {
    if (batch <= 0 || nsplit < 1 || nsplit > 9) return hipErrorInvalidValue;
    hipLaunchKernelGGL(valueOutKernel, dim3((batch + 3) / 4), dim3(256), 0, stream,
                       h, b1, nsplit, partStride, w2, b2, value, draw, batch, hidden);
    return hipGetLastError();
}

namespace {
__global__ __launch_bounds__(256) void gatherLogitsKernel(
    const float* __restrict__ policy, const uint16_t* __restrict__ idx,
    const uint32_t* __restrict__ offsets, float* __restrict__ out, int batch, int softmax) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= batch) return;
    const uint32_t lo = offsets[b], hi = offsets[b + 1];
    const float* row = policy + (size_t)b * 2187;
    if (!softmax) {
        for (uint32_t i = lo + lane; i < hi; i += 64) out[i] = row[idx[i] < 2187 ? idx[i] : 0];
        return;
    }
    // softmax(T=1) over this position's moves: max, sum of exp, normalise (f32, like the host's)
    float m = -INFINITY;
    for (uint32_t i = lo + lane; i < hi; i += 64) m = fmaxf(m, row[idx[i] < 2187 ? idx[i] : 0]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    float sum = 0.f;
    for (uint32_t i = lo + lane; i < hi; i += 64) {
        const float e = expf(row[idx[i] < 2187 ? idx[i] : 0] - m);
        out[i] = e;
        sum += e;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    const float inv = 1.0f / sum;
    for (uint32_t i = lo + lane; i < hi; i += 64) out[i] *= inv;
}
} // namespace

hipError_t launchGatherLogits(const float* policy, const uint16_t* idx, const uint32_t* offsets,
                              float* out, int batch, int softmax, hipStream_t stream) {
    if (batch <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gatherLogitsKernel, dim3((batch + 3) / 4), dim3(256), 0, stream,
                       policy, idx, offsets, out, batch, softmax);
    return hipGetLastError();
}

} // namespace nsg
