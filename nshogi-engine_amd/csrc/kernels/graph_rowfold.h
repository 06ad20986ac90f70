// graph_rowfold.h -- the fold over the C contiguous floats at channel `offset` of a row by a group of 16 lanes: the one
// definition of the lane split and of the order of every add that graph_chanreduce.hip (kLaunchChanReduce) and
// graph_normalize.hip (kLaunchNormalize) share, so that a norm computed inside the fused normalise launch has the bits
// of the stand-alone reduction.  Device code only.
//
// The row's range [offset, offset + C) is cut, by (C, offset) alone, into
//   head   the 0..3 elements in front of the first 16-byte boundary    lane l < head reads element l          (scalar loads)
//   body   (C - head) / 4 float4s                                     lane l reads float4s l, l + 16, ...   (16-byte loads)
//   tail   the (C - head) % 4 elements behind the last float4         lane l < tail reads element l of them (scalar loads)
// Each lane takes its elements into one accumulator in that order (head, body ascending with x y z w of each float4 in
// turn, tail), starting from the fold's identity, and the sixteen accumulators meet in a butterfly over lane distances
// 8, 4, 2, 1 (__shfl_xor inside the group of 16).  Nothing outside [offset, offset + C) is read.
#ifndef NSG_GRAPH_ROWFOLD_H
#define NSG_GRAPH_ROWFOLD_H

#include "graph_kernels.h"

namespace nsg {
namespace graph {

constexpr int kRowGroup = 16; // lanes per row

// What a lane does with one element: the RedModes that are one pass (kRedMax, kRedMin, kRedSum, kRedL1, kRedSumSq), and
// the second pass of a log-sum-exp, acc + expf(x - m) with m the row's max.
constexpr int kFoldExpSum = 64;

template <int Fold> __device__ __forceinline__ float foldIdentity() {
    return Fold == kRedMax ? -INFINITY : Fold == kRedMin ? INFINITY : 0.f;
}
template <int Fold> __device__ __forceinline__ float foldTake(float acc, float x, float m) {
    if (Fold == kRedMax) return fmaxf(acc, x);
    if (Fold == kRedMin) return fminf(acc, x);
    if (Fold == kRedL1) return acc + fabsf(x);
    if (Fold == kRedSumSq) return fmaf(x, x, acc);
    if (Fold == kFoldExpSum) return acc + expf(x - m);
    return acc + x;
}
// two lanes' accumulators in the butterfly
template <int Fold> __device__ __forceinline__ float foldMeet(float a, float b) {
    return Fold == kRedMax ? fmaxf(a, b) : Fold == kRedMin ? fminf(a, b) : a + b;
}

// The fold of the row at p = row + offset (inOff: that offset, for the alignment of the body), every lane of the group
// returning the result.  A group that is not `live` loads nothing but stays in the wave's shuffles.  m: kFoldExpSum's max.
template <int Fold>
__device__ __forceinline__ float rowFold(const float* __restrict__ p, int inOff, int C, int lane, bool live, float m = 0.f) {
    float acc = foldIdentity<Fold>();
    if (live) {
        const int lead = (4 - (inOff & 3)) & 3;
        const int head = lead < C ? lead : C;
        const int body = (C - head) >> 2, tail = (C - head) & 3;
        if (lane < head) acc = foldTake<Fold>(acc, p[lane], m);
        const float4* q = reinterpret_cast<const float4*>(p + head); // 16-byte aligned: rows are, and inOff + head is a multiple of 4
        for (int i = lane; i < body; i += kRowGroup) {
            const float4 v = q[i];
            acc = foldTake<Fold>(foldTake<Fold>(foldTake<Fold>(foldTake<Fold>(acc, v.x, m), v.y, m), v.z, m), v.w, m);
        }
        if (lane < tail) acc = foldTake<Fold>(acc, p[head + 4 * body + lane], m);
    }
    for (int d = kRowGroup / 2; d > 0; d >>= 1) acc = foldMeet<Fold>(acc, __shfl_xor(acc, d, kRowGroup));
    return acc;
}

} // namespace graph
} // namespace nsg

#endif
