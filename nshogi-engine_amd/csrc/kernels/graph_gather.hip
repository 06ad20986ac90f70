// graph_gather.hip -- Gather with constant indices and board flips of the general graph path: a table-driven copy
// inside each board.  Per board the source is a block of `blockFloats` floats and the output `rowsPerBoard` rows of
// outStride floats; output element (r, c) with c < C is src[board * blockFloats + rowTab[r] + colTab[c]].  Which form
// the planner lowered (a channel list, the squares re-ordered or mirrored, one square's token, one channel of every
// square, the flattened view of a spatial tensor) is in the two tables only (onnx_graph.h, Launch::gatherTabOff).
//
//   * a thread owns four consecutive output channels of one (board, row): one 16-byte load of colTab, one load of
//     rowTab[r], four scalar loads from the source, one 16-byte store.  Every source element may lie anywhere in the
//     block, so there is nothing to vectorise on the read side and nothing to share: no LDS, no barrier, no atomics;
//   * the lanes of a wave walk consecutive 16-byte pieces of an output row, then the next row: the stores coalesce, and
//     so do the loads wherever the table holds runs (a flip or one square's token reads whole rows);
//   * a lane's channels at or past C are stored as zeros without loading; colTab's pad entries are zeros and are not used;
//   * the tables are validated by the planner (no entry negative, max(rowTab) + max(colTab) < blockFloats): every read
//     stays inside the board's own block, so a board's bits do not depend on its batch.  There is no check here.
//
// A gather moves bits: the output is bit for bit the source's elements.
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

constexpr int kGatherThreads = 256;

__global__ __launch_bounds__(kGatherThreads) void graphGather(const float* __restrict__ src, long blockFloats,
                                                              const int* __restrict__ rowTab, const int* __restrict__ colTab,
                                                              float* __restrict__ out, int outStride, int C, int rowsPerBoard,
                                                              int boards) {
    const int q4 = outStride >> 2;
    const long idx = (long)blockIdx.x * kGatherThreads + threadIdx.x;
    if (idx >= (long)boards * rowsPerBoard * q4) return;
    const long br = idx / q4; // board * rowsPerBoard + r: the output row
    const int c0 = (int)(idx - br * q4) * 4;
    const long b = br / rowsPerBoard;
    const int r = (int)(br - b * rowsPerBoard);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c0 < C) {
        const int4 ct = *(const int4*)(colTab + c0);
        const float* p = src + b * blockFloats + rowTab[r];
        v.x = p[ct.x];
        if (c0 + 1 < C) v.y = p[ct.y];
        if (c0 + 2 < C) v.z = p[ct.z];
        if (c0 + 3 < C) v.w = p[ct.w];
    }
    *(float4*)(out + br * outStride + c0) = v;
}

} // namespace

hipError_t launchGraphGather(const float* src, long blockFloats, const int* rowTab, const int* colTab, float* out,
                             int outStride, int C, int rowsPerBoard, int boards, hipStream_t stream) {
    if (boards <= 0 || rowsPerBoard <= 0 || blockFloats <= 0 || C <= 0 || outStride <= 0 || outStride % 16 != 0 ||
        C > outStride || !src || !rowTab || !colTab || !out)
        return hipErrorInvalidValue;
    const long items = (long)boards * rowsPerBoard * (outStride / 4);
    hipLaunchKernelGGL(graphGather, dim3((unsigned)((items + kGatherThreads - 1) / kGatherThreads)), dim3(kGatherThreads), 0,
                       stream, src, blockFloats, rowTab, colTab, out, outStride, C, rowsPerBoard, boards);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
