// graph_exec.h -- the general graph path's executor: one launch of a GraphPlan (onnx_graph.h) onto the device.
// graph_exec.hip holds one function per argument record, each marshaling its record into the launch wrappers of
// kernels/graph_kernels.h; nsg_capi.hip's enqueueGraph walks the plan and calls runLaunch for every launch.
#ifndef NSG_GRAPH_EXEC_H
#define NSG_GRAPH_EXEC_H

#include <hip/hip_runtime.h>

#include "onnx_graph.h"

namespace nsg {
namespace graph {

// The device memory a plan's views name: the plane buffer (View::buf == -1), the activation buffers (View::buf >= 0) and
// the plan's constants (GraphPlan::weights, uploaded once).
struct GraphBufs {
    float* planes;
    float* const* act;
    const float* weights;
};

// Enqueues launch L for `boards` boards on `stream`.
hipError_t runLaunch(const Launch& L, const GraphBufs& bufs, int boards, hipStream_t stream);

} // namespace graph
} // namespace nsg

#endif
