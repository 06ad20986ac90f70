// plan_lifetimes.h -- what assignBuffers knew before it renamed the views: printed by `plan_dump --lifetimes` and checked
// by tests/plan_check.py (the rules R1-R5 of DESIGN.md section 13.7).  A debug table beside the plan: it is no part of
// GraphPlan, nothing on the device reads it, and nsg_capi.hip does not include this file.
#ifndef NSG_PLAN_LIFETIMES_H
#define NSG_PLAN_LIFETIMES_H

#include "onnx_graph.h"

namespace nsg {
namespace graph {

struct ViewTrace {
    std::string field; // the view's name in its record's views() (onnx_graph.h); an elementwise source is named by its mode
    int virt = -1;     // its virtual buffer before the renaming (-1: the plane buffer, -2: no residual)
    View v;            // the view as the launch sees it, renamed
};
struct LifetimeTrace {
    std::vector<std::vector<ViewTrace>> launches; // per launch, in forEachNamedView's order: `out` is the last
    std::vector<ViewTrace> outputs;               // policy, value, draw
    std::vector<int> virtStride, virtAlsoFlat, virtPhys; // per virtual buffer (a line tensor's stride: lines * stride)
    std::vector<bool> virtSpatial;
};

// buildPlan, and the table of the plan it returns
bool buildPlanTraced(const void* data, size_t size, int numChannels, GraphPlan* plan, LifetimeTrace* trace, std::string* error);

} // namespace graph
} // namespace nsg

#endif
