// graph_act.h -- the activation of the general graph path's kernels: the conv, dense and depthwise epilogues
// (graph_conv.hip) and the elementwise program's kEltAct (graph_ops.hip) share this one definition.  Device code.
#ifndef NSG_GRAPH_ACT_H
#define NSG_GRAPH_ACT_H

#include <hip/hip_runtime.h>

#include "../onnx_graph.h"

namespace nsg {
namespace graph {

__device__ inline float applyAct(float v, int act) {
    switch (act) {
    case kActRelu: return v > 0.f ? v : 0.f;
    case kActSigmoid: return 1.f / (1.f + expf(-v));
    case kActTanh: return tanhf(v);
    case kActSwish: return v / (1.f + expf(-v));
    case kActSoftplus: return v > 20.f ? v : log1pf(expf(v)); // torch's threshold
    case kActErf: return erff(v);
    // exact GELU; 1 + erf(x) as erfc(-x), which keeps its relative accuracy where erf(x) is near -1 (1 + erff(x) is 0
    // from x = -4 on, and a few bits above that)
    case kActGelu: return 0.5f * v * erfcf(v * -0.70710678118654752f);
    case kActRelu6: return fminf(fmaxf(v, 0.f), 6.f);
    // relu6(v + 3) / 6 as torch defines it: v + 3 is exact around the knee at -3, where v / 6 + 0.5 cancels and
    // carries the rounding of v / 6 into the result (8 to 11 ulps on a grid of 1/8)
    case kActHardSwish: return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);
    case kActHardSigmoid: return fminf(fmaxf(v + 3.f, 0.f), 6.f) * (1.f / 6.f);
    default: return v;
    }
}

} // namespace graph
} // namespace nsg

#endif
