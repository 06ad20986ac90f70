// graph_act.h -- the activation of the general graph path's kernels: the conv, dense and depthwise epilogues
// (graph_conv.hip) and the elementwise program's kEltAct (graph_ops.hip) share this one definition.  Device code.
#ifndef NSG_GRAPH_ACT_H
#define NSG_GRAPH_ACT_H

#include <hip/hip_runtime.h>

#include "../onnx_graph.h"

namespace nsg {
namespace graph {

// The maths codes, out of line: graphConv's epilogue unrolls applyAct 24 times, and with these cases inlined its text
// outgrew the instruction cache (the 3x3 kernel ran 2 to 7 % slower on a net that uses none of them).
__device__ __attribute__((noinline)) float applyActMath(float v, int act) {
    switch (act) {
    case kActExp: return expf(v);
    case kActLog: return logf(v);
    // sqrtf and the division are the correctly rounded ones (hipcc's default): 0 ulps
    case kActSqrt: return sqrtf(v);
    case kActRecip: return 1.f / v;
    // v tanh(softplus(v)) with tanh(log(1 + e)) = ((1 + e)^2 - 1) / ((1 + e)^2 + 1) = n / (n + 2), n = e (e + 2), e = exp(v):
    // no difference of near-equal terms at either end.  e underflows to 0 far left (v * 0 = -0, never inf * 0); from
    // v = 20 on the factor is 1 in f32 (1 - 2 exp(-40)) and e^2 would overflow from v = 44 on
    case kActMish: {
        if (v > 20.f) return v;
        const float e = expf(v), n = e * (e + 2.f);
        return v * (n / (n + 2.f));
    }
    // 0.5 v (1 + tanh(u)), u = sqrt(2/pi) (v + 0.044715 v^3), as v / (1 + exp(-2u)): 1 + tanh(u) = 2 / (1 + exp(-2u))
    // cancels nowhere (1 + tanhf(u) is 0 from u = -9 on).  u = v (k + 0.044715 k v^2) needs no v^3; where v^2 overflows
    // u is +-inf and the result v or -0, as it is long before
    case kActGeluTanh: {
        const float u2 = v * fmaf(v * v, (float)(-2.0 * 0.7978845608028654 * 0.044715), (float)(-2.0 * 0.7978845608028654));
        return v / (1.f + expf(u2));
    }
    case kActSoftsign: return v / (1.f + fabsf(v));
    default: return v;
    }
}

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
    default: return act >= kActExp ? applyActMath(v, act) : v;
    }
}

} // namespace graph
} // namespace nsg

#endif
