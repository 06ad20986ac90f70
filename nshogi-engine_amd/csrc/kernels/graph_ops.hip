// graph_ops.hip -- the general graph path's small kernels: the fused elementwise chain, the mean and the max over
// the 81 squares, channel concat / copy, flatten to ONNX order, and the scatter into the evaluator's outputs.  One thread
// per output element; every kernel writes zeros into the channels between C and the row stride.
#include "graph_act.h"
#include "graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

constexpr int kThreads = 256;

unsigned blocksFor(long n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// The program is read from the kernel arguments (constant memory): one kernel serves every chain.
__global__ __launch_bounds__(kThreads) void graphElt(EltArgs a) {
    const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= a.rows * a.outStride) return;
    const long row = idx / a.outStride;
    const int c = (int)(idx - row * a.outStride);
    if (c >= a.C) {
        a.out[idx] = 0.f;
        return;
    }
    float r[kMaxEltRegs];
    for (int i = 0; i < a.ncode; ++i) {
        const uint32_t in = a.code[i];
        const int op = in & 0xff, dst = (in >> 8) & 0xff, x = (in >> 16) & 0xff, y = in >> 24;
        float v;
        switch (op) {
        case kEltLoad: {
            const float* p = a.src[x];
            switch (a.mode[x]) {
            case kSrcSame: v = p[(size_t)row * a.stride[x] + a.offset[x] + c]; break;
            case kSrcBoard: v = p[(size_t)(row / 81) * a.stride[x] + a.offset[x] + c]; break;
            case kSrcChannel: v = p[c]; break;
            case kSrcSquareChannel: v = p[(size_t)(row % 81) * a.C + c]; break;
            case kSrcRankLine: // one value per rank, broadcast over its files
                v = p[(size_t)((row / 81) * a.bufLines[x] + a.line0[x] + (int)(row % 81) / 9) * a.stride[x] + a.offset[x] + c];
                break;
            case kSrcFileLine: // one value per file, broadcast over its ranks
                v = p[(size_t)((row / 81) * a.bufLines[x] + a.line0[x] + (int)(row % 81) % 9) * a.stride[x] + a.offset[x] + c];
                break;
            case kSrcLine: // a view of outLines of the buffer's lines
                v = p[(size_t)((row / a.outLines) * a.bufLines[x] + a.line0[x] + (int)(row % a.outLines)) * a.stride[x] + a.offset[x] + c];
                break;
            case kSrcRowOne: v = p[(size_t)row * a.stride[x] + a.offset[x]]; break; // channel 0 of a one-channel view's row
            case kSrcBoardOne: v = p[(size_t)(row / 81) * a.stride[x] + a.offset[x]]; break; // ... of its board's flat row
            case kSrcSquare: v = p[row % 81]; break;
            default: v = a.scalar[x]; break;
            }
            break;
        }
        case kEltAct: v = applyAct(r[x], y); break;
        case kEltAdd: v = r[x] + r[y]; break;
        case kEltSub: v = r[x] - r[y]; break;
        case kEltMul: v = r[x] * r[y]; break;
        case kEltMax: v = fmaxf(r[x], r[y]); break;
        case kEltMin: v = fminf(r[x], r[y]); break;
        case kEltLeaky: v = r[x] > 0.f ? r[x] : r[x] * r[y]; break;
        case kEltNeg: v = -r[x]; break;
        case kEltAbs: v = fabsf(r[x]); break;
        case kEltPow: v = powf(r[x], r[y]); break;
        default: v = r[x] / r[y]; break;
        }
        r[dst] = v;
    }
    a.out[idx] = r[a.outReg];
}

__global__ __launch_bounds__(kThreads) void graphMean(const float* __restrict__ in, int inStride, int inOff, int C,
                                                      float* __restrict__ out, int outStride, int boards) {
    const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (long)boards * outStride) return;
    const long b = idx / outStride;
    const int c = (int)(idx - b * outStride);
    float s = 0.f;
    if (c < C) {
        const float* p = in + (size_t)b * 81 * inStride + inOff + c;
        for (int sq = 0; sq < 81; ++sq) s += p[(size_t)sq * inStride];
        s /= 81.f;
    }
    out[idx] = s;
}

// The max over the 81 squares; graphMean's indexing, so that graphMean itself stays as it was.
__global__ __launch_bounds__(kThreads) void graphMax(const float* __restrict__ in, int inStride, int inOff, int C,
                                                     float* __restrict__ out, int outStride, int boards) {
    const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (long)boards * outStride) return;
    const long b = idx / outStride;
    const int c = (int)(idx - b * outStride);
    float s = 0.f;
    if (c < C) {
        const float* p = in + (size_t)b * 81 * inStride + inOff + c;
        s = p[0];
        for (int sq = 1; sq < 81; ++sq) s = fmaxf(s, p[(size_t)sq * inStride]);
    }
    out[idx] = s;
}

__global__ __launch_bounds__(kThreads) void graphConcat(ConcatArgs a) {
    const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= a.rows * a.outStride) return;
    const long row = idx / a.outStride;
    const int c = (int)(idx - row * a.outStride);
    float v = 0.f;
    for (int s = 0; s < a.nseg; ++s)
        if (c >= a.dstOff[s] && c < a.dstOff[s] + a.count[s])
            v = a.src[s][(size_t)row * a.stride[s] + a.offset[s] + (c - a.dstOff[s])];
    a.out[idx] = v;
}

__global__ __launch_bounds__(kThreads) void graphFlatten(const float* __restrict__ in, int inStride, int inOff, int C,
                                                         float* __restrict__ out, int outStride, int boards) {
    const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (long)boards * outStride) return;
    const long b = idx / outStride;
    const int k = (int)(idx - b * outStride);
    float v = 0.f;
    if (k < C * 81) {
        const int c = k / 81, sq = k - c * 81;
        v = in[(size_t)(b * 81 + sq) * inStride + inOff + c];
    }
    out[idx] = v;
}

__global__ __launch_bounds__(kThreads) void graphOutputs(DevView pol, int polSpatial, DevView val, DevView drw,
                                                         float* __restrict__ dstPolicy, float* __restrict__ dstValue,
                                                         float* __restrict__ dstDraw, int boards) {
    constexpr int kPolicy = 2187;
    const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= (long)boards * kPolicy) return;
    const long b = idx / kPolicy;
    const int k = (int)(idx - b * kPolicy);
    if (polSpatial) {
        const int c = k / 81, sq = k - c * 81;
        dstPolicy[idx] = pol.p[(size_t)(b * 81 + sq) * pol.stride + pol.offset + c];
    } else {
        dstPolicy[idx] = pol.p[(size_t)b * pol.stride + pol.offset + k];
    }
    if (k == 0) {
        dstValue[b] = val.p[(size_t)b * val.stride + val.offset];
        dstDraw[b] = drw.p[(size_t)b * drw.stride + drw.offset];
    }
}

} // namespace

hipError_t launchGraphElt(const EltArgs& a, hipStream_t stream) {
    if (a.rows <= 0 || a.ncode <= 0 || a.ncode > kMaxEltCode) return hipErrorInvalidValue;
    for (int i = 0; i < kMaxEltSrcs; ++i) {
        const bool line = a.mode[i] == kSrcRankLine || a.mode[i] == kSrcFileLine || a.mode[i] == kSrcLine;
        const int lines = a.mode[i] == kSrcLine ? a.outLines : 9;
        if (line && (a.line0[i] < 0 || lines <= 0 || a.line0[i] + lines > a.bufLines[i])) return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(graphElt, dim3(blocksFor(a.rows * a.outStride)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchGraphMean(DevView in, float* out, int outStride, int boards, hipStream_t stream) {
    if (boards <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(graphMean, dim3(blocksFor((long)boards * outStride)), dim3(kThreads), 0, stream, in.p, in.stride,
                       in.offset, in.C, out, outStride, boards);
    return hipGetLastError();
}

hipError_t launchGraphMax(DevView in, float* out, int outStride, int boards, hipStream_t stream) {
    if (boards <= 0 || in.offset + in.C > in.stride || outStride < in.C) return hipErrorInvalidValue;
    hipLaunchKernelGGL(graphMax, dim3(blocksFor((long)boards * outStride)), dim3(kThreads), 0, stream, in.p, in.stride,
                       in.offset, in.C, out, outStride, boards);
    return hipGetLastError();
}

hipError_t launchGraphConcat(const ConcatArgs& a, hipStream_t stream) {
    if (a.rows <= 0 || a.nseg <= 0 || a.nseg > kMaxCopySegs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(graphConcat, dim3(blocksFor(a.rows * a.outStride)), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launchGraphFlatten(DevView in, float* out, int outStride, int boards, hipStream_t stream) {
    if (boards <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(graphFlatten, dim3(blocksFor((long)boards * outStride)), dim3(kThreads), 0, stream, in.p,
                       in.stride, in.offset, in.C, out, outStride, boards);
    return hipGetLastError();
}

hipError_t launchGraphOutputs(DevView policy, bool policySpatial, DevView value, DevView draw, float* dstPolicy,
                              float* dstValue, float* dstDraw, int boards, hipStream_t stream) {
    if (boards <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(graphOutputs, dim3(blocksFor((long)boards * 2187)), dim3(kThreads), 0, stream, policy,
                       policySpatial ? 1 : 0, value, draw, dstPolicy, dstValue, dstDraw, boards);
    return hipGetLastError();
}

} // namespace graph
} // namespace nsg
