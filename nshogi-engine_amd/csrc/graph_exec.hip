// graph_exec.hip -- see graph_exec.h: one function per argument record of onnx_graph.h, each marshaling its record
// into the launch wrappers of kernels/graph_kernels.h.  Host code only: the kernels are in kernels/graph_*.hip.
#include "graph_exec.h"

#include "kernels/graph_kernels.h"

namespace nsg {
namespace graph {

namespace {

struct Exec {
    const View& out;
    const GraphBufs& bufs;
    const int B;
    const hipStream_t s;

    float* ptr(const View& v) const { return v.buf < 0 ? bufs.planes : bufs.act[(size_t)v.buf]; }
    DevView dv(const View& v) const {
        DevView d;
        d.p = ptr(v); d.stride = v.stride; d.offset = v.offset; d.C = v.C;
        return d;
    }
    long rowsOf(const View& v) const { return v.spatial ? (long)B * 81 : v.lines ? (long)B * v.lines : (long)B; }
    const float* wts(size_t off) const { return bufs.weights + off; }

    hipError_t operator()(const ConvArgs& A) const {
        DevView res;
        if (A.res.buf != kNoRes) res = dv(A.res);
        switch (A.kernel()) {
        case ConvArgs::kDepthwise:
            return launchGraphDepthwise(ptr(A.in), A.in.stride, wts(A.wOff), wts(A.biasOff), res, ptr(out), out.stride, out.C,
                                        A.kh, A.kw, A.dh, A.dw, B, A.act, s);
        case ConvArgs::kGrouped:
            return launchGraphConvGrouped(ptr(A.in), A.in.stride, wts(A.wOff), wts(A.biasOff), (const int*)wts(A.gTabOff), res,
                                          ptr(out), out.stride, out.C, A.kh, A.kw, A.dh, A.dw, B, A.act, s);
        case ConvArgs::kGeo:
            return launchGraphConvGeo(ptr(A.in), A.in.stride, wts(A.wOff), wts(A.biasOff), res, ptr(out), out.stride, out.C,
                                      A.cinPad, A.coutTiles, A.kh, A.kw, A.dh, A.dw, B, A.act, s);
        case ConvArgs::kTile:
            break;
        }
        // a dense layer runs over groups of 81 rows: boards, or the (board, head) rows of a head-row tensor
        const long denseRows = (long)B * A.rowsPerBoard;
        const int groups = A.dense ? (int)((denseRows + 80) / 81) : B;
        return launchGraphConv(ptr(A.in), A.in.stride, wts(A.wOff), wts(A.biasOff), res, ptr(out), out.stride, out.C, A.cinPad,
                               A.coutTiles, A.taps, groups, A.dense ? denseRows : rowsOf(out), A.act, s);
    }

    hipError_t operator()(const EltProgram& A) const {
        EltArgs a{};
        for (size_t i = 0; i < A.srcs.size(); ++i) {
            const EltSrc& S = A.srcs[i];
            a.mode[i] = S.mode;
            a.scalar[i] = S.scalar;
            if (S.mode == kSrcChannel || S.mode == kSrcSquareChannel || S.mode == kSrcSquare) a.src[i] = wts(S.constOff);
            else if (S.mode != kSrcScalar) { a.src[i] = ptr(S.v); a.stride[i] = S.v.stride; a.offset[i] = S.v.offset; }
            a.bufLines[i] = S.v.bufLines;
            a.line0[i] = S.v.line0;
        }
        a.outLines = out.lines;
        for (size_t i = 0; i < A.code.size(); ++i)
            a.code[i] = (uint32_t)A.code[i].op | (uint32_t)A.code[i].dst << 8 | (uint32_t)A.code[i].a << 16 | (uint32_t)A.code[i].b << 24;
        a.ncode = (int)A.code.size();
        a.outReg = A.eltOut;
        a.out = ptr(out);
        a.outStride = out.stride;
        a.C = out.C;
        a.rows = rowsOf(out);
        return launchGraphElt(a, s);
    }

    hipError_t operator()(const SquareReduceArgs& A) const {
        return A.max ? launchGraphMax(dv(A.in), ptr(out), out.stride, B, s) : launchGraphMean(dv(A.in), ptr(out), out.stride, B, s);
    }

    hipError_t operator()(const ConcatSegs& A) const {
        ConcatArgs a{};
        for (size_t i = 0; i < A.segs.size(); ++i) {
            const CopySeg& S = A.segs[i];
            a.src[i] = ptr(S.v); a.stride[i] = S.v.stride; a.offset[i] = S.v.offset;
            a.count[i] = S.v.C; a.dstOff[i] = S.dstOff;
        }
        a.nseg = (int)A.segs.size();
        a.out = ptr(out);
        a.outStride = out.stride;
        a.rows = rowsOf(out);
        return launchGraphConcat(a, s);
    }

    hipError_t operator()(const FlattenArgs& A) const { return launchGraphFlatten(dv(A.in), ptr(out), out.stride, B, s); }

    hipError_t operator()(const PoolArgs& A) const {
        return launchGraphPool(dv(A.in), ptr(out), out.stride, A.kh, A.kw, A.dh, A.dw, A.poolMode, B, s);
    }

    hipError_t operator()(const LinePoolArgs& A) const {
        return launchGraphLinePool(dv(A.in), ptr(out), out.stride, out.bufLines, out.line0, A.lineFiles, A.poolMode, B, s);
    }

    hipError_t operator()(const LayerNormArgs& A) const {
        return launchGraphLayerNorm(dv(A.in), wts(A.wOff), wts(A.biasOff), A.eps, ptr(out), out.stride, rowsOf(out), s);
    }

    hipError_t operator()(const GroupNormArgs& A) const {
        return launchGraphGroupNorm(dv(A.in), A.groups, wts(A.wOff), wts(A.biasOff), A.eps, A.act, ptr(out), out.stride, B, s);
    }

    hipError_t operator()(const RmsNormArgs& A) const {
        return launchGraphRmsNorm(dv(A.in), wts(A.wOff), A.eps, ptr(out), out.stride, rowsOf(out), s);
    }

    hipError_t operator()(const AttentionArgs& A) const {
        RtBias rt;
        if (A.hasRtBias) {
            rt.p = ptr(A.rtBias) + A.rtBias.offset;
            rt.boardStride = A.rtBias.stride;
            rt.headStride = A.rtHeadStride;
            rt.scale = A.rtScale;
        }
        return launchGraphAttention(dv(A.in), dv(A.attK), dv(A.attV), A.hasBias ? wts(A.biasOff) : nullptr, A.scale, rt, ptr(out),
                                    out.stride, A.heads, A.headDim, B, s);
    }

    hipError_t operator()(const BmmArgs& A) const {
        return A.bmmNN ? launchGraphBmmNN(dv(A.in), dv(A.bmmB), A.scale, A.act, ptr(out), out.stride, B, s)
                       : launchGraphBmmNT(dv(A.in), dv(A.bmmB), A.scale, A.act, ptr(out), out.stride, B, s);
    }

    hipError_t operator()(const TokenMixArgs& A) const {
        return launchGraphTokenMix(dv(A.in), wts(A.wOff), A.mixD, A.mixStages, A.act, A.mixAct2, ptr(out), out.stride, B, s);
    }

    hipError_t operator()(const GatherArgs& A) const {
        const int* tabs = (const int*)wts(A.gatherTabOff); // rowTab, then colTab at the next multiple of 4 ints
        return launchGraphGather(ptr(A.in), A.gatherBlock, tabs, tabs + (A.gatherRows + 3) / 4 * 4, ptr(out), out.stride, out.C,
                                 A.gatherRows, B, s);
    }

    hipError_t operator()(const ChanReduceArgs& A) const {
        return launchGraphChanReduce(dv(A.in), A.redMode, A.scale, ptr(out), out.stride, rowsOf(out), s);
    }

    hipError_t operator()(const NormalizeArgs& A) const {
        return launchGraphNormalize(dv(A.in), A.p, A.eps, ptr(out), out.stride, rowsOf(out), s);
    }
};

} // namespace

hipError_t runLaunch(const Launch& L, const GraphBufs& bufs, int boards, hipStream_t stream) {
    return std::visit(Exec{L.out, bufs, boards, stream}, L.args);
}

} // namespace graph
} // namespace nsg
