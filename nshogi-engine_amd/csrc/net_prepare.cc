// net_prepare.cc -- see net_prepare.h.
#include "net_prepare.h"

#include "../../include/nsg.h" // the error codes, NSG_NUM_SQUARES, NSG_MOVE_INDEX_MAX

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <thread>

namespace nsg {

namespace {

int fail(std::string* err, int code, const char* fmt, ...) {
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    *err = buf;
    return code;
}

int roundUp(int a, int b) { return (a + b - 1) / b * b; }

} // namespace

int parseBlob(const void* blob, size_t size, NetView* nv, std::string* err) {
    if (size < 64) return fail(err, NSG_E_FORMAT, "weight blob too small (%zu bytes)", size);
    const unsigned char* p = (const unsigned char*)blob;
    if (memcmp(p, "NSGW", 4) != 0) return fail(err, NSG_E_FORMAT, "bad magic (not an NSGW file)");
    uint32_t h[15];
    memcpy(h, p + 4, sizeof(h));
    if (h[0] != 1) return fail(err, NSG_E_FORMAT, "unsupported NSGW version %u", h[0]);
    nv->cin = (int)h[1]; nv->F = (int)h[2]; nv->blocks = (int)h[3];
    nv->pc = (int)h[4]; nv->vc = (int)h[5]; nv->vh = (int)h[6];
    memcpy(&nv->eps, &h[7], 4);
    const size_t F = nv->F, C = nv->cin, VC = nv->vc, VH = nv->vh, PC = nv->pc;
    if (F == 0 || C == 0 || VC == 0 || VH == 0 || PC == 0 || nv->blocks < 0)
        return fail(err, NSG_E_FORMAT, "zero dimension in NSGW header");
    const size_t need = F * C * 9 + 4 * F + (size_t)nv->blocks * 2 * (F * F * 9 + 4 * F) +
                        PC * F + PC + VC * F + 4 * VC + VH * VC * 81 + VH + 2 * VH + 2;
    if (size != 64 + need * sizeof(float))
        return fail(err, NSG_E_FORMAT, "NSGW size mismatch: have %zu, header implies %zu", size,
                    64 + need * sizeof(float));
    nv->params = need;
    const float* f = (const float*)(p + 64);
    nv->stemW = f; f += F * C * 9;
    nv->stemBn = f; f += 4 * F;
    nv->w1.resize(nv->blocks); nv->bn1.resize(nv->blocks);
    nv->w2.resize(nv->blocks); nv->bn2.resize(nv->blocks);
    for (int k = 0; k < nv->blocks; ++k) {
        nv->w1[k] = f; f += F * F * 9;
        nv->bn1[k] = f; f += 4 * F;
        nv->w2[k] = f; f += F * F * 9;
        nv->bn2[k] = f; f += 4 * F;
    }
    nv->polW = f; f += PC * F;
    nv->polB = f; f += PC;
    nv->valW = f; f += VC * F;
    nv->valBn = f; f += 4 * VC;
    nv->fc1W = f; f += VH * VC * 81;
    nv->fc1B = f; f += VH;
    nv->fc2W = f; f += 2 * VH;
    nv->fc2B = f; f += 2;
    return NSG_OK;
}

int checkSpecialised(const NetView& nv, int numChannels, std::string* err) {
    if (nv.cin != numChannels)
        return fail(err, NSG_E_FORMAT, "weight file expects %d input planes, evaluator has %d", nv.cin, numChannels);
    // trt.cc:193-210: the policy output must have ml::MoveIndexMax elements
    if (nv.pc * NSG_NUM_SQUARES != NSG_MOVE_INDEX_MAX)
        return fail(err, NSG_E_FORMAT, "Unexpected PolicySize: %d (expected: %d).",
                    nv.pc * NSG_NUM_SQUARES, NSG_MOVE_INDEX_MAX);
    if (nv.F % 64 != 0) return fail(err, NSG_E_FORMAT, "trunk width %d is not a multiple of 64", nv.F);
    if (nv.vh % 64 != 0) return fail(err, NSG_E_FORMAT, "value hidden width %d is not a multiple of 64", nv.vh);
    return NSG_OK;
}

namespace {

// BN folding in double: w' = w * g/sqrt(v+eps), b' = beta - mean * g/sqrt(v+eps)
void foldBn(const float* bn, int n, float eps, std::vector<double>* scale, std::vector<float>* bias) {
    scale->resize(n);
    bias->resize(n);
    for (int i = 0; i < n; ++i) {
        const double g = bn[0 * n + i], b = bn[1 * n + i], m = bn[2 * n + i], v = bn[3 * n + i];
        const double s = g / std::sqrt(v + (double)eps);
        (*scale)[i] = s;
        (*bias)[i] = (float)(b - m * s);
    }
}

// kF16m8's correction operands are e4m3 copies under FIXED scales (kernels.h): x_hi as it is and
// x_lo * 2^12 must stay below 448, i.e. activations below ~224 (an f16 residual is at most 2^-11 of its
// value); beyond that the copies clamp and the error drifts from 1e-4 towards plain f16's 1e-2
// (profiles/r02/c_envelope_sweep.txt).  The bound is estimated from the WEIGHTS at load time by pushing
// a second moment through the folded layers -- uncorrelated inputs: E[y_c^2] = |w'_c|^2 E[x^2] + b'_c^2,
// a ReLU keeps half of it, a residual add sums the branches -- and taking six standard deviations of the
// widest channel.  Crude (it ignores correlations) but monotone in what matters: BN gains, weight norms.
void pushConvMoment(const float* w, const double* scale, const float* bias, int cout, int cin, int taps,
                    double in2, double* out2Max, double* out2Mean) {
    double worst = 0.0, mean = 0.0;
    for (int n = 0; n < cout; ++n) {
        double ss = 0.0;
        const float* wn = w + (size_t)n * cin * taps;
        for (int k = 0; k < cin * taps; ++k) ss += (double)wn[k] * wn[k];
        const double y2 = ss * scale[n] * scale[n] * in2 + (double)bias[n] * bias[n];
        worst = std::max(worst, y2);
        mean += y2;
    }
    *out2Max = worst;
    *out2Mean = mean / cout;
}

struct Conv3Ctx { const float* w; const double* scale; int cin; };
float conv3Get(const void* c, int n, int k, int tap) {
    const Conv3Ctx* x = (const Conv3Ctx*)c;
    return (float)((double)x->w[((size_t)n * x->cin + k) * 9 + tap] * x->scale[n]);
}
struct HeadsCtx { const float* valW; const double* valScale; const float* polW; int F, vc, pc; };
float headsGet(const void* c, int n, int k, int) {
    const HeadsCtx* x = (const HeadsCtx*)c;
    if (n < x->vc) return (float)((double)x->valW[(size_t)n * x->F + k] * x->valScale[n]);
    if (n < x->vc + x->pc) return x->polW[(size_t)(n - x->vc) * x->F + k];
    return 0.f;
}
struct Fc1Ctx { const float* w; int vc; };
float fc1Get(const void* c, int n, int k, int) {
    const Fc1Ctx* x = (const Fc1Ctx*)c;
    const int sq = k / x->vc, ch = k - sq * x->vc; // device K index = sq*VC + c
    return x->w[(size_t)n * x->vc * 81 + (size_t)ch * 81 + sq];
}

// ---------------------------------------------------------------------------
// Host-side weight packing.  Record (q, nf, lane) holds, for MFMA row
// rho = lane & 15 and lane group g = lane >> 4 of output fragment nf:
//   out channel n = (nf / 4) * 64 + (rho >> 2) * 16 + (nf % 4) * 4 + (rho & 3)
//   record      q = (kc*taps + tap)*2 + s
//   f32  : 4 values, input channel kc*32 + s*16 + 4*g + i          (i = 0..3)
//   16b  : 8 values, input channel kc*64 + s*32 + 8*g + i          (i = 0..7)
//   f16x3: 8 values, input channel kc*32 + 8*g + i; s = 0: hi, 1: lo
// Sixteen zero records are appended so the kernel's prefetch (up to 16 records ahead for
// small-batch tiles) never reads past the allocation.
// ---------------------------------------------------------------------------
inline uint16_t hostF32ToF16(float f) {
    const _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
inline uint16_t hostF32ToBf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40); // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u); // round to nearest even
    return (uint16_t)(u >> 16);
}

// OCP e4m3 (bias 7, max 448, no infinities), round to nearest even, saturating.
uint8_t hostF32ToE4m3(float v) {
    const uint8_t sign = std::signbit(v) ? 0x80 : 0;
    float a = std::fabs(v);
    if (!(a == a)) return sign | 0x7f;
    if (a >= 448.f) return sign | 0x7e;
    if (a < 0x1p-10f) return sign; // below half the smallest subnormal (2^-9)
    int e;
    (void)std::frexp(a, &e); // a = m * 2^e, m in [0.5, 1)
    int ex = e - 1;          // a in [2^ex, 2^(ex+1))
    if (ex < -6) ex = -6;    // subnormal range: step 2^-9
    const float step = std::ldexp(1.f, ex - 3);
    float q = std::nearbyint(a / step); // ties to even (default rounding mode)
    float r = q * step;
    if (r >= 448.f) return sign | 0x7e;
    // re-derive exponent after rounding (may have carried)
    int e2;
    (void)std::frexp(r, &e2);
    int ex2 = e2 - 1;
    if (r < 0x1p-6f) { // subnormal
        return sign | (uint8_t)std::lrint(r / 0x1p-9f);
    }
    const int mant = (int)std::lrint(r / std::ldexp(1.f, ex2 - 3)) - 8;
    return sign | (uint8_t)(((ex2 + 7) << 3) | (mant & 7));
}

// e2m3 (fp6: 1 sign, 2 exponent, 3 mantissa bits, bias 1, max 7.5), round to nearest even, saturating;
// the value is already divided by its block scale.
uint8_t hostF32ToE2m3(float v) {
    const uint8_t sign = std::signbit(v) ? 0x20 : 0;
    float a = std::fabs(v);
    if (!(a == a) || a >= 7.5f) return sign | 0x1f;
    int ex = 0; // a in [2^ex, 2^(ex+1)), clamped to the format's three binades; below 1: subnormal step 1/8
    if (a >= 4.f) ex = 2; else if (a >= 2.f) ex = 1;
    const float step = std::ldexp(1.f, ex - 3);
    const float r = std::nearbyint(a / step) * step; // ties to even
    if (r >= 7.5f) return sign | 0x1f;
    if (r < 1.f) return sign | (uint8_t)std::lrint(r * 8.f);
    int e2 = r >= 4.f ? 2 : (r >= 2.f ? 1 : 0);
    const int mant = (int)std::lrint(r / std::ldexp(1.f, e2 - 3)) - 8;
    return sign | (uint8_t)(((e2 + 1) << 3) | (mant & 7));
}

// The MX operand of one lane in the kF16m6 layout: 32 values -> 24 bytes of e2m3 codes (value j at
// bits [6j, 6j+6)), then the E8M0 exponent of the block (OCP MX rule: floor(log2(max|v|)) - 2), 7 bytes pad.
void packE2m3Block(const float* v, unsigned char* out32) {
    float maxAbs = 0.f;
    for (int j = 0; j < 32; ++j) maxAbs = std::fmax(maxAbs, std::fabs(v[j]));
    int e8 = 0;
    if (maxAbs > 0.f && std::isfinite(maxAbs)) {
        int e;
        (void)std::frexp(maxAbs, &e); // maxAbs in [2^(e-1), 2^e)
        e8 = std::min(254, std::max(1, e - 1 - 2 + 127));
    }
    memset(out32, 0, 32);
    const float inv = std::ldexp(1.f, 127 - e8);
    for (int j = 0; j < 32; ++j) {
        const unsigned code = e8 ? hostF32ToE2m3(v[j] * inv) : 0u;
        const int bit = 6 * j;
        out32[bit / 8] |= (unsigned char)(code << (bit % 8));
        if (bit % 8 > 2) out32[bit / 8 + 1] |= (unsigned char)(code >> (8 - bit % 8));
    }
    out32[24] = (unsigned char)e8;
}

// kF16m8 / kF16m6 conv weights (see kernels.h): per chunk pair (A, B) and tap t the slabs A.m_t, B.m_t, X_t
// in stream order.
void packTileWeightsM8(WeightGetter get, const void* ctx, int taps, int kReal, int kdim, int cout,
                       float scale, unsigned char* out, bool fp6) {
    const int npairs = kdim / 64;
    const int nft = cout / 16;
    // per tap: [main A: nft KiB][main B: nft KiB][MX slab: kF16m8 2 nft KiB; kF16m6 nft/4 groups of 6400 bytes =
    // 4 x 1 KiB code dwords 0-3, 4 x 512 B code dwords 4-5, 256 B exponent dwords (byte j = fragment j of the group)]
    const size_t mainSet = (size_t)nft * 1024, xSet = (size_t)nft * (fp6 ? 1600 : 2048), tapStride = 2 * mainSet + xSet;
    auto chan = [](int nf, int rho) {
        return (nf / kNfrag) * kNfrag * 16 + (rho >> 2) * 4 * kNfrag + (nf % kNfrag) * 4 + (rho & 3);
    };
    auto wval = [&](int n, int k, int t) { return (k < kReal) ? get(ctx, n, k, t) * scale : 0.f; };
    for (int cp = 0; cp < npairs; ++cp) {
        for (int t = 0; t < taps; ++t) {
            unsigned char* base = out + ((size_t)cp * taps + t) * tapStride;
            for (int half = 0; half < 2; ++half) { // main slabs: w_hi of chunk A, then of chunk B, 8 f16 per lane
                const int c = 2 * cp + half;
                for (int nf = 0; nf < nft; ++nf)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int rho = lane & 15, g = lane >> 4, n = chan(nf, rho);
                        unsigned char* rec = base + half * mainSet + ((size_t)nf * 64 + lane) * 16;
                        for (int i = 0; i < 8; ++i) {
                            const _Float16 h = (_Float16)wval(n, c * 32 + 8 * g + i, t);
                            memcpy(rec + i * 2, &h, 2);
                        }
                    }
            }
            unsigned char* xs = base + 2 * mainSet;
            if (fp6) { // MX slab, kF16m6: k-group g = (chunk g>>1, term g&1), one 24-byte e2m3 block + exponent per lane
                for (int nf = 0; nf < nft; ++nf)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int rho = lane & 15, g = lane >> 4, n = chan(nf, rho);
                        const int c = 2 * cp + (g >> 1);
                        float v32[32];
                        for (int j = 0; j < 32; ++j) {
                            // term 0: w_lo against the x_hi block; term 1: the copy of w_hi against the x_lo block
                            const float v = wval(n, c * 32 + j, t);
                            const _Float16 h = (_Float16)v;
                            v32[j] = (g & 1) ? (float)h : v - (float)h;
                        }
                        unsigned char blk[32];
                        packE2m3Block(v32, blk);
                        unsigned char* grp = xs + (size_t)(nf / kNfrag) * 6400;
                        const int j4 = nf % kNfrag;
                        memcpy(grp + (size_t)j4 * 1024 + lane * 16, blk, 16);
                        memcpy(grp + 4096 + (size_t)j4 * 512 + lane * 8, blk + 16, 8);
                        grp[6144 + lane * 4 + j4] = blk[24];
                    }
            } else
            for (int nf = 0; nf < nft; ++nf) // MX slab: k-group g = (chunk g>>1, term g&1), 32 fp8 per lane
                for (int h16 = 0; h16 < 2; ++h16)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int rho = lane & 15, g = lane >> 4, n = chan(nf, rho);
                        const int c = 2 * cp + (g >> 1);
                        unsigned char* rec = xs + (((size_t)nf * 2 + h16) * 64 + lane) * 16;
                        for (int i = 0; i < 16; ++i) {
                            const float v = wval(n, c * 32 + 16 * h16 + i, t);
                            const _Float16 h = (_Float16)v;
                            const float lo = v - (float)h;
                            rec[i] = (g & 1) ? hostF32ToE4m3(std::ldexp((float)h, kM8WHiShift))
                                             : hostF32ToE4m3(std::ldexp(lo, kM8WLoShift));
                        }
                    }
        }
    }
}
} // namespace

void packTileWeights(WeightGetter get, const void* ctx, int taps, int kReal,
                     int kdim, int cout, int prec, float scale, void* dst) {
    const int kcCh = chunkChannels(prec);
    const int nkc = kdim / kcCh;
    const int nft = cout / 16;
    const int spt = recordsPerTap(prec);
    const int per = (prec == kFp32) ? 4 : 8; // values per record
    unsigned char* out = (unsigned char*)dst;
    memset(out, 0, tileWeightRecords(taps, kdim, cout, prec) * 16);
    if (isMx(prec)) {
        packTileWeightsM8(get, ctx, taps, kReal, kdim, cout, scale, out, prec == kF16m6);
        return;
    }
    for (int c = 0; c < nkc; ++c)
        for (int t = 0; t < taps; ++t)
            for (int s = 0; s < spt; ++s) {
                const size_t q = ((size_t)c * taps + t) * spt + s;
                for (int nf = 0; nf < nft; ++nf)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int rho = lane & 15, g = lane >> 4;
                        const int n = (nf / kNfrag) * kNfrag * 16 + (rho >> 2) * 4 * kNfrag +
                                      (nf % kNfrag) * 4 + (rho & 3);
                        unsigned char* rec = out + ((q * nft + nf) * 64 + lane) * 16;
                        for (int i = 0; i < per; ++i) {
                            // kF16x3: both records cover the chunk's 32 channels
                            const int k = (prec == kF16x3) ? c * kcCh + per * g + i
                                                           : c * kcCh + s * (kcCh / 2) + per * g + i;
                            const float v = (k < kReal) ? get(ctx, n, k, t) * scale : 0.f;
                            if (prec == kFp32) {
                                memcpy(rec + i * 4, &v, 4);
                            } else if (prec == kF16x3) {
                                // records: w_hi (products with x_hi and x_lo), w_lo (with x_hi)
                                const _Float16 h = (_Float16)v;
                                const _Float16 l = (_Float16)(v - (float)h);
                                const _Float16 pick = (s == 1) ? l : h;
                                memcpy(rec + i * 2, &pick, 2);
                            } else {
                                const uint16_t hb = (prec == kFp16) ? hostF32ToF16(v) : hostF32ToBf16(v);
                                memcpy(rec + i * 2, &hb, 2);
                            }
                        }
                    }
            }
}

namespace {

// Host half of a layer upload: picks the power-of-two weight scale and packs the fragment
// records.  Pure function of its arguments (runs on worker threads at load time).
void packLayer(WeightGetter get, const void* ctx, int taps, int kReal, int kdim, int cout,
               int coutReal, int prec, std::vector<unsigned char>* host, float* accScale) {
    host->assign(tileWeightRecords(taps, kdim, cout, prec) * 16, 0);
    float scale = 1.f;
    if (prec == kF16x3 || isMx(prec)) {
        // power-of-two scale putting the largest |w| in [2^8, 2^9): hi and lo of every
        // weight that matters stay in f16's normal range; undone exactly by accScale
        float maxAbs = 0.f;
        for (int n = 0; n < coutReal; ++n)
            for (int k = 0; k < kReal; ++k)
                for (int t = 0; t < taps; ++t) maxAbs = std::fmax(maxAbs, std::fabs(get(ctx, n, k, t)));
        if (maxAbs > 0.f && std::isfinite(maxAbs)) {
            int e = 0;
            std::frexp(maxAbs, &e); // maxAbs = m * 2^e, m in [0.5, 1)
            scale = std::ldexp(1.0f, 9 - e);
        }
    }
    *accScale = 1.0f / scale;
    packTileWeights(get, ctx, taps, kReal, kdim, cout, prec, scale, host->data());
}

// The activation bound estimate (see pushConvMoment).
double estimateActivationBound(const NetView& nv) {
    std::vector<double> sc;
    std::vector<float> bi;
    double worst = 0.0, mean = 0.0, peak2 = 0.0;
    // feature planes are 0/1 (a handful of scalar planes in [0,1]): second moment <= the plane density, ~0.2
    foldBn(nv.stemBn, nv.F, nv.eps, &sc, &bi);
    pushConvMoment(nv.stemW, sc.data(), bi.data(), nv.F, nv.cin, 9, 0.2, &worst, &mean);
    peak2 = worst;
    double x2 = 0.5 * mean; // after the ReLU
    for (int k = 0; k < nv.blocks; ++k) {
        foldBn(nv.bn1[k], nv.F, nv.eps, &sc, &bi);
        pushConvMoment(nv.w1[k], sc.data(), bi.data(), nv.F, nv.F, 9, x2, &worst, &mean);
        peak2 = std::max(peak2, worst);
        const double y2 = 0.5 * mean;
        foldBn(nv.bn2[k], nv.F, nv.eps, &sc, &bi);
        pushConvMoment(nv.w2[k], sc.data(), bi.data(), nv.F, nv.F, 9, y2, &worst, &mean);
        peak2 = std::max(peak2, worst + x2); // the residual add
        x2 = 0.5 * (mean + x2);
    }
    return 6.0 * std::sqrt(peak2);
}

// 3x3 layers: BN folding on the caller's thread, fragment packing on worker threads.
void prepareTrunk(const NetView& nv, int prec, PreparedNet* W) {
    struct Job {
        std::vector<double> scale;
        const float* w;
        int cinReal, prec;
        PreparedLayer* L;
    };
    W->conv1.resize(nv.blocks); W->conv2.resize(nv.blocks);
    if (isMx(prec)) { W->conv1X3.resize(nv.blocks); W->conv2X3.resize(nv.blocks); }
    std::vector<Job> jobs;
    auto add = [&](const float* w, const float* bn, int cinReal, int kdim, PreparedLayer* L, PreparedLayer* Lx3) {
        Job j;
        foldBn(bn, nv.F, nv.eps, &j.scale, &L->bias);
        L->cin = kdim;
        j.w = w; j.cinReal = cinReal; j.prec = prec; j.L = L;
        jobs.push_back(j);
        if (isMx(prec)) { // the f16x3 copy of the trunk (small batches)
            Lx3->bias = L->bias; Lx3->cin = kdim;
            j.prec = kF16x3; j.L = Lx3;
            jobs.push_back(std::move(j));
        }
    };
    add(nv.stemW, nv.stemBn, nv.cin, W->cpad, &W->stem, &W->stemX3);
    for (int k = 0; k < nv.blocks; ++k) {
        add(nv.w1[k], nv.bn1[k], nv.F, nv.F, &W->conv1[k], isMx(prec) ? &W->conv1X3[k] : nullptr);
        add(nv.w2[k], nv.bn2[k], nv.F, nv.F, &W->conv2[k], isMx(prec) ? &W->conv2X3[k] : nullptr);
    }
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t i; (i = next.fetch_add(1)) < jobs.size();) {
            Job& j = jobs[i];
            Conv3Ctx c{j.w, j.scale.data(), j.cinReal};
            packLayer(conv3Get, &c, 9, j.cinReal, j.L->cin, nv.F, nv.F, j.prec, &j.L->image, &j.L->accScale);
        }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nthreads = std::min<size_t>(jobs.size(), std::max(1u, std::min(hw ? hw : 1u, 8u)));
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

} // namespace

int prepareNet(const void* blob, size_t size, int prec, int numChannels, bool m8Guard, PreparedNet* out, std::string* err) {
    NetView nv;
    int rc;
    if ((rc = parseBlob(blob, size, &nv, err))) return rc;
    if ((rc = checkSpecialised(nv, numChannels, err))) return rc;

    const int kc = inputChannelGranule(prec); // input channels are padded to whole chunks (kF16m8: chunk pairs)
    PreparedNet* W = out;
    *W = PreparedNet();
    W->F = nv.F; W->blocks = nv.blocks; W->vc = nv.vc; W->vh = nv.vh; W->cin = nv.cin;
    W->cpad = roundUp(nv.cin, kc);
    W->headsCout = roundUp(nv.vc + nv.pc, 64);
    W->fc1K = roundUp(81 * nv.vc, chunkChannels(headPrecision(prec)));
    W->params = nv.params;

    prepareTrunk(nv, prec, W);
    // heads: [value conv (BN folded) | policy conv | zero pad]
    {
        std::vector<double> scale;
        std::vector<float> bias;
        foldBn(nv.valBn, nv.vc, nv.eps, &scale, &bias);
        std::vector<float>& hb = W->heads.bias;
        hb.assign(W->headsCout, 0.f);
        for (int i = 0; i < nv.vc; ++i) hb[i] = bias[i];
        for (int i = 0; i < nv.pc; ++i) hb[nv.vc + i] = nv.polB[i];
        HeadsCtx c{nv.valW, scale.data(), nv.polW, nv.F, nv.vc, nv.pc};
        W->heads.cin = nv.F;
        packLayer(headsGet, &c, 1, nv.F, nv.F, W->headsCout, nv.vc + nv.pc, headPrecision(prec), &W->heads.image, &W->heads.accScale);
    }
    {
        W->fc1.bias.assign(nv.fc1B, nv.fc1B + nv.vh);
        Fc1Ctx c{nv.fc1W, nv.vc};
        W->fc1.cin = W->fc1K;
        packLayer(fc1Get, &c, 1, 81 * nv.vc, W->fc1K, nv.vh, nv.vh, headPrecision(prec), &W->fc1.image, &W->fc1.accScale);
    }
    W->actBound = estimateActivationBound(nv);
    W->outsideM8Window = prec == kF16m8 && W->actBound > 224.0 && m8Guard;
    W->fc2W.assign(nv.fc2W, nv.fc2W + (size_t)2 * nv.vh);
    W->fc2B.assign(nv.fc2B, nv.fc2B + 2);
    return NSG_OK;
}

// x, y, z with x and z swapped after every block: a block reads x, writes y, then reads y, adds x and writes z.
TrunkSequence trunkSequence(int blocks) {
    TrunkSequence q;
    int x = kBufAct0, y = kBufAct1, z = kBufAct2;
    q.steps.push_back(TrunkStep{kBufPlanes, kBufNone, x, kStem, 0});
    for (int k = 0; k < blocks; ++k) {
        q.steps.push_back(TrunkStep{x, kBufNone, y, kConv1, k});
        q.steps.push_back(TrunkStep{y, x, z, kConv2, k});
        std::swap(x, z);
    }
    q.outBuf = x;
    return q;
}

} // namespace nsg
