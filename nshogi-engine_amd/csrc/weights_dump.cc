// weights_dump -- what the host-only weight preparation (net_prepare.h) makes of a fixed set of generated nets, as text
// (tests/test_net_prepare.py compares it with tests/golden/net_prepare.txt).  Links net_prepare.cc alone.
//
//   == net F= blocks= gain= prec=        one section per net and precision.  The nets: 45 input planes (so that cpad >
//                                        cin at every granule), pc = 27, vc = 3, vh = 64, F = 64 and 128 (the kF16m6
//                                        slab groups fragments by four: 128 gives a second group), 0 to 2 blocks, BN
//                                        gains x1, and one net with gains x32 whose bound leaves the kF16m8 window
//   dims ...                             the PreparedNet's dims
//   actBound outsideM8Window             the bound as a hex float
//   layer cin bytes accScale image bias  per layer in upload order: padded input channels, size of the packed image,
//                                        accScale as a hex float, 64-bit FNV-1a of the image and of the bias
//   == sequence blocks=                  the 3x3 layers' buffers (trunkSequence): in, residual, out, weights per step
//   == refusals                          code and message of every blob or shape the loader refuses
#include "net_prepare.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace nsg;

namespace {

const char* const kPrecNames[] = {"fp32", "fp16", "bf16", "f16x3", "f16m8", "f16m6"};

// Values from an integer LCG (Knuth's MMIX constants), exact in f32: no std:: distribution, whose output differs
// between libraries.
struct Lcg {
    uint64_t s;
    float unit() { // a multiple of 2^-23 in [-1, 1)
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (float)((int)(s >> 40) - (1 << 23)) / (float)(1 << 23);
    }
};

struct Dims { int cin, F, blocks, pc, vc, vh; };

std::vector<unsigned char> makeBlob(const Dims& d, float gain, uint64_t seed) {
    std::vector<float> f;
    Lcg r{seed};
    auto weights = [&](size_t n, float amp) { for (size_t i = 0; i < n; ++i) f.push_back(r.unit() * amp); };
    auto bn = [&](int n) { // gamma, beta, mean, variance
        for (int i = 0; i < n; ++i) f.push_back((1.0f + 0.5f * r.unit()) * gain);
        weights(n, 0.25f);
        weights(n, 0.25f);
        for (int i = 0; i < n; ++i) f.push_back(1.0f + 0.5f * r.unit());
    };
    weights((size_t)d.F * d.cin * 9, 0.125f); bn(d.F);
    for (int k = 0; k < 2 * d.blocks; ++k) { weights((size_t)d.F * d.F * 9, 0.0625f); bn(d.F); }
    weights((size_t)d.pc * d.F, 0.125f); weights(d.pc, 0.25f);
    weights((size_t)d.vc * d.F, 0.125f); bn(d.vc);
    weights((size_t)d.vh * d.vc * 81, 0.125f); weights(d.vh, 0.25f);
    weights((size_t)2 * d.vh, 0.125f); weights(2, 0.25f);
    std::vector<unsigned char> blob(64 + f.size() * 4, 0);
    const float eps = 1e-5f;
    const uint32_t h[7] = {1, (uint32_t)d.cin, (uint32_t)d.F, (uint32_t)d.blocks, (uint32_t)d.pc, (uint32_t)d.vc, (uint32_t)d.vh};
    memcpy(blob.data(), "NSGW", 4);
    memcpy(blob.data() + 4, h, sizeof(h));
    memcpy(blob.data() + 4 + sizeof(h), &eps, 4);
    memcpy(blob.data() + 64, f.data(), f.size() * 4);
    return blob;
}

uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001b3ull;
    return h;
}

void printLayer(const std::string& name, const PreparedLayer& L) {
    if (L.image.empty()) return; // (the kF16x3 copies of a precision that is not MX)
    printf("%s cin=%d bytes=%zu accScale=%a image=%016llx bias=%016llx\n", name.c_str(), L.cin, L.image.size(), (double)L.accScale,
           (unsigned long long)fnv1a(L.image.data(), L.image.size()),
           (unsigned long long)fnv1a(L.bias.data(), L.bias.size() * 4));
}

void dumpNet(const Dims& d, int gain) {
    const std::vector<unsigned char> blob = makeBlob(d, (float)gain, 1000u * d.F + 10u * d.blocks + gain);
    for (int prec = kFp32; prec <= kF16m6; ++prec) {
        printf("== net F=%d blocks=%d gain=%d prec=%s\n", d.F, d.blocks, gain, kPrecNames[prec]);
        PreparedNet N;
        std::string err;
        const int rc = prepareNet(blob.data(), blob.size(), prec, d.cin, true, &N, &err);
        if (rc) { printf("error %d: %s\n", rc, err.c_str()); continue; }
        printf("dims F=%d blocks=%d vc=%d vh=%d cin=%d cpad=%d headsCout=%d fc1K=%d params=%llu\n", N.F, N.blocks, N.vc, N.vh,
               N.cin, N.cpad, N.headsCout, N.fc1K, (unsigned long long)N.params);
        printf("actBound=%a outsideM8Window=%d\n", N.actBound, (int)N.outsideM8Window);
        printLayer("stem", N.stem);
        printLayer("stemX3", N.stemX3);
        for (int k = 0; k < N.blocks; ++k) {
            const std::string i = "[" + std::to_string(k) + "]";
            printLayer("conv1" + i, N.conv1[k]);
            if (isMx(prec)) printLayer("conv1X3" + i, N.conv1X3[k]);
            printLayer("conv2" + i, N.conv2[k]);
            if (isMx(prec)) printLayer("conv2X3" + i, N.conv2X3[k]);
        }
        printLayer("heads", N.heads);
        printLayer("fc1", N.fc1);
        printf("fc2 w=%016llx b=%016llx\n", (unsigned long long)fnv1a(N.fc2W.data(), N.fc2W.size() * 4),
               (unsigned long long)fnv1a(N.fc2B.data(), N.fc2B.size() * 4));
    }
}

void refusal(const char* what, std::vector<unsigned char> blob, int numChannels) {
    PreparedNet N;
    std::string err;
    const int rc = prepareNet(blob.data(), blob.size(), kFp32, numChannels, true, &N, &err);
    printf("%s: %d %s\n", what, rc, err.c_str());
}

} // namespace

int main() {
    for (int F : {64, 128})
        for (int blocks = 0; blocks <= 2; ++blocks) dumpNet(Dims{45, F, blocks, 27, 3, 64}, 1);
    dumpNet(Dims{45, 64, 1, 27, 3, 64}, 32);

    static const char* const kBufNames[] = {"-", "planes", "act0", "act1", "act2"};
    static const char* const kWeightNames[] = {"stem", "conv1", "conv2"};
    for (int blocks = 0; blocks <= 3; ++blocks) {
        const TrunkSequence q = trunkSequence(blocks);
        printf("== sequence blocks=%d ends in %s\n", blocks, kBufNames[q.outBuf + 1]);
        for (const TrunkStep& t : q.steps)
            printf("%s[%d] in=%s residual=%s out=%s\n", kWeightNames[t.weights], t.block, kBufNames[t.in + 1],
                   kBufNames[t.residual + 1], kBufNames[t.out + 1]);
    }

    printf("== refusals\n");
    const Dims good{45, 64, 0, 27, 3, 64};
    const std::vector<unsigned char> blob = makeBlob(good, 1.f, 1);
    auto with = [&](size_t off, uint32_t v) { std::vector<unsigned char> b = blob; memcpy(b.data() + off, &v, 4); return b; };
    refusal("short blob", std::vector<unsigned char>(blob.begin(), blob.begin() + 63), 45);
    refusal("bad magic", with(0, 0x5847534eu), 45);
    refusal("version 2", with(4, 2), 45);
    refusal("vc = 0", with(24, 0), 45);
    refusal("one float short", std::vector<unsigned char>(blob.begin(), blob.end() - 4), 45);
    refusal("46 planes", blob, 46);
    refusal("pc = 26", makeBlob(Dims{45, 64, 0, 26, 3, 64}, 1.f, 1), 45);
    refusal("F = 96", makeBlob(Dims{45, 96, 0, 27, 3, 64}, 1.f, 1), 45);
    refusal("vh = 32", makeBlob(Dims{45, 64, 0, 27, 3, 32}, 1.f, 1), 45);
    return 0;
}
