// net_prepare.h -- everything a load of the specialised ResNet path computes on the host: the NSGW v1 parser, BN folding
// in double, the power-of-two weight scale, the re-layout into MFMA fragment order, the activation-bound estimate and
// the buffer rotation of the 3x3 layers.  Host-only arithmetic on host memory: no device, no environment, no evaluator
// (nsg_capi.hip uploads the PreparedNet it gets back, layer by layer).  tests/golden/net_prepare.txt pins its output
// (weights_dump.cc, tests/test_net_prepare.py).
#ifndef NSG_NET_PREPARE_H
#define NSG_NET_PREPARE_H

#include "launch_form.h" // Precision and what each precision's records and chunks measure

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace nsg {

// Parsed view of an NSGW v1 blob (DESIGN.md "Weight file").
struct NetView {
    int cin, F, blocks, pc, vc, vh;
    float eps;
    const float* stemW; const float* stemBn;
    std::vector<const float*> w1, bn1, w2, bn2;
    const float* polW; const float* polB;
    const float* valW; const float* valBn;
    const float* fc1W; const float* fc1B;
    const float* fc2W; const float* fc2B;
    uint64_t params;
};
// Both return NSG_OK or NSG_E_FORMAT with the message in *err.
int parseBlob(const void* blob, size_t size, NetView* nv, std::string* err);
// What the specialised loader refuses in a parsed blob: an ONNX model it refuses goes to the general graph path instead.
int checkSpecialised(const NetView& nv, int numChannels, std::string* err);

// Host-side re-layout.  get(n, k, tap) returns the (already BN-folded) weight
// of output channel n, input channel k (< kReal), tap (< taps); input
// channels [kReal, kdim) are zero padding, as are output channels for which
// get() returns 0.
typedef float (*WeightGetter)(const void* ctx, int n, int k, int tap);
// `scale` multiplies every weight before conversion (a power of two chosen per
// tensor for kF16x3 so hi and lo stay in f16's normal range; the kernel undoes it
// exactly through accScale = 1/scale).  dst holds tileWeightRecords() x 16 bytes.
void packTileWeights(WeightGetter get, const void* ctx, int taps, int kReal,
                     int kdim, int cout, int prec, float scale, void* dst);

// One layer as the device will hold it.
struct PreparedLayer {
    std::vector<unsigned char> image; // fragment-ordered weights
    std::vector<float> bias;          // f32 [cout], zero beyond the real output channels
    int cin = 0;                      // padded input channels
    float accScale = 1.f;             // 1 / (power-of-two weight scale), split precisions only
};

struct PreparedNet {
    int F = 0, blocks = 0, vc = 0, vh = 0, cin = 0, cpad = 0, headsCout = 0, fc1K = 0;
    uint64_t params = 0;
    // Estimated largest trunk activation and, for kF16m8, whether it leaves the window its fixed-scale e4m3 copies
    // cover: then every batch runs the kF16x3 copy of the trunk.
    double actBound = 0.0;
    bool outsideM8Window = false;
    PreparedLayer stem;
    std::vector<PreparedLayer> conv1, conv2;
    // an MX precision also holds the trunk in kF16x3 form, for the batches without an MX plan
    PreparedLayer stemX3;
    std::vector<PreparedLayer> conv1X3, conv2X3;
    PreparedLayer heads; // [value conv (BN folded) | policy conv | zero pad]
    PreparedLayer fc1;
    std::vector<float> fc2W, fc2B;
};

// Parses and checks an NSGW v1 blob for an evaluator of `numChannels` input planes and prepares every layer for
// `prec`; the 3x3 layers are packed by up to 8 threads.  m8Guard: let a kF16m8 net whose bound leaves the window fall
// back to its kF16x3 copy (NSG_M8_GUARD).  NSG_OK, or NSG_E_FORMAT with the message in *err.
int prepareNet(const void* blob, size_t size, int prec, int numChannels, bool m8Guard, PreparedNet* out, std::string* err);

// The 3x3 layers of a net of `blocks` residual blocks in launch order, and the buffers they rotate through.
enum TrunkBuffer { kBufNone = -1, kBufPlanes = 0, kBufAct0 = 1, kBufAct1 = 2, kBufAct2 = 3 };
enum TrunkWeights { kStem = 0, kConv1 = 1, kConv2 = 2 };
struct TrunkStep {
    int in, residual, out; // TrunkBuffer; residual: kBufNone but for a block's second layer
    int weights, block;    // TrunkWeights; conv1[block] / conv2[block]
};
struct TrunkSequence {
    std::vector<TrunkStep> steps; // 1 + 2 * blocks
    int outBuf = kBufAct0;        // the buffer the last step writes
};
TrunkSequence trunkSequence(int blocks);

} // namespace nsg

#endif
