// launch_form.h -- which launch form a batch of the specialised ResNet path takes: the tile plans, the predicates of the
// persistent launches, and chooseLaunchForm(), the ONE statement of the decision.  Host-only integer arithmetic: no
// device, no environment, no evaluator (nsg_capi.hip fills a LaunchConfig and executes the LaunchForm it gets back).
// tests/golden/launch_forms.txt is the decision as a table (form_dump.cc, tests/test_launch_forms.py).
#ifndef NSG_LAUNCH_FORM_H
#define NSG_LAUNCH_FORM_H

#include <stddef.h>

namespace nsg {

// (the arithmetic of each precision: kernels/kernels.h)
enum Precision { kFp32 = 0, kFp16 = 1, kBf16 = 2, kF16x3 = 3, kF16m8 = 4, kF16m6 = 5 };
// the two split-precision trunk formats that run their correction terms on the MX instruction
constexpr bool isMx(int prec) { return prec == kF16m8 || prec == kF16m6; }
// Precision of the 1x1 heads / value MLP of an evaluator whose trunk runs at `prec`.
inline int headPrecision(int prec) { return isMx(prec) ? (int)kF16x3 : prec; }

// What the kernels (kernels/kernels.h) and the host-only weight preparation (net_prepare.h) both read of a precision.
constexpr int kM8WLoShift = 10;  // weight record  = e4m3(w_lo * 2^10)
constexpr int kM8WHiShift = -2;  // weight record  = e4m3(w_hi * 2^-2); both products carry 2^-10
// Bytes one activation channel occupies (a kF16x3 pair is 2 + 2 bytes, kF16m8 2 + 1 + 1).
inline int elemSize(int prec) { return (prec == kFp32 || prec == kF16x3 || isMx(prec)) ? 4 : 2; }
// Channels per 128-byte K chunk of the trunk convolution.
inline int chunkChannels(int prec) { return 128 / elemSize(prec); }
// Packed weight records per (chunk, tap): the two K halves, or for kF16x3 (w_hi, w_lo)
// -- w_hi serves both of its products from registers.
inline int recordsPerTap(int) { return 2; }
// 1-KiB-per-fragment weight records per channel chunk.  kF16m8 (chunks go in pairs A, B): per
// tap one f16 record for each chunk (w_hi) plus two records holding the 32 fp8 bytes per lane of
// the MX operand (k-group g: chunk g>>1, g&1 ? e4m3(w_hi) : e4m3(w_lo)) -- 4 per tap and pair.
inline int recordsPerChunk(int taps, int prec) {
    return isMx(prec) ? 2 * taps : taps * recordsPerTap(prec);
}
// Input channels are padded to whole chunks; kF16m8 to whole chunk pairs.
inline int inputChannelGranule(int prec) { return isMx(prec) ? 2 * chunkChannels(prec) : chunkChannels(prec); }
// Fragment-ordered weights: number of 16-byte lane records INCLUDING the
// trailing zero slabs the kernel's prefetch may touch.
inline size_t tileWeightRecords(int taps, int kdim, int cout, int prec) {
    const int nkc = kdim / chunkChannels(prec);
    const size_t nft = (size_t)(cout / 16);
    if (prec == kF16m6) // packed MX slabs: per tap and chunk pair nft x (1024 + 1024 + 1600) bytes (mfma_tile.h, kPackX)
        return (size_t)(nkc / 2) * taps * nft * 3648 / 16 + 16 * nft * 64;
    return ((size_t)nkc * recordsPerChunk(taps, prec) + 16) * nft * 64; // + 16 zero records: deepest prefetch
}
// K slices of the value MLP's first layer (launchDense, kernels/kernels.h).
inline int denseSplits(int kdim, int prec) {
    const int nkc = kdim / chunkChannels(prec);
    for (int s = 9; s > 1; --s)
        if (nkc % s == 0) return s;
    return 1;
}

struct ConvPlan {
    int nb;      // boards per workgroup
    int nfrag;   // 16-channel output fragments per wave (fixed at pack time)
    int nwaves;  // waves per workgroup
    int msplit = 1; // wave groups that split the tile's row fragments between them (small one-board tiles: 2)
    int ksplit = 1; // kF16m8 one-board tiles: waves of a channel group that split the input-channel chunk pairs between them
    int sslab = 1;  // MX two-board tiles at mid batches: waves of a channel group that split every chunk pair's slabs between them
};
constexpr int kNfrag = 4; // every packed tensor uses 4 fragments (64 channels) per wave

// Tuning overrides (0 = automatic), read from NSG_CONV_NB / _NWAVES / _NFRAG when an
// evaluator is created.
struct ConvTuning {
    int nb = 0, nwaves = 0, nfrag = 0, msplit = 0; // msplit: NSG_CONV_MSPLIT (1 = never split rows)
    int splitBatch = 1;    // NSG_SPLIT_BATCH=0: never run a batch as a full part + remainder
    int splitBatchMax3 = 9;  // NSG_SPLIT_BATCH_MAX: largest batch, in quarters of the CU count, that starts with a full chip of two-board tiles
    int rowsplit8Max = -1; // NSG_ROWSPLIT8_MAX_BATCH: largest batch whose four-way K split also splits the rows over two workgroups (-1: CUs / 8)
    int ksplit3 = 1;       // NSG_KSPLIT3=0: 192-channel nets keep the plans they had before the three-way K split
    int slabSplit = 0;     // NSG_SLAB_SPLIT=1: slab-split two-board tiles at mid batches (measured 8-11 % slower than the plans they would replace: opt-in)
    bool fullTilesOnly = false; // kF16m8: 4 fragments per wave at every batch size
};

// Picks a tile configuration for (batch, cout).
ConvPlan chooseConvPlan(int batch, int cout, int computeUnits, const ConvTuning& tune = ConvTuning());

// Persistent trunk (launchTrunk): needs cout == nwaves*64 (one workgroup covers all output channels of its boards).
bool canRunTrunk(int cout, const ConvPlan& plan);

// Cooperative trunk (launchCoopTrunk): the K-split plans of an f16m6 evaluator.  *firstSeparate: the stem has fewer chunk
// pairs than the plan splits K by and runs another kernel (its own launch, ahead of the cooperative one, which then
// starts at the first residual layer).
bool canRunCoopTrunk(int cout, int stemKdim, int prec, const ConvPlan& plan, bool* firstSeparate = nullptr);
int coopMembers(int cout, const ConvPlan& plan); // workgroups per board
// Every workgroup of the cooperative launch resident at once.  sameXcd (the kernels' tile::kCoopSameXcd): blockIdx.x
// picks the XCD (workgroups are dealt round-robin, gridDim.x is padded to a multiple of eight), so the members of
// ceil(boards / 8) boards must fit ONE XCD's share of the CUs.
bool coopFits(int boards, int members, int computeUnits, bool sameXcd);

// Team trunk (launchTeamTrunk): workgroups per board of a launch of `boards` boards of a `channels`-wide trunk on a
// device of `computeUnits` CUs (every member must be resident at once); 0: no team size fits.  forceRowGroups > 0: at
// most that many row groups.
constexpr int kTeamMaxBoards = 16;
int teamMembers(int boards, int channels, int computeUnits, int forceRowGroups);

// Everything the decision reads, as plain values (nsg_capi.hip, launchConfigOf).
struct LaunchConfig {
    int prec = kFp32;         // the evaluator's precision
    int F = 0, cpad = 0;      // trunk channels, padded input channels of the stem
    int blocks = 0;           // residual blocks
    int trunkLayerCount = 0;  // entries of the persistent-trunk layer list
    int cus = 0;              // compute units of the device
    int numChains = 2;        // NSG_CHAINS
    ConvTuning tuning;
    int useTrunkKernel = -1;  // NSG_TRUNK_KERNEL: 1 wherever the plan allows, 0 never, -1 where it measured faster
    int chainMinBatch = 0;    // NSG_CHAIN_MIN_BATCH; 0 = more 2-board tiles than CUs
    int chainDelayUs = 0;     // NSG_CHAIN_DELAY_US
    int teamMaxBatch = kTeamMaxBoards; // NSG_TEAM_MAX_BATCH
    int teamForceRowGroups = 0;        // NSG_TEAM_MEMBERS / 16
    int coopForced = 0;       // NSG_COOP_TRUNK=1: wherever a plan allows it; unset: where it measured faster
    int ksplit4Max = -1;      // NSG_KSPLIT4_MAX_BATCH: largest batch that takes the four-way K split (-1: CUs / 4)
    bool coopSameXcd = true;  // tile::kCoopSameXcd
    bool outsideM8Window = false; // an MX evaluator whose network left the fixed-scale window runs as kF16x3
    bool teamAvailable = false;   // a team layer list exists and no team launch has given up
    bool coopAvailable = false;   // the cooperative trunk is enabled and its flags and status word exist
};

// The launch form of one batch.
struct LaunchForm {
    enum Kind { Team, Coop, WholeTrunk, Parts, Chains, Single };
    struct Part { int off, count; ConvPlan plan; int trunkPrec; };
    Kind kind = Single;
    // the tile plan; Team: a description (16 weight fragments x row groups per board, K over 8 waves); Parts: parts[0]'s
    ConvPlan plan{0, 0, 0};
    int members = 0;        // Team, Coop: workgroups per board
    bool stemFirst = false; // Coop: the stem is its own launch ahead of the cooperative one
    int nParts = 0;         // Parts: a full part with the plan of the size below + the remainder with ITS plan
    Part parts[3] = {};
    int chains = 1;         // concurrent launch chains (Parts: nParts)
    int per = 0;            // Chains: boards per chain, whole 2-board tiles
    bool stagger = false;   // Chains: every tile resident at once, so a phase shift between the chains can pay
    int trunkPrec = kFp32;  // the precision the trunk (of the first part) runs in: kF16x3 where an MX plan has no MX form
    int trunkLaunchesPerFwd = 0; // launches between the profiling bracket's trunk events
};

// The tile plan of a batch of B boards (precision, channel count, CU count, tuning).
ConvPlan planForBatch(const LaunchConfig& c, int B);
LaunchForm chooseLaunchForm(const LaunchConfig& c, int B);

} // namespace nsg

#endif
