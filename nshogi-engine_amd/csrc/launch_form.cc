// launch_form.cc -- the launch form of a batch (launch_form.h): pure host arithmetic.
#include "launch_form.h"

#include <algorithm>

namespace nsg {

ConvPlan chooseConvPlan(int batch, int cout, int computeUnits, const ConvTuning& tune) {
    ConvPlan p;
    const int groups = cout / (kNfrag * 16); // 64-channel weight groups
    // Full tiles: 4 fragments (64 channels) per wave, widest workgroup that divides
    // the channel groups (its waves share one LDS image of the input tile).
    p.nfrag = kNfrag;
    // A full tile's wave needs the whole register file of its SIMD, so a CU hosts
    // 4 waves: one 4-wave workgroup or two 2-wave workgroups fill it, a 3-wave
    // workgroup leaves a SIMD idle (40x384: 2-wave groups +17 % over 3-wave groups).
    p.nwaves = (groups % 4 == 0) ? 4 : (groups % 2 == 0) ? 2 : (groups % 3 == 0) ? 3 : 1;
    // Two boards per workgroup waste less of the last 16-row fragment (162 -> 176
    // rows vs 81 -> 96) but halve the grid: use them once the grid still covers
    // most of the chip.
    const int simds = computeUnits * 4;
    auto waves = [&](int nb, int nfrag) { return ((batch + nb - 1) / nb) * (cout / (16 * nfrag)); };
    p.nb = (waves(2, 4) * 4 >= simds * 3) ? 2 : 1;
    // Small batches: a wave's run time is set by fragments-per-wave x K, so when
    // the grid leaves SIMDs idle give each wave fewer channels (2 or 1 fragments,
    // four waves per workgroup) until the chip is covered.
    if (waves(p.nb, 4) * 4 < simds * 3) {
        for (int nf : {2, 1}) {
            for (int nb : {2, 1}) {
                if (cout % (4 * nf * 16) != 0) continue;
                if (waves(nb, nf) * 4 >= simds * 3 || (nf == 1 && nb == 1)) {
                    p.nb = nb; p.nfrag = nf; p.nwaves = 4;
                    goto chosen;
                }
            }
        }
    }
chosen:
    // A small-tile plan whose grid needs a second round of workgroups (more workgroups than CUs:
    // the CUs that get two take twice as long as the rest) loses to one full one-board tile per
    // board when those tiles fit in one round: B = 129..191 on 256 CUs (129: 2.13 -> 1.9 ms).
    if (p.nfrag < 4 && tune.nfrag == 0 && tune.nb == 0) {
        const int perBoard = cout / (16 * p.nfrag * 4); // workgroups per tile of the small plan
        const int nwg = ((batch + p.nb - 1) / p.nb) * perBoard;
        if (nwg > computeUnits && batch <= computeUnits && 2 * batch > computeUnits) {
            p.nb = 1; p.nfrag = 4;
            p.nwaves = (groups % 4 == 0) ? 4 : (groups % 2 == 0) ? 2 : (groups % 3 == 0) ? 3 : 1;
        }
    }
    const int kEnvNb = tune.nb, kEnvNwaves = tune.nwaves, kEnvNfrag = tune.fullTilesOnly ? 4 : tune.nfrag;
    if (kEnvNb == 1 || kEnvNb == 2) p.nb = kEnvNb;
    if (kEnvNfrag) {
        const int v = kEnvNfrag;
        if (v == 1 || v == 2) { p.nfrag = v; p.nwaves = 4; }
        if (v == 4) { p.nfrag = 4; p.nwaves = (groups % 4 == 0) ? 4 : (groups % 2 == 0) ? 2 : (groups % 3 == 0) ? 3 : 1; }
    }
    if (kEnvNwaves >= 1 && kEnvNwaves <= 4 && groups % kEnvNwaves == 0 && p.nfrag == kNfrag) p.nwaves = kEnvNwaves;
    // One board, one fragment per wave: every wave reads every row fragment from LDS for one MFMA
    // each (LDS-bound).  Two wave groups on half the rows each with two fragments per wave cover
    // the same 64 channels per workgroup with half the LDS reads.
    if (p.nb == 1 && p.nfrag == 1 && p.nwaves == 4 && tune.msplit != 1 && kEnvNfrag == 0) {
        p.nfrag = 2;
        p.msplit = 2;
    }
    return p;
}

bool canRunTrunk(int cout, const ConvPlan& plan) {
    return plan.nfrag == kNfrag && plan.msplit == 1 && plan.ksplit == 1 && plan.sslab == 1 && cout == plan.nwaves * 64 &&
           (plan.nwaves == 4 || plan.nwaves == 3);
}

bool canRunCoopTrunk(int cout, int stemKdim, int prec, const ConvPlan& plan, bool* firstSeparate) {
    if (prec != kF16m6 || plan.nb != 1 || plan.nfrag != kNfrag || plan.sslab != 1) return false;
    const bool rows = plan.msplit == 1 || plan.msplit == 2 || plan.msplit == 3 || plan.msplit == 6;
    bool sep = false, ok = false;
    if (cout == 256 && plan.nwaves == 4 && plan.ksplit == 2 && plan.msplit == 1) { ok = true; sep = !(stemKdim % 128 == 0 && stemKdim <= 256); }
    else if (cout == 256 && plan.nwaves == 4 && plan.ksplit == 4 && rows) { ok = true; sep = !(stemKdim == 256); }
    else if (cout == 192 && plan.nwaves == 3 && plan.ksplit == 3 && rows) { ok = true; sep = !(stemKdim == 192); }
    if (firstSeparate) *firstSeparate = sep;
    return ok;
}

int coopMembers(int cout, const ConvPlan& plan) {
    const bool rowWG = plan.msplit > 1 && plan.ksplit > 1;
    const int chanGroups = plan.nwaves / (rowWG ? plan.ksplit : plan.msplit * plan.ksplit);
    return cout / (chanGroups * plan.nfrag * 16) * (rowWG ? plan.msplit : 1);
}

bool coopFits(int boards, int members, int computeUnits, bool sameXcd) {
    if (sameXcd) return (long)((boards + 7) / 8) * members <= computeUnits / 8;
    return (long)boards * members <= computeUnits;
}

// Members per board = weight fragments (trunk channels / 16: 16 or 12) x row groups, as many as fit the chip's CUs (a
// member owns a CU: 147 KB of LDS): with 16 fragments on 256 CUs 96 (one row fragment each) for one or two boards,
// 48 (two) for three to five, 32 (three) for six to eight, 16 (the whole board) for nine to sixteen.  Measured, evals/s
// at 2 / 3 / 4 / 5 boards: 96 members 11.2k / - / - / -, 48 members 9.2k / 13.5k / 17.7k / 21.6k, 32 members 7.8k /
// 11.5k / 15.4k / 18.8k; 6 / 8 boards: 32 members 22.5k / 29.3k, 16 members 16.2k / 21.3k
// (profiles/r03/g_team_trunk_members.txt).  Every member must be resident at once (they wait for each other): a
// device with fewer CUs (a partition, a CU mask) gets the largest team that fits, or none -- 0 -- and the caller
// runs the per-layer kernels.  `forceRowGroups` (NSG_TEAM_MEMBERS / 16) asks for fewer row groups than that.
int teamMembers(int boards, int channels, int computeUnits, int forceRowGroups) {
    const int nj = channels / 16;
    for (int rg : {6, 3, 2, 1}) {
        if (forceRowGroups > 0 && rg > forceRowGroups) continue;
        if ((long)boards * nj * rg <= computeUnits) return nj * rg;
    }
    return 0;
}

namespace {

// no NSG_CONV_* override asks for a particular per-layer plan
bool automaticPlan(const ConvTuning& t) { return t.nb == 0 && t.nfrag == 0 && t.nwaves == 0 && t.msplit == 0; }
// ... and no chain knob for a particular chaining
bool automaticChains(const LaunchConfig& c) { return c.chainMinBatch <= 0 && c.chainDelayUs == 0; }

// kF16m8 runs full tiles only; smaller launch plans use the kF16x3 copy of the trunk
int trunkPrecisionOf(const LaunchConfig& c, const ConvPlan& plan) {
    return isMx(c.prec) && (plan.nfrag != 4 || c.outsideM8Window) ? (int)kF16x3 : c.prec;
}

} // namespace

ConvPlan planForBatch(const LaunchConfig& c, int B) {
    const ConvTuning& tuning = c.tuning;
    const int F = c.F;
    const long cus = c.cus;
    ConvPlan plan = chooseConvPlan(B, F, c.cus, tuning);
    // kF16m8 keeps four image buffers in LDS (125 KB for two boards): a CU holds one two-board
    // workgroup, so where the channel count only allows two-wave workgroups (F = 384) one-board
    // tiles (74 KB) keep all four SIMDs busy with two workgroups per CU
    // (an F16M8 evaluator whose network left the fixed-scale window runs as kF16x3: none of the MX plans apply)
    const bool mx = isMx(c.prec) && !c.outsideM8Window;
    if (mx && plan.nfrag == 4 && plan.nwaves <= 2 && tuning.nb == 0) plan.nb = 1;
    // Mid batches -- the engine's default batch of 128 and its benchmark's 60..159 -- run kF16m8
    // one-board tiles whose four waves are two row groups x two 64-channel groups (two workgroups per
    // board) wherever those fill more than half the CUs in one round of workgroups
    if (mx && plan.nfrag != 4 && F % 128 == 0 && tuning.nfrag == 0 && tuning.msplit != 1) {
        const long wgM8 = (long)B * (F / 128);
        if (F == 256 && c.cpad == 128 && tuning.msplit != 2 &&
            (c.ksplit4Max >= 0 ? B <= c.ksplit4Max : (long)B * 4 <= cus)) {
            // small batches: four workgroups per board, each one 64-channel group whose four waves take one chunk
            // pair apiece (K split by four, whole board resident in LDS)
            plan.nb = 1; plan.nfrag = 4; plan.nwaves = 4; plan.msplit = 1; plan.ksplit = 4;
            // ... and while eight workgroups per board still fit the chip in one round, the rows are split
            // over two workgroups as well (NSG_ROWSPLIT8_MAX_BATCH, read when the evaluator is created)
            // -- two, three or six row groups of three, two or one fragment: as many as fit the chip in one round
            const int k8max = tuning.rowsplit8Max;
            if (k8max >= 0 ? B <= k8max : true) {
                // (three row groups = twelve workgroups per board: three boards' do not fit an XCD, so 17-21 boards have
                // no cooperative form with them; two row groups as ONE cooperative launch beat three as per-layer
                // launches by 2...9 %: profiles/r04/zn_*.  Without the cooperative trunk -- switched off, the device's
                // lock lost, after a give-up -- three row groups it is.)
                const bool coop = c.coopAvailable && c.prec == kF16m6;
                if ((long)B * 24 <= cus) plan.msplit = 6;
                else if ((long)B * 12 <= cus && !coop) plan.msplit = 3;
                else if ((long)B * 8 <= cus) plan.msplit = 2;
            }
        } else
        if (wgM8 <= cus && wgM8 * 2 > cus) { // (measured: 1.17-1.29 ms for every B in 65..128; kF16x3 plans 1.26-1.54 ms)
            plan.nb = 1; plan.nfrag = 4; plan.nwaves = 4; plan.msplit = 2;
            // K split instead of the row split where the whole board fits in LDS (<= 256 channels) and both
            // the stem's and the trunk's chunk pairs halve evenly; NSG_CONV_MSPLIT=2 keeps the row split
            const int stemChunks = c.cpad / 32, trunkChunks = F / 32;
            if (tuning.msplit != 2 && trunkChunks <= 8 && trunkChunks % 4 == 0 && stemChunks % 4 == 0 && stemChunks <= 8) {
                plan.msplit = 1;
                plan.ksplit = 2;
            }
        }
    }

    // 192 channels (BASELINE configs[1]: 10x192 at batch 64) are three chunk pairs: up to CUs/3 boards run one
    // 64-channel group per workgroup whose three waves take one pair each, all of the board's chunk tiles resident
    // (the four-way K split of the 256-channel nets, three ways), the rows over as many workgroups as fit one round.
    if (mx && F == 192 && c.cpad == 128 && tuning.nb == 0 && tuning.nfrag == 0 && tuning.nwaves == 0 &&
        tuning.msplit != 2 && tuning.ksplit3 != 0) {
        if ((long)B * 3 <= cus) {
            plan = ConvPlan{};
            plan.nb = 1; plan.nfrag = 4; plan.nwaves = 3; plan.msplit = 1; plan.ksplit = 3;
            if (tuning.msplit != 1) {
                if ((long)B * 18 <= cus) plan.msplit = 6;
                else if ((long)B * 9 <= cus) plan.msplit = 3;
                else if ((long)B * 6 <= cus) plan.msplit = 2;
            }
        }
    }

    // Mid batches, MX arithmetic: two-board tiles of ONE 64-channel group (or two) per workgroup whose waves split
    // every chunk pair's slabs between them (mfma_tile.h, OwnSeq) -- where one workgroup per (two boards, group)
    // fills more than half the CUs in one round and the four-workgroups-per-board K split does not apply.  Against
    // the one-board tiles it replaces: a workgroup streams half the weights for twice the boards, and the
    // two-board tile's edge-packed rows need 19 % fewer matrix instructions per board.  MEASURED SLOWER (round 3,
    // profiles/r03/d_*): 113k against 123k evals/s at 128 boards, 134k against 151k at 256 -- a wave's share of a
    // chunk pair is 4.2k cycles of MFMAs, and the pair's two tile round trips, its barrier and the one-slab lead of
    // the MX weight records no longer hide behind it.  Opt-in: NSG_SLAB_SPLIT=1.
    if (mx && tuning.slabSplit == 1 && automaticPlan(tuning) && !(plan.ksplit == 4)) {
        const long tiles = (B + 1) / 2;
        for (int ss : {4, 2}) {
            if (F % (256 / ss) != 0) continue;
            const long wgs = tiles * (F / (256 / ss));
            if (wgs <= cus && wgs * 2 > cus) {
                plan = ConvPlan{};
                plan.nb = 2; plan.nfrag = 4; plan.nwaves = 4; plan.sslab = ss;
                break;
            }
        }
    }

    return plan;
}

LaunchForm chooseLaunchForm(const LaunchConfig& c, int B) {
    LaunchForm f;
    const int F = c.F, cus = c.cus;
    // the tile plan is chosen for the whole batch: all chains run concurrently
    const ConvPlan plan = planForBatch(c, B);
    const bool mx = isMx(c.prec) && !c.outsideM8Window;
    const bool automatic = automaticPlan(c.tuning);
    f.plan = plan;
    f.trunkPrec = c.prec;
    f.trunkLaunchesPerFwd = 1; // (the persistent forms)

    // The smallest batches: every 3x3 layer in one persistent launch, a board per team of 16-96 workgroups
    // (kernels/team_trunk.hip), when no tuning override asks for a particular per-layer plan.
    if (automatic && c.useTrunkKernel != 1 && c.teamAvailable && B <= c.teamMaxBatch)
        f.members = teamMembers(B, F, cus, c.teamForceRowGroups);
    if (f.members > 0) {
        f.kind = LaunchForm::Team;
        f.plan = ConvPlan{};
        f.plan.nb = 1; f.plan.nfrag = 1; f.plan.nwaves = 8; f.plan.ksplit = 8; // 16 weight fragments x 2 or 6 row groups per board, K over 8 waves
        f.plan.msplit = f.members / (F / 16); // row groups
        f.trunkPrec = kF16x3;
        return f;
    }

    // Mid batches on the K-split plans: the cooperative trunk, when every workgroup of its grid is resident at once
    if (c.coopAvailable && automatic && c.useTrunkKernel != 1 && mx && automaticChains(c) &&
        canRunCoopTrunk(F, c.cpad, c.prec, plan, &f.stemFirst) &&
        coopFits(B, coopMembers(F, plan), cus, c.coopSameXcd) &&
        c.trunkLayerCount < 127 && // (a launch's flag values fit the 128 the base advances by)
        // measured: 256 channels with up to eight members per board +1...8 % (24-128 boards;
        // profiles/r04/o_cooperative_trunk_all_k_split_plans_sweep.txt; twelve members, 17-21 boards, do not fit an
        // XCD's CUs three boards at a time); 192 channels +1...9 % (17-80 boards) since the hand-off stays in the XCD's L2
        // (profiles/r04/zd_cooperative_trunk_192_channels.txt; -2...-8 % with write-through stores)
        (c.coopForced || (F == 256 && coopMembers(F, plan) <= 8) || F == 192)) {
        f.kind = LaunchForm::Coop;
        f.members = coopMembers(F, plan);
        return f;
    }
    f.stemFirst = false;

    // A batch with more tiles than CUs runs as two independent chains of half-batch
    // launches on separate streams: boards never interact, so chain A's layer l+1 may
    // start while chain B is still in layer l.  The partly filled last round of
    // workgroups of one chain's launch is topped up by the other chain's launch instead
    // of idling the chip (B=640: 82.7k -> 111.6k evals/s; B=1024: 113.8k -> 119.7k).
    // With NSG_CHAIN_DELAY_US set, two staggered chains also run when all tiles are resident at
    // once on more than half the chip (B = 512 on 256 CUs; not the f32 kernel, which is matrix-bound at
    // 0.85 of its peak and loses 2 %).  With more tiles than CUs the chains compete for CUs and topping-up
    // matters more than phase: those always run unstaggered (staggered B = 640 loses 2 %).
    const int tiles = ((B + 1) / 2) * std::max(1, F / (plan.nwaves * plan.nfrag * 16)); // of a 2-board plan
    const bool oneRound = tiles <= cus;
    int chains = 1;
    if (plan.nb == 2) {
        if (c.chainMinBatch > 0) chains = B >= c.chainMinBatch ? c.numChains : 1;
        else if (!oneRound) chains = c.numChains;
        else if (2 * tiles > cus && c.chainDelayUs != 0 && c.prec != kFp32) chains = std::min(c.numChains, 2);
    }

    // One persistent launch for all 2N+1 3x3 layers without hand-off: forced (NSG_TRUNK_KERNEL=1), or kF16m6 where
    // every tile of the batch is resident at once and the per-layer alternatives measured slower
    bool trunkWanted = c.useTrunkKernel == 1;
    if (c.useTrunkKernel < 0 && c.prec == kF16m6 && plan.nfrag == 4 && automatic && automaticChains(c)) {
        const long t = (B + plan.nb - 1) / plan.nb; // tiles = workgroups of the persistent launch
        trunkWanted = t <= cus && (plan.nb == 1 ? t * 16 >= (long)cus * 9 : t * 4 >= (long)cus * 3);
    }
    const bool trunkKernel = trunkWanted && !c.outsideM8Window && canRunTrunk(F, plan);
    if (trunkKernel) chains = 1;
    f.chains = chains;
    f.trunkPrec = trunkPrecisionOf(c, plan);
    f.trunkLaunchesPerFwd = 2 * c.blocks; // (the 2N residual convs)

    // Two-part batches.  Between the sizes whose plans fill the chip exactly, one plan for the whole batch leaves
    // CUs idle (B = CUs/2 + 1 .. CUs as one-board tiles: one workgroup per board) or pays a two-board tile for a
    // half-empty chip (B = CUs + 1 ..).  Boards never interact, so such a batch runs as a FULL part with the plan of
    // the size below (CUs/2 boards, two-way K split; CUs boards, one-board tiles) plus the remainder with ITS plan
    // (up to CUs/4 boards: the K split by four), on two streams like the half-batch chains above.
    if (mx && !trunkKernel && c.numChains >= 2 && c.tuning.splitBatch != 0 && F == 256 && c.cpad == 128 && automatic &&
        automaticChains(c)) {
        // (measured on 256 CUs, profiles/r02/n_ab_two_part_batches.txt: 129 +10.6 %, 144 +7.7 %, 168 +5.7 %, 176 +2.5 %,
        // 192 -5.9 %; 257 +52 %, 288 +37 %, 320 +27 %, 352 +18 %, 368 +14 %, 384 -7 %: from 3/2 of the CUs on
        // the two-board tiles cover three quarters of the chip and win)
        int off = 0, rem = B;
        auto take = [&](int count) {
            const ConvPlan p = planForBatch(c, count);
            f.parts[f.nParts++] = LaunchForm::Part{off, count, p, trunkPrecisionOf(c, p)};
            off += count; rem -= count;
        };
        // more two-board tiles than CUs: one full chip of them first, the rest by the rules below (instead of two
        // half-batch chains; only just above 2 CUs boards: 513-576 +2-3.5 %, from 640 on the two chains are 3-11 %
        // faster, profiles/r02/n_ab_two_part_batches.txt)
        if (rem > 2 * cus && rem <= c.tuning.splitBatchMax3 * cus / 4) take(2 * cus);
        if (rem > cus && rem < cus + cus / 2) take(cus);
        else if (rem > cus / 2 && rem <= cus / 2 + 3 * cus / 16) take(cus / 2);
        if (f.nParts > 0 && rem > 0) take(rem);
        if (f.nParts < 2) f.nParts = 0;
    }
    if (f.nParts > 0) {
        f.kind = LaunchForm::Parts;
        f.plan = f.parts[0].plan;
        f.chains = f.nParts;
        f.trunkPrec = f.parts[0].trunkPrec;
    } else if (trunkKernel) {
        f.kind = LaunchForm::WholeTrunk;
        f.trunkLaunchesPerFwd = 1; // (stem + 2N convs in ONE launch)
    } else if (chains > 1) {
        f.kind = LaunchForm::Chains;
        f.per = ((B + chains - 1) / chains + 1) / 2 * 2;
        f.stagger = oneRound;
    }
    return f;
}

} // namespace nsg
