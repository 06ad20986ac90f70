// nsg_capi.hip -- implementation of the C ABI declared in include/nsg.h.
//
// One nsg_evaluator = one (device, stream) executor, the role the reference
// gives to infer::TensorRT (src/infer/trt.h:42-88, src/infer/trt.cc).  The
// forward pass it enqueues replaces trt.cc:234-272:
//     H2D bitboards -> feature planes -> policy/value/draw network -> 3x D2H
// all on the evaluator's own non-blocking stream.  No CPU fallback exists:
// every compute entry fails with NSG_E_HIP when no device is usable.
#include "../../include/nsg.h"
#include "kernels/kernels.h"
#include "net_prepare.h"
#include "onnx_reader.h"
#include "onnx_graph.h"
#include "graph_exec.h"
#include "kernels/graph_kernels.h" // launchGraphOutputs: the output scatter (the plan's launches go through graph_exec.h)

#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <strings.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace {

thread_local std::string gLastError;

int fail(int code, const char* fmt, ...) {
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    gLastError = buf;
    return code;
}

#define NSG_HIP(call)                                                             \
    do {                                                                          \
        hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess)                                                     \
            return fail(NSG_E_HIP, "%s failed: %s (%s:%d)", #call,                \
                        hipGetErrorString(e_), __FILE__, __LINE__);               \
    } while (0)

// rocprofv3 markers (the reference has no profiler hooks; the build adds them): with
// NSG_ROCTX=1 every forward pass brackets its phases -- H2D, planes, trunk, heads, D2H -- with roctx
// ranges, resolved from librocprofiler-sdk-roctx.so at first use (no link-time dependency; without the
// variable, or without the library, a range is two predictable branches).  The ranges mark where the
// phase is ENQUEUED on the host; `rocprofv3 --marker-trace --kernel-trace` lines them up with the kernels.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char* e = getenv("NSG_ROCTX");
        if (!e || e[0] == '0') return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return;
        push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
        pop = (int (*)())dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
const Roctx& roctx() {
    static const Roctx r;
    return r;
}
struct Range {
    bool on;
    explicit Range(const char* name) : on(roctx().push != nullptr) {
        if (on) roctx().push(name);
    }
    ~Range() {
        if (on) roctx().pop();
    }
    Range(const Range&) = delete;
    Range& operator=(const Range&) = delete;
};

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    int alloc(size_t n, bool zero) {
        release();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(NSG_E_HIP, "hipMalloc(%zu) failed: %s", n, hipGetErrorString(e));
        }
        bytes = n;
        if (zero) {
            e = hipMemset(p, 0, n);
            if (e != hipSuccess) return fail(NSG_E_HIP, "hipMemset failed: %s", hipGetErrorString(e));
        }
        return NSG_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    ~DevBuf() { release(); }
};

struct ConvLayer {
    DevBuf w;    // fragment-ordered weights
    DevBuf bias; // f32 [cout]
    int cin = 0; // padded input channels
    float accScale = 1.f; // 1 / (power-of-two weight scale), kF16x3 only
};

// Everything nsg_load* uploads: read-only after the load, so evaluators on one device share
// one copy (nsg_load_shared) and evaluators on other devices take a peer copy of it.
struct NetWeights {
    int gpu = 0;
    int prec = 0;
    int F = 0, blocks = 0, vc = 0, vh = 0, cin = 0, cpad = 0, headsCout = 0, fc1K = 0;
    uint64_t params = 0;
    // Estimated largest trunk activation (estimateActivationBound) and, for kF16m8, whether it leaves the
    // window its fixed-scale e4m3 copies cover: then every batch runs the kF16x3 copy of the trunk.
    double actBound = 0.0;
    bool outsideM8Window = false;
    ConvLayer stem;
    std::vector<ConvLayer> conv1, conv2;
    // kF16m8 also holds the trunk in kF16x3 form: batches too small for full
    // tiles (4 fragments per wave) run the kF16x3 small-tile kernels instead
    ConvLayer stemX3;
    std::vector<ConvLayer> conv1X3, conv2X3;
    ConvLayer heads;
    ConvLayer fc1;
    DevBuf fc2W, fc2B;
    ~NetWeights() {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        (void)hipSetDevice(gpu); // the buffers are released on the device that owns them
        stem = ConvLayer(); stemX3 = ConvLayer(); heads = ConvLayer(); fc1 = ConvLayer();
        conv1.clear(); conv2.clear(); conv1X3.clear(); conv2X3.clear();
        fc2W.release(); fc2B.release();
        if (cur >= 0) (void)hipSetDevice(cur);
    }
};

// The general graph path: the immutable plan and its constants uploaded to one device.
// Evaluators of that device share it (nsg_load_shared); activation buffers are each evaluator's own.
struct GraphWeights {
    int gpu = 0;
    std::shared_ptr<const nsg::graph::GraphPlan> plan;
    DevBuf w;
    ~GraphWeights() {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        (void)hipSetDevice(gpu);
        w.release();
        if (cur >= 0) (void)hipSetDevice(cur);
    }
};

constexpr int kMaxEventPairs = 1024;

} // namespace

struct nsg_evaluator {
    int gpu = 0;
    int batchMax = 0;
    int numChannels = 0;
    int prec = NSG_PRECISION_FP32;
    bool loaded = false;
    hipStream_t stream = nullptr;
    hipDeviceProp_t prop{};

    // network dims
    int F = 0, blocks = 0, vc = 0, vh = 0, cpad = 0, headsCout = 0, fc1K = 0;
    uint64_t params = 0;

    // device buffers (sized for batchMax rounded up to whole workgroups)
    DevBuf input;         // bitboards  [B][C][16 B]          (trt.cc:57-58)
    DevBuf planes;        // trunk input [Bpad][81][cpad] T   (trt.cc:59-60, other layout)
    DevBuf act[3];        // trunk activations [Bpad][81][F] T
    DevBuf policy;        // [B][2187] f32                    (trt.cc:61-62)
    DevBuf value, draw;   // [B] f32                          (trt.cc:63-66)
    DevBuf moveIdx, moveOff, gathered; // legal-move gather (allocated on first use)
    DevBuf vfeat;         // [B][fc1K] T
    DevBuf hidden;        // [K slices][B][VH] f32 partial sums of the value MLP's first layer
    DevBuf scratch;       // debug read-back

    std::shared_ptr<NetWeights> W; // shared by the evaluators of one device (nsg_load_shared)
    // general graph path: set instead of W when the loaded network runs on it
    std::shared_ptr<GraphWeights> G;
    DevBuf gPlanes;               // [batchMax * 81][planeStride] f32 input planes
    std::vector<DevBuf> gAct;     // the plan's activation buffers, sized for batchMax
    std::vector<float*> gActPtr;  // ... and their device pointers, as graph_exec.h's GraphBufs takes them
    int graphMode = 0;            // nsg_set_graph_mode
    int loadedNodes = 0;          // ONNX nodes of a family model on the specialised path (0: an NSGW blob)
    int lastTrunkPrec = -1; // precision the most recent forward ran its trunk in
    // host statistics (mcts::Statistics evaluationCount / batchSizeAccumulated, statistics.h:74-98)
    uint64_t statBatches = 0, statPositions = 0;
    DevBuf stamps;           // diagnostic builds: per-layer, per-workgroup cycle stamps
    DevBuf trunkLayers;      // persistent-trunk layer list (stem + 2 per block)
    int trunkLayerCount = 0;
    // One persistent launch for all 3x3 layers (a workgroup owns its boards through every layer: no grid barrier, no
    // launch boundary, workgroups drift apart instead of hitting memory in lock-step).  -1 (default): taken by a
    // kF16m6 evaluator where every tile of the batch is resident at once AND the per-layer alternatives measured
    // slower -- on 256 CUs 144..256 boards (one-board tiles; +13 % at 160-176 where it replaces the 128 + rest
    // two-part batch, +7 % at 192-256) and 384..512 boards (two-board tiles: +6-7 % on game positions, +3-4 % on the
    // benchmark's replicated initial position); with more tiles than CUs the second round waits for 41 layers of the
    // first (-35 %), 257..383 boards keep the two-part batches (profiles/r04/j_persistent_trunk_vs_per_layer_by_batch.txt).
    // NSG_TRUNK_KERNEL=1 forces it wherever the plan allows, =0 switches it off.  (Rounds 2-3, before the loop read its
    // weights and tiles through buffer descriptors: +1.6-2.4 % at 512, -3..-7 % at 160-192; r1: +-0 % kF16m8, -6 % kF16x3.)
    int useTrunkKernel = -1;

    nsg::TrunkSequence seq;   // the 3x3 layers' buffers and weights in launch order (net_prepare.h), built by finishLoad
    void* trunkOut = nullptr; // which act[] holds the trunk output of the last forward

    // Team trunk (kernels/team_trunk.hip): up to sixteen boards, every 3x3 layer in one persistent launch, kF16x3
    // arithmetic.  NSG_TEAM_TRUNK=0 switches it off.  One team launch per DEVICE at a time (teamToken below).
    DevBuf teamLayers;       // nsg::TeamLayer list (stem + 2 per block) on the kF16x3 copy of the trunk
    DevBuf teamSets;         // 2 hand-off sets x 4 images x teamBoards boards (nsg::TeamHandoff)
    int teamBoards = 0;      // boards an image holds: min(batchMax, kTeamMaxBoards)
    int teamSet = 0;         // the set the next launch writes
    int teamDirty[2] = {0, 0}; // boards of each set that do not hold the sentinel
    int teamLayerCount = 0;
    int teamEnabled = 1;
    int teamForceRowGroups = 0; // NSG_TEAM_MEMBERS / 16, read when the evaluator is created (0: as many as fit)
    int teamMaxBatch = nsg::kTeamMaxBoards; // NSG_TEAM_MAX_BATCH, likewise
    int teamLastMembers = 0; // workgroups per board of the most recent team launch
    uint64_t teamFallbacks = 0; // team launches that gave up and were re-run on the per-layer kernels (nsg_get_team_stats)
    int teamLockedOut = 0;      // another PROCESS holds this device's team token (teamDeviceLock): per-layer kernels only
    bool teamLockHeld = false;  // this evaluator holds a reference on the process's lock of the device
    // Cooperative trunk (mfma_tile.h, coopTrunkKernel): a K-split plan of a kF16m6 net (17 boards upward: launch_form.h,
    // canRunCoopTrunk) as ONE launch whose workgroups per board hand their output slices to each other.  NSG_COOP_TRUNK=0 switches it off.  Shares the team
    // trunk's device token (both need every workgroup of their grid resident), status word and recovery.
    DevBuf coopFlags;           // [batchMax][members] unsigned; values count on from launch to launch (coopFlagBase)
    unsigned coopFlagBase = 0;  // first flag value of the next cooperative launch
    int coopEnabled = 1;
    int coopForced = 0;         // NSG_COOP_TRUNK=1: wherever a plan allows it; unset: where it measured faster (enqueueForward)
    int lastPersistent = 0;     // what the most recent forward ran: 0 per-layer / persistent-without-hand-off, 1 team trunk, 2 cooperative trunk
    int lastWholeTrunk = 0;     // the most recent forward ran every 3x3 layer as ONE launch without hand-off (launchTrunk)
    int lastParts = 0;          // ... as a two-part batch of this many parts (0: not split into parts)
    int coopFaultXccLaunches = 0; // NSG_COOP_FAULT_XCC_LAUNCHES (test hook), see enqueueCoop
    int teamFaultLaunches = 0;  // NSG_TEAM_FAULT_LAUNCHES (test hook): this many team launches are made ONE WORKGROUP SHORT,
                                // so that the team waits in vain, gives up and the recovery path runs
    // What the most recent compute call queued behind its forward: should the team launch of that forward give up
    // (teamRecover), the same batch is re-run on the per-layer kernels and these copies are issued again.
    struct Pending {
        int kind = 0; // 0 nothing, 1 nsg_compute_nonblocking, 2 nsg_compute_gather_nonblocking, 3 nsg_forward_resident
        size_t n = 0, total = 0;
        int softmax = 0;
        float* pol = nullptr; float* win = nullptr; float* draw = nullptr; float* vals = nullptr;
    } pending;
    hipEvent_t teamDone = nullptr; // behind this evaluator's most recent team launch (the token's next holder waits for it)
    int* teamStatusHost = nullptr; // host-mapped: raised by the kernel when a bounded spin runs out
    int* teamStatusDev = nullptr;
    bool teamLast = false;   // the most recent forward ran the team trunk

    // chains: large batches run as independent half-batch launch chains
    static constexpr int kMaxChains = 4;
    hipStream_t chainStream[kMaxChains - 1] = {};
    hipEvent_t forkEvent = nullptr;
    hipEvent_t joinEvent[kMaxChains - 1] = {};
    int numChains = 2;        // NSG_CHAINS (3 about equal, 4 slower: DESIGN.md 6)
    int chainMinBatch = 0;    // NSG_CHAIN_MIN_BATCH; 0 = more 2-board tiles than CUs
    nsg::ConvTuning tuning;   // NSG_CONV_* overrides, read at creation
    nsg::ConvPlan lastPlan{0, 0, 0};
    int lastChains = 0;
    // Staggered chains: chain c starts c/chains of a conv layer's duration after chain 0, so one
    // chain's memory bursts (tile loads, residual reads, output stores) fall into the other's matrix
    // phase instead of colliding with its bursts.  The layer time is measured on the first chained
    // forward of a given shape (HIP events around chain 0's residual trunk); results do not depend on it.
    // Off by default: measured +2.5 %, +2 % and +0.3 % at B = 512 (20x256, kF16m8) on three boxes, -2.4 % on
    // 10x192 and nothing below a full chip -- too fragile to be the default.
    int chainDelayUs = 0;     // NSG_CHAIN_DELAY_US: 0 = no stagger, -1 = measured layer time / chains, > 0 = fixed
    hipEvent_t calibEv[2] = {};
    bool calibPending = false;
    int calibKey = -1;        // launch shape (rounds of workgroups per chain launch, chains) the measurement belongs to
    int calibPendingKey = -1;
    float calibLayerUs = 0.f;

    // profiling
    bool profile = false;
    std::vector<hipEvent_t> ev; // 4 per forward: fwd begin, trunk begin, trunk end, fwd end
    int evUsed = 0;
    double trunkMs = 0, fwdMs = 0;
    uint64_t trunkLaunches = 0, forwards = 0;
    int pendingTrunkLaunchesPerFwd = 0;
};

namespace {

int bind(nsg_evaluator* ev) {
    NSG_HIP(hipSetDevice(ev->gpu));
    return NSG_OK;
}

int drainProfile(nsg_evaluator* ev) {
    if (ev->evUsed == 0) return NSG_OK;
    NSG_HIP(hipStreamSynchronize(ev->stream));
    for (int i = 0; i < ev->evUsed; i += 4) {
        float a = 0, b = 0;
        NSG_HIP(hipEventElapsedTime(&a, ev->ev[i + 1], ev->ev[i + 2]));
        NSG_HIP(hipEventElapsedTime(&b, ev->ev[i + 0], ev->ev[i + 3]));
        ev->trunkMs += a;
        ev->fwdMs += b;
        ev->trunkLaunches += (uint64_t)ev->pendingTrunkLaunchesPerFwd;
        ev->forwards += 1;
    }
    ev->evUsed = 0;
    return NSG_OK;
}

// Uploads one prepared layer (caller's thread, bound to the evaluator's device) and releases its host image.
int commitLayer(nsg::PreparedLayer& P, ConvLayer* L) {
    L->accScale = P.accScale;
    int rc = L->w.alloc(P.image.size(), false);
    if (rc) return rc;
    NSG_HIP(hipMemcpy(L->w.p, P.image.data(), P.image.size(), hipMemcpyHostToDevice));
    std::vector<unsigned char>().swap(P.image);
    rc = L->bias.alloc(P.bias.size() * 4, false);
    if (rc) return rc;
    NSG_HIP(hipMemcpy(L->bias.p, P.bias.data(), P.bias.size() * 4, hipMemcpyHostToDevice));
    L->cin = P.cin;
    return NSG_OK;
}

int roundUp(int a, int b) { return (a + b - 1) / b * b; }

// One wave that spins for `ticks` of the 100 MHz constant clock: phase-shifts a chain.
__global__ void delayKernel(unsigned long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

// Two team launches on one device could each hold CUs that the other's not-yet-scheduled members need.  One token
// per device: an evaluator launches a team trunk if it holds the token already (its launches are ordered on its own
// stream); otherwise its stream first waits -- on the device, hipStreamWaitEvent -- for the event behind the holder's
// most recent team launch, and it takes the token.  Waiting -- not falling back to the per-layer kernels -- keeps the
// arithmetic of a batch independent of timing: a self-play engine's two executors then produce the same bits in
// every run.  The mutex is held from the hand-over of the token until the new holder's launch AND its event are in
// its stream (TeamTokenGuard around enqueueTeam): released in between, the old holder could come back, find nothing
// to wait for yet, take the token back and launch beside the new one -- two engine threads of one self-play process
// did exactly that, and both launches timed out.
std::mutex gTeamMutex;
nsg_evaluator* gTeamOwner[64] = {};
struct TeamTokenGuard {
    std::unique_lock<std::mutex> lock;
    bool held = false;
    explicit TeamTokenGuard(nsg_evaluator* ev) : lock(gTeamMutex) {
        nsg_evaluator*& owner = gTeamOwner[ev->gpu & 63];
        if (owner != ev && owner != nullptr && owner->teamDone &&
            hipStreamWaitEvent(ev->stream, owner->teamDone, 0) != hipSuccess)
            return;
        owner = ev;
        held = true;
    }
};
void releaseTeamToken(nsg_evaluator* ev) {
    std::lock_guard<std::mutex> lock(gTeamMutex);
    if (gTeamOwner[ev->gpu & 63] == ev) gTeamOwner[ev->gpu & 63] = nullptr;
}

// ... and one PROCESS per device: two processes' team launches would starve each other the same way, and no stream
// event reaches across processes.  The first evaluator of a process that builds a team layer list for a device takes
// an advisory lock (flock, released when the process ends) on a file named after the device's PCI bus id; a process
// that finds the lock taken keeps to the per-layer kernels on that device.  (A file system the other process does
// not share -- another container -- is not covered: there the bounded spins and teamRecover are what is left.)
// The lock is counted: the last evaluator of the process that used it gives it back (nsg_destroy).
// NSG_TEAM_LOCK_DIR names the directory of the lock files (default /dev/shm, then /tmp) -- for processes that share a
// device but not those directories.  Returns false only when ANOTHER process holds the lock.
struct TeamDeviceLocks {
    std::mutex m;
    int fd[64];
    int refs[64];
    TeamDeviceLocks() { for (int i = 0; i < 64; ++i) { fd[i] = -1; refs[i] = 0; } }
};
TeamDeviceLocks& teamLocks() {
    static TeamDeviceLocks t;
    return t;
}
bool teamDeviceLock(int gpu) {
    TeamDeviceLocks& T = teamLocks();
    std::lock_guard<std::mutex> lock(T.m);
    const int g = gpu & 63;
    if (T.refs[g] > 0) { ++T.refs[g]; return true; } // this process holds it (or found nothing to lock: fd -1)
    char bus[64] = "";
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), gpu) != hipSuccess || !bus[0]) snprintf(bus, sizeof(bus), "gpu%d", gpu);
    for (char* c = bus; *c; ++c)
        if (*c == ':' || *c == '/' || *c == '.') *c = '_';
    const char* envDir = getenv("NSG_TEAM_LOCK_DIR");
    const char* dirs[2] = {envDir && *envDir ? envDir : "/dev/shm", envDir && *envDir ? nullptr : "/tmp"};
    for (const char* dir : dirs) {
        if (!dir) continue;
        char path[512];
        snprintf(path, sizeof(path), "%s/nsg_team_token_%s.lock", dir, bus);
        const mode_t old = umask(0);
        const int f = open(path, O_CREAT | O_RDWR | O_CLOEXEC, 0666);
        umask(old);
        if (f < 0) continue;
        if (flock(f, LOCK_EX | LOCK_NB) == 0) { T.fd[g] = f; T.refs[g] = 1; return true; }
        const bool taken = errno == EWOULDBLOCK;
        close(f);
        if (taken) return false;
    }
    T.fd[g] = -1; // no lock file could be opened: nothing to coordinate through (see above)
    T.refs[g] = 1;
    return true;
}
void teamDeviceUnlock(int gpu) {
    TeamDeviceLocks& T = teamLocks();
    std::lock_guard<std::mutex> lock(T.m);
    const int g = gpu & 63;
    if (T.refs[g] > 0 && --T.refs[g] == 0 && T.fd[g] >= 0) {
        close(T.fd[g]); // (closing the descriptor gives the flock back)
        T.fd[g] = -1;
    }
}

// Everything chooseLaunchForm (launch_form.h) reads of this evaluator, as plain values.
nsg::LaunchConfig launchConfigOf(const nsg_evaluator* ev) {
    // (NSG_KSPLIT4_MAX_BATCH: experiment knob, read once -- largest batch that takes the four-way K split)
    static const int k4max = [] { const char* e = getenv("NSG_KSPLIT4_MAX_BATCH"); return e ? atoi(e) : -1; }();
    nsg::LaunchConfig c;
    c.prec = ev->prec;
    c.F = ev->F; c.cpad = ev->cpad; c.blocks = ev->blocks;
    c.trunkLayerCount = ev->trunkLayerCount;
    c.cus = ev->prop.multiProcessorCount;
    c.numChains = ev->numChains;
    c.tuning = ev->tuning;
    c.useTrunkKernel = ev->useTrunkKernel;
    c.chainMinBatch = ev->chainMinBatch;
    c.chainDelayUs = ev->chainDelayUs;
    c.teamMaxBatch = ev->teamMaxBatch;
    c.teamForceRowGroups = ev->teamForceRowGroups;
    c.coopForced = ev->coopForced;
    c.ksplit4Max = k4max;
    c.coopSameXcd = nsg::coopSameXcd();
    c.outsideM8Window = ev->W->outsideM8Window;
    c.teamAvailable = ev->teamLayerCount > 0 && ev->teamEnabled;
    c.coopAvailable = ev->coopEnabled && ev->teamStatusDev && ev->coopFlags.p;
    return c;
}

// The value / policy heads of boards [off, off + count) behind a trunk whose output for them starts at `x` (the tail
// of every forward).
int enqueueHeads(nsg_evaluator* ev, void* x, int off, int count, int hprec, hipStream_t s) {
    Range headsRange("nsg.heads");
    float* policy = (float*)ev->policy.p + (size_t)off * NSG_MOVE_INDEX_MAX;
    void* vfeat = (unsigned char*)ev->vfeat.p + (size_t)off * ev->fc1K * nsg::elemSize(hprec);
    float* hidden = (float*)ev->hidden.p + (size_t)off * ev->vh;
    NSG_HIP(nsg::launchHeads(x, ev->W->heads.w.p, (const float*)ev->W->heads.bias.p, policy, vfeat, count, ev->F,
                             ev->headsCout, ev->vc, ev->fc1K, ev->W->heads.accScale, hprec, s));
    const size_t partStride = (size_t)ev->batchMax * ev->vh; // floats between the K slices' partial sums
    NSG_HIP(nsg::launchDense(vfeat, ev->W->fc1.w.p, (const float*)ev->W->fc1.bias.p, hidden, count, ev->fc1K,
                             ev->vh, partStride, ev->W->fc1.accScale, hprec, s));
    NSG_HIP(nsg::launchValueOut(hidden, (const float*)ev->W->fc1.bias.p, nsg::denseSplits(ev->fc1K, hprec), partStride,
                                (const float*)ev->W->fc2W.p, (const float*)ev->W->fc2B.p,
                                (float*)ev->value.p + off, (float*)ev->draw.p + off, count, ev->vh, s));
    return NSG_OK;
}

// What a step of ev->seq names: a buffer of the evaluator, the weights of a layer (x3: in the kF16x3 copy of the trunk).
void* trunkBuffer(const nsg_evaluator* ev, int buf) {
    return buf == nsg::kBufNone ? nullptr : buf == nsg::kBufPlanes ? ev->planes.p : ev->act[buf - nsg::kBufAct0].p;
}
const ConvLayer& trunkWeights(const NetWeights& N, const nsg::TrunkStep& t, bool x3) {
    if (t.weights == nsg::kStem) return x3 ? N.stemX3 : N.stem;
    if (t.weights == nsg::kConv1) return (x3 ? N.conv1X3 : N.conv1)[(size_t)t.block];
    return (x3 ? N.conv2X3 : N.conv2)[(size_t)t.block];
}

// The output of the persistent launches' layer list: the buffer the sequence ends in.
void* trunkListOutput(nsg_evaluator* ev) {
    return ev->trunkOut = trunkBuffer(ev, ev->seq.outBuf);
}

// The whole forward of a batch of at most kTeamMaxBoards boards with the team trunk (under the device's token).
int enqueueTeam(nsg_evaluator* ev, int B, int members, hipStream_t s, hipEvent_t trunkBegin, hipEvent_t trunkEnd) {
    {   // (the feature bitboards are decoded by the first layer of the team launch itself)
        Range r("nsg.trunk");
        if (trunkBegin) NSG_HIP(hipEventRecord(trunkBegin, s));
        nsg::TeamHandoff ho;
        ho.imageStride = (size_t)ev->teamBoards * 81 * 1024;
        const size_t setBytes = 4 * ho.imageStride;
        ho.set = (unsigned char*)ev->teamSets.p + (size_t)ev->teamSet * setBytes;
        ho.other = (unsigned char*)ev->teamSets.p + (size_t)(1 - ev->teamSet) * setBytes;
        ho.cleanBoards = ev->teamDirty[1 - ev->teamSet];
        ho.bits = ev->input.p;
        ho.bitChannels = ev->numChannels;
        const int shortBy = ev->teamFaultLaunches > 0 ? 1 : 0;
        if (shortBy) --ev->teamFaultLaunches;
        NSG_HIP(nsg::launchTeamTrunk((const nsg::TeamLayer*)ev->teamLayers.p, ev->teamLayerCount, B, ev->F, members, ho,
                                     ev->teamStatusDev, s, shortBy));
        ev->teamLastMembers = members;
        NSG_HIP(hipEventRecord(ev->teamDone, s)); // (under the token's mutex: enqueuePersistent)
        ev->teamDirty[1 - ev->teamSet] = 0;
        ev->teamDirty[ev->teamSet] = B;
        ev->teamSet = 1 - ev->teamSet;
        if (trunkEnd) NSG_HIP(hipEventRecord(trunkEnd, s));
    }
    return enqueueHeads(ev, trunkListOutput(ev), 0, B, nsg::kF16x3, s);
}

// The whole forward of a mid batch with the cooperative trunk (under the device's token).
int enqueueCoop(nsg_evaluator* ev, int B, const nsg::LaunchForm& form, hipStream_t s, hipEvent_t trunkBegin, hipEvent_t trunkEnd) {
    const int prec = ev->prec;
    {
        Range r("nsg.planes");
        NSG_HIP(nsg::launchExtractBitsAct(ev->planes.p, (const uint64_t*)ev->input.p, B, ev->numChannels, ev->cpad, prec, s));
    }
    {
        Range r("nsg.trunk");
        // flag values count on across launches (24 bits; the array is cleared when they run out): no memset per forward
        if (ev->coopFlagBase + 256u >= (1u << 24)) {
            NSG_HIP(hipMemsetAsync(ev->coopFlags.p, 0, ev->coopFlags.bytes, s));
            ev->coopFlagBase = 0;
        }
        const unsigned flagBase = ev->coopFlagBase;
        ev->coopFlagBase += 128; // (more than any net's 3x3 layers: 1 + 2 x 40)
        if (form.stemFirst) // the stem has fewer chunk pairs than the plan splits K by: its own launch, the plan's stem kernel
            NSG_HIP(nsg::launchConv3x3(ev->planes.p, ev->W->stem.w.p, (const float*)ev->W->stem.bias.p, nullptr, ev->act[0].p, B,
                                       ev->cpad, ev->F, 1, ev->W->stem.accScale, prec, form.plan, s, nullptr, false));
        const int l0 = form.stemFirst ? 1 : 0;
        if (trunkBegin) NSG_HIP(hipEventRecord(trunkBegin, s));
        // (test hook NSG_TEAM_FAULT_LAUNCHES: the last board's second member leaves at once and never publishes)
        // (NSG_COOP_FAULT_XCC_LAUNCHES: every board's second member claims another XCD, what a placement the hand-off
        // cannot use looks like)
        int faultBoard = ev->teamFaultLaunches > 0 ? B - 1 : -1;
        if (faultBoard >= 0) --ev->teamFaultLaunches;
        else if (ev->coopFaultXccLaunches > 0) { faultBoard = -2; --ev->coopFaultXccLaunches; }
        NSG_HIP(nsg::launchCoopTrunk((const unsigned char*)ev->trunkLayers.p + (size_t)l0 * nsg::trunkLayerBytes(),
                                     ev->trunkLayerCount - l0, B, ev->F, prec, form.plan, (unsigned*)ev->coopFlags.p, flagBase,
                                     ev->teamStatusDev, s, faultBoard));
        NSG_HIP(hipEventRecord(ev->teamDone, s));
        if (trunkEnd) NSG_HIP(hipEventRecord(trunkEnd, s));
    }
    return enqueueHeads(ev, trunkListOutput(ev), 0, B, nsg::headPrecision(prec), s);
}

// The team or the cooperative trunk.  Two such launches on one device could starve each other: under the device's token.
int enqueuePersistent(nsg_evaluator* ev, int B, const nsg::LaunchForm& form, hipStream_t s, hipEvent_t trunkBegin,
                      hipEvent_t trunkEnd) {
    const bool team = form.kind == nsg::LaunchForm::Team;
    TeamTokenGuard token(ev);
    if (!token.held)
        return fail(NSG_E_HIP, team ? "team trunk: hipStreamWaitEvent on the device's other team launch failed"
                                    : "cooperative trunk: hipStreamWaitEvent on the device's other persistent launch failed");
    return team ? enqueueTeam(ev, B, form.members, s, trunkBegin, trunkEnd) : enqueueCoop(ev, B, form, s, trunkBegin, trunkEnd);
}

// Every 3x3 layer in one persistent launch whose workgroups own whole boards (no hand-off).
int enqueueWholeTrunk(nsg_evaluator* ev, int B, const nsg::ConvPlan& plan, hipStream_t s, hipEvent_t trunkBegin,
                      hipEvent_t trunkEnd) {
    const int prec = ev->prec;
    NSG_HIP(nsg::launchExtractBitsAct(ev->planes.p, (const uint64_t*)ev->input.p, B, ev->numChannels, ev->cpad, prec, s));
    if (trunkBegin) NSG_HIP(hipEventRecord(trunkBegin, s));
    NSG_HIP(nsg::launchTrunk(ev->trunkLayers.p, ev->trunkLayerCount, B, prec, plan, s));
    if (trunkEnd) NSG_HIP(hipEventRecord(trunkEnd, s));
    return enqueueHeads(ev, trunkListOutput(ev), 0, B, nsg::headPrecision(prec), s);
}

// One chain = the whole forward for boards [off, off + count) on stream `s`, the trunk in `prec`: the evaluator's
// precision, or kF16x3 -- the kF16x3 copy of the trunk -- where an MX evaluator's plan has no MX form (LaunchForm::trunkPrec).
int enqueueChain(nsg_evaluator* ev, int off, int count, const nsg::ConvPlan& plan, int prec, hipStream_t s,
                 bool stampsOk, hipEvent_t trunkBegin = nullptr, hipEvent_t trunkEnd = nullptr) {
    const bool x3Fallback = prec != ev->prec;
    const size_t es = (size_t)nsg::elemSize(prec);
    // this chain's boards of the sequence's four buffers
    void* buf[4];
    for (int b = nsg::kBufPlanes; b <= nsg::kBufAct2; ++b)
        buf[b] = (unsigned char*)trunkBuffer(ev, b) + (size_t)off * 81 * (b == nsg::kBufPlanes ? ev->cpad : ev->F) * es;
    const uint64_t* input = (const uint64_t*)ev->input.p + (size_t)off * ev->numChannels * 2;
    // feature planes (replaces cuda::extractBits, trt.cc:255-258)
    {
        Range r("nsg.planes");
        NSG_HIP(nsg::launchExtractBitsAct(buf[nsg::kBufPlanes], input, count, ev->numChannels, ev->cpad, prec, s));
    }
    const int hprec = nsg::headPrecision(prec); // kF16m8: the last trunk layer writes the kF16x3 layout
    void* x = buf[ev->seq.outBuf];
    {
        Range trunkRange("nsg.trunk");
        // stem + residual trunk
        const int nl = (int)ev->seq.steps.size();
        for (int i = 0; i < nl; ++i) {
            const nsg::TrunkStep& t = ev->seq.steps[(size_t)i];
            const ConvLayer& L = trunkWeights(*ev->W, t, x3Fallback);
            unsigned long long* st = nullptr;
#ifdef NSG_DIAG_STAMPS
            if (ev->stamps.p && stampsOk && i > 0) st = (unsigned long long*)ev->stamps.p + (size_t)(i - 1) * 4096 * 8;
#else
            (void)stampsOk;
#endif
            NSG_HIP(nsg::launchConv3x3(buf[t.in], L.w.p, (const float*)L.bias.p, t.residual == nsg::kBufNone ? nullptr : buf[t.residual],
                                       buf[t.out], count, L.cin, ev->F, 1, L.accScale, prec, plan, s, st,
                                       hprec != prec && i == nl - 1));
            if (i == 0 && trunkBegin) NSG_HIP(hipEventRecord(trunkBegin, s));
        }
        if (trunkEnd) NSG_HIP(hipEventRecord(trunkEnd, s));
        if (off == 0) ev->trunkOut = x;
    }
    return enqueueHeads(ev, x, off, count, hprec, s);
}

// A forward pass of the general graph path: the plane expansion, the plan's launches in order, the output scatter.
// Always exact fp32; profiling brackets the span from the first to the last conv / dense launch as "trunk".
int enqueueGraph(nsg_evaluator* ev, int B) {
    namespace gr = nsg::graph;
    hipStream_t s = ev->stream;
    const gr::GraphPlan& P = *ev->G->plan;
    const gr::GraphBufs bufs{(float*)ev->gPlanes.p, ev->gActPtr.data(), (const float*)ev->G->w.p};
    auto dv = [&](const gr::View& v) { // (the three output views)
        gr::DevView d;
        d.p = v.buf < 0 ? bufs.planes : bufs.act[(size_t)v.buf]; d.stride = v.stride; d.offset = v.offset; d.C = v.C;
        return d;
    };
    const bool prof = ev->profile;
    if (prof && ev->evUsed + 4 > (int)ev->ev.size()) {
        int rc = drainProfile(ev);
        if (rc) return rc;
    }
    hipEvent_t* e = prof ? &ev->ev[ev->evUsed] : nullptr;
    if (prof) NSG_HIP(hipEventRecord(e[0], s));
    ev->teamLast = false;
    ev->lastPersistent = 0;
    ev->lastWholeTrunk = 0;
    ev->lastParts = 0;
    ev->lastPlan = nsg::ConvPlan{0, 0, 0};
    ev->lastChains = 0;
    ev->lastTrunkPrec = nsg::kFp32;
    ev->trunkOut = nullptr;
    NSG_HIP(nsg::launchExtractBitsAct(ev->gPlanes.p, (const uint64_t*)ev->input.p, B, ev->numChannels, P.planeStride,
                                      nsg::kFp32, s));
    if (prof && P.convLaunches == 0) { NSG_HIP(hipEventRecord(e[1], s)); NSG_HIP(hipEventRecord(e[2], s)); }
    int convs = 0;
    for (const gr::Launch& L : P.launches) { // each launch: graph_exec.hip
        const bool conv = L.is<gr::ConvArgs>();
        if (prof && conv && convs == 0) NSG_HIP(hipEventRecord(e[1], s));
        NSG_HIP(gr::runLaunch(L, bufs, B, s));
        if (prof && conv && ++convs == P.convLaunches) NSG_HIP(hipEventRecord(e[2], s));
    }
    NSG_HIP(gr::launchGraphOutputs(dv(P.policy), P.policy.spatial, dv(P.value), dv(P.draw), (float*)ev->policy.p,
                                   (float*)ev->value.p, (float*)ev->draw.p, B, s));
    if (prof) {
        NSG_HIP(hipEventRecord(e[3], s));
        ev->evUsed += 4;
        ev->pendingTrunkLaunchesPerFwd = P.convLaunches;
    }
    return NSG_OK;
}

// Chains and Parts: independent launch chains on separate streams, forked from and joined to `s` -- half-batch chains of
// one plan, or a full part plus remainder parts with their own plans.
int enqueueForked(nsg_evaluator* ev, int B, const nsg::LaunchForm& form, hipStream_t s, hipEvent_t trunkBegin,
                  hipEvent_t trunkEnd) {
    const bool isParts = form.kind == nsg::LaunchForm::Parts;
    // stagger: measured layer time / chains (first forward of a launch shape runs unstaggered and is timed)
    int delayUs = !isParts && (form.stagger || ev->chainDelayUs > 0) ? ev->chainDelayUs : 0;
    bool calibrate = false;
    if (delayUs < 0) {
        if (ev->calibPending) { // the previous forward has been awaited: its events are complete
            float ms = 0.f;
            if (hipEventSynchronize(ev->calibEv[1]) == hipSuccess &&
                hipEventElapsedTime(&ms, ev->calibEv[0], ev->calibEv[1]) == hipSuccess && ev->blocks > 0) {
                ev->calibLayerUs = ms * 1000.f / (float)(2 * ev->blocks);
                ev->calibKey = ev->calibPendingKey;
            }
            ev->calibPending = false;
        }
        const int wgPerChain = (form.per / 2) * std::max(1, ev->F / (form.plan.nwaves * form.plan.nfrag * 16));
        const int rounds = (wgPerChain + ev->prop.multiProcessorCount - 1) / ev->prop.multiProcessorCount;
        const int key = rounds * 16 + form.chains;
        if (key == ev->calibKey && ev->calibLayerUs > 0.f) {
            delayUs = (int)(ev->calibLayerUs / (float)form.chains + 0.5f);
        } else {
            delayUs = 0;
            calibrate = ev->blocks > 0;
            ev->calibPendingKey = key;
        }
    }
    NSG_HIP(hipEventRecord(ev->forkEvent, s));
    if (trunkBegin) NSG_HIP(hipEventRecord(trunkBegin, s));
    for (int c = 0; c < form.chains; ++c) {
        const int off = isParts ? form.parts[c].off : c * form.per;
        const int count = isParts ? form.parts[c].count : std::min(form.per, B - off);
        if (count <= 0) break;
        hipStream_t cs = (c == 0) ? s : ev->chainStream[c - 1];
        if (c > 0) NSG_HIP(hipStreamWaitEvent(cs, ev->forkEvent, 0));
        if (c > 0 && delayUs > 0) {
            hipLaunchKernelGGL(delayKernel, dim3(1), dim3(64), 0, cs, (unsigned long long)delayUs * 100ull * c);
        }
        const bool timeIt = calibrate && c == 0;
        int rc = enqueueChain(ev, off, count, isParts ? form.parts[c].plan : form.plan,
                              isParts ? form.parts[c].trunkPrec : form.trunkPrec, cs, c == 0,
                              timeIt ? ev->calibEv[0] : nullptr, timeIt ? ev->calibEv[1] : nullptr);
        if (rc) return rc;
        if (timeIt) ev->calibPending = true;
        if (c > 0) {
            NSG_HIP(hipEventRecord(ev->joinEvent[c - 1], cs));
            NSG_HIP(hipStreamWaitEvent(s, ev->joinEvent[c - 1], 0));
        }
    }
    if (trunkEnd) NSG_HIP(hipEventRecord(trunkEnd, s));
    return NSG_OK;
}

// What the nsg_get_last_* getters report of a forward that takes `form`.
void recordLaunchForm(nsg_evaluator* ev, const nsg::LaunchForm& form) {
    ev->lastPersistent = form.kind == nsg::LaunchForm::Team ? 1 : form.kind == nsg::LaunchForm::Coop ? 2 : 0;
    ev->teamLast = ev->lastPersistent != 0;
    ev->lastWholeTrunk = form.kind == nsg::LaunchForm::WholeTrunk ? 1 : 0;
    ev->lastParts = form.nParts;
    ev->lastPlan = form.plan;
    ev->lastChains = form.chains;
    ev->lastTrunkPrec = form.trunkPrec;
}

// A forward pass: WHICH launches a batch of n boards takes is chooseLaunchForm's business (launch_form.h); this issues them.
int enqueueForward(nsg_evaluator* ev, size_t n) {
    const int B = (int)n;
    ++ev->statBatches;
    ev->statPositions += n;
    if (ev->G) return enqueueGraph(ev, B); // the general graph path: none of the plan / team / chain logic below
    hipStream_t s = ev->stream;
    // (a give-up word still raised here belongs to a forward nobody waited for: its batch is gone, neither persistent
    // path is taken again)
    if (ev->teamStatusHost && *ev->teamStatusHost != 0) {
        *ev->teamStatusHost = 0;
        ev->teamEnabled = 0;
        ev->coopEnabled = 0;
        ++ev->teamFallbacks;
        releaseTeamToken(ev);
    }
    const nsg::LaunchForm form = nsg::chooseLaunchForm(launchConfigOf(ev), B);
    recordLaunchForm(ev, form);

    const bool prof = ev->profile;
    if (prof && ev->evUsed + 4 > (int)ev->ev.size()) {
        int rc = drainProfile(ev);
        if (rc) return rc;
    }
    hipEvent_t* e = prof ? &ev->ev[ev->evUsed] : nullptr;
    hipEvent_t trunkBegin = prof ? e[1] : nullptr, trunkEnd = prof ? e[2] : nullptr;
    if (prof) NSG_HIP(hipEventRecord(e[0], s));
    int rc = NSG_OK;
    switch (form.kind) {
    case nsg::LaunchForm::Team:
    case nsg::LaunchForm::Coop: rc = enqueuePersistent(ev, B, form, s, trunkBegin, trunkEnd); break;
    case nsg::LaunchForm::WholeTrunk: rc = enqueueWholeTrunk(ev, B, form.plan, s, trunkBegin, trunkEnd); break;
    case nsg::LaunchForm::Parts:
    case nsg::LaunchForm::Chains: rc = enqueueForked(ev, B, form, s, trunkBegin, trunkEnd); break;
    case nsg::LaunchForm::Single: rc = enqueueChain(ev, 0, B, form.plan, form.trunkPrec, s, true, trunkBegin, trunkEnd); break;
    }
    if (rc) return rc;
    if (prof) {
        NSG_HIP(hipEventRecord(e[3], s));
        ev->evUsed += 4;
        // launches bracketed by e[1]..e[2]: the 2N residual convs, or the ONE persistent launch
        ev->pendingTrunkLaunchesPerFwd = form.trunkLaunchesPerFwd;
    }
    return NSG_OK;
}

// Second half of every load: adopt the (possibly shared) weights and allocate this evaluator's own
// activation buffers, sized for batchMax.
int finishLoad(nsg_evaluator* ev, std::shared_ptr<NetWeights> W) {
    int rc;
    const int prec = ev->prec;
    const int es = nsg::elemSize(prec);
    ev->G.reset();
    ev->gAct.clear();
    ev->gActPtr.clear();
    ev->gPlanes.release();
    ev->loadedNodes = 0;
    ev->W = std::move(W);
    const NetWeights& N = *ev->W;
    ev->F = N.F; ev->blocks = N.blocks; ev->vc = N.vc; ev->vh = N.vh;
    ev->cpad = N.cpad; ev->headsCout = N.headsCout; ev->fc1K = N.fc1K; ev->params = N.params;
    // activation buffers: whole workgroups of up to 2 boards
    const size_t bpad = (size_t)roundUp(ev->batchMax, 2);
    if ((rc = ev->planes.alloc(bpad * 81 * ev->cpad * es, true))) return rc;
    for (int i = 0; i < 3; ++i)
        if ((rc = ev->act[i].alloc(bpad * 81 * N.F * es, true))) return rc;
    if ((rc = ev->vfeat.alloc((size_t)ev->batchMax * ev->fc1K * es, true))) return rc;
    if ((rc = ev->hidden.alloc((size_t)ev->batchMax * N.vh * 4 * nsg::denseSplits(ev->fc1K, nsg::headPrecision(prec)), true))) return rc;
    ev->seq = nsg::trunkSequence(N.blocks);
    const int nl = (int)ev->seq.steps.size();
    {   // persistent-trunk layer list
        std::vector<unsigned char> host((size_t)nl * nsg::trunkLayerBytes());
        for (int i = 0; i < nl; ++i) {
            const nsg::TrunkStep& t = ev->seq.steps[(size_t)i];
            const ConvLayer& L = trunkWeights(N, t, false);
            nsg::fillTrunkLayer(host.data(), i, trunkBuffer(ev, t.in), L.w.p, (const float*)L.bias.p, trunkBuffer(ev, t.residual),
                                trunkBuffer(ev, t.out), L.cin, N.F, 1, L.accScale,
                                nsg::isMx(prec) && N.blocks > 0 && i == nl - 1);
        }
        if ((rc = ev->trunkLayers.alloc(host.size(), false))) return rc;
        NSG_HIP(hipMemcpy(ev->trunkLayers.p, host.data(), host.size(), hipMemcpyHostToDevice));
        ev->trunkLayerCount = nl;
        const char* env = getenv("NSG_TRUNK_KERNEL");
        ev->useTrunkKernel = !env ? -1 : (env[0] == '1' ? 1 : 0);
    }
    // what the persistent launches with hand-offs share: the event behind the most recent one, the host-mapped give-up word
    if (!ev->teamDone) NSG_HIP(hipEventCreateWithFlags(&ev->teamDone, hipEventDisableTiming));
    if (!ev->teamStatusHost) {
        NSG_HIP(hipHostMalloc((void**)&ev->teamStatusHost, 64, hipHostMallocMapped));
        *ev->teamStatusHost = 0;
        NSG_HIP(hipHostGetDevicePointer((void**)&ev->teamStatusDev, ev->teamStatusHost, 0));
    }
    {   // cooperative trunk (mid batches): flags of (board, member)
        const char* env = getenv("NSG_COOP_TRUNK");
        ev->coopEnabled = (env && env[0] == '0') ? 0 : 1;
        ev->coopForced = (env && env[0] == '1') ? 1 : 0;
        if (prec == nsg::kF16m6 && (N.F == 256 || N.F == 192) && N.blocks >= 1 && ev->coopEnabled) {
            if ((rc = ev->coopFlags.alloc((size_t)ev->batchMax * 24 * sizeof(unsigned), true))) return rc;
        } else {
            ev->coopEnabled = 0;
        }
    }
    // team trunk layer list: the kF16x3 copy of the trunk (an MX evaluator keeps one for batches without an MX plan;
    // a kF16x3 evaluator's own records), the same sequence
    ev->teamLayerCount = 0;
    const bool mxHere = nsg::isMx(prec);
    if ((mxHere || prec == nsg::kF16x3) && N.blocks >= 1 && nsg::teamTrunkSupports(N.F, ev->cpad, 1) &&
        (!mxHere || (N.stemX3.w.p && N.conv1X3.size() == (size_t)N.blocks))) {
        std::vector<nsg::TeamLayer> host((size_t)nl);
        for (int i = 0; i < nl; ++i) {
            const nsg::TrunkStep& t = ev->seq.steps[(size_t)i];
            const ConvLayer& L = trunkWeights(N, t, mxHere);
            host[(size_t)i] = nsg::TeamLayer{(const unsigned char*)trunkBuffer(ev, t.in), (const nsg::team_u32x4*)L.w.p,
                                             (const float*)L.bias.p, (const unsigned char*)trunkBuffer(ev, t.residual),
                                             (unsigned char*)trunkBuffer(ev, t.out), L.cin, N.F, 1, L.accScale};
        }
        if ((rc = ev->teamLayers.alloc(host.size() * sizeof(nsg::TeamLayer), false))) return rc;
        NSG_HIP(hipMemcpy(ev->teamLayers.p, host.data(), host.size() * sizeof(nsg::TeamLayer), hipMemcpyHostToDevice));
        ev->teamBoards = ev->batchMax < nsg::kTeamMaxBoards ? ev->batchMax : nsg::kTeamMaxBoards;
        const size_t setsBytes = 2 * 4 * (size_t)ev->teamBoards * 81 * 1024;
        if ((rc = ev->teamSets.alloc(setsBytes, false))) return rc;
        NSG_HIP(hipMemset(ev->teamSets.p, 0xff, setsBytes));
        ev->teamSet = 0;
        ev->teamDirty[0] = ev->teamDirty[1] = 0;
        ev->teamLayerCount = nl;
        const char* env = getenv("NSG_TEAM_TRUNK");
        ev->teamEnabled = (env && env[0] == '0') ? 0 : 1;
    }
    if ((ev->teamLayerCount > 0 && ev->teamEnabled) || ev->coopEnabled) {
        if (!ev->teamLockHeld) {
            if (teamDeviceLock(ev->gpu)) {
                ev->teamLockHeld = true;
            } else { // another process runs persistent launches with hand-offs on this device
                ev->teamEnabled = 0;
                ev->coopEnabled = 0;
                ev->teamLockedOut = 1;
            }
        }
    }
    NSG_HIP(hipDeviceSynchronize());
    ev->calibKey = -1; // a new network: re-measure the layer time for the chain stagger
    ev->calibPending = false;
    ev->loaded = true;
    return NSG_OK;
}

// Load half of the general graph path: adopt the (possibly shared) plan and allocate this evaluator's activation
// buffers for batchMax.
int finishGraphLoad(nsg_evaluator* ev, std::shared_ptr<GraphWeights> G) {
    int rc;
    const nsg::graph::GraphPlan& P = *G->plan;
    ev->loaded = false;
    ev->W.reset();
    ev->G = std::move(G);
    ev->F = 0; ev->blocks = 0; ev->vc = 0; ev->vh = 0; ev->cpad = 0; ev->headsCout = 0; ev->fc1K = 0;
    ev->params = P.params;
    ev->trunkOut = nullptr;
    ev->lastTrunkPrec = -1;
    // (the specialised path's buffers of an earlier load are not used by a general graph)
    ev->trunkLayerCount = 0;
    ev->teamLayerCount = 0;
    ev->coopEnabled = 0;
    if ((rc = ev->gPlanes.alloc((size_t)ev->batchMax * 81 * P.planeStride * sizeof(float), true))) return rc;
    ev->gAct.clear();
    ev->gActPtr.clear();
    ev->gAct.resize(P.bufSpatialStride.size());
    for (size_t i = 0; i < ev->gAct.size(); ++i) {
        if ((rc = ev->gAct[i].alloc(nsg::graph::bufferFloats(P, i, ev->batchMax) * sizeof(float), true))) return rc;
        ev->gActPtr.push_back((float*)ev->gAct[i].p);
    }
    NSG_HIP(hipDeviceSynchronize());
    ev->loaded = true;
    return NSG_OK;
}

int uploadGraph(nsg_evaluator* ev, std::shared_ptr<const nsg::graph::GraphPlan> plan) {
    int rc = bind(ev);
    if (rc) return rc;
    auto G = std::make_shared<GraphWeights>();
    G->gpu = ev->gpu;
    G->plan = std::move(plan);
    const std::vector<float>& w = G->plan->weights;
    if ((rc = G->w.alloc(w.size() * sizeof(float), false))) return rc;
    if (!w.empty()) NSG_HIP(hipMemcpy(G->w.p, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    return finishGraphLoad(ev, std::move(G));
}

int checkCompute(nsg_evaluator* ev, size_t n) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (!ev->loaded) return fail(NSG_E_NOT_LOADED, "no weights loaded (call nsg_load first)");
    if (n == 0 || n > (size_t)ev->batchMax)
        return fail(NSG_E_INVALID, "batch size %zu outside [1, %d]", n, ev->batchMax);
    // the calling thread may never have called resetGPU for this evaluator (a pipeline's launch
    // thread, a self-play worker's second executor): every launch below must go to ev's device
    return bind(ev);
}

// What a compute call queues behind its forward: the legal-move gather and the D2H copies (trt.cc:265-271).
int enqueueOutputs(nsg_evaluator* ev) {
    const nsg_evaluator::Pending& P = ev->pending;
    if (P.kind == 1) {
        NSG_HIP(hipMemcpyAsync(P.pol, ev->policy.p, P.n * NSG_MOVE_INDEX_MAX * sizeof(float), hipMemcpyDeviceToHost, ev->stream));
    } else if (P.kind == 2) {
        if (P.total) {
            NSG_HIP(nsg::launchGatherLogits((const float*)ev->policy.p, (const uint16_t*)ev->moveIdx.p,
                                            (const uint32_t*)ev->moveOff.p, (float*)ev->gathered.p, (int)P.n, P.softmax, ev->stream));
            NSG_HIP(hipMemcpyAsync(P.vals, ev->gathered.p, P.total * sizeof(float), hipMemcpyDeviceToHost, ev->stream));
        }
    } else {
        return NSG_OK;
    }
    NSG_HIP(hipMemcpyAsync(P.win, ev->value.p, P.n * sizeof(float), hipMemcpyDeviceToHost, ev->stream));
    NSG_HIP(hipMemcpyAsync(P.draw, ev->draw.p, P.n * sizeof(float), hipMemcpyDeviceToHost, ev->stream));
    return NSG_OK;
}

// Called behind every synchronisation of ev->stream that may follow a forward.  A team launch whose members waited
// for each other in vain (a device partition smaller than the grid, another process's persistent kernel on the CUs)
// has raised the host-mapped give-up word and unwound; what it left in the output buffers is undefined.  The batch
// is still in ev->input (and the gather's indices in ev->moveIdx): run it again on the per-layer kernels, issue the
// call's copies again, wait.  The team path stays off for this evaluator from here on; nsg_get_team_stats counts.
int teamRecover(nsg_evaluator* ev) {
    if (!ev->teamStatusHost || *ev->teamStatusHost == 0) return NSG_OK;
    *ev->teamStatusHost = 0;
    if (ev->lastPersistent == 2) ev->coopEnabled = 0; // the cooperative trunk gave up: the per-layer kernels of the same plan
    else ev->teamEnabled = 0;
    ++ev->teamFallbacks;
    releaseTeamToken(ev);
    if (ev->pending.kind == 0 || ev->pending.n == 0 || !ev->teamLast) return NSG_OK;
    --ev->statBatches; // (the same batch, not a new one)
    ev->statPositions -= ev->pending.n;
    int rc = enqueueForward(ev, ev->pending.n);
    if (rc) return rc;
    if ((rc = enqueueOutputs(ev))) return rc;
    NSG_HIP(hipStreamSynchronize(ev->stream));
    return NSG_OK;
}

int syncAndRecover(nsg_evaluator* ev) {
    NSG_HIP(hipStreamSynchronize(ev->stream));
    return teamRecover(ev);
}

} // namespace

extern "C" {

const char* nsg_last_error(void) { return gLastError.c_str(); }
const char* nsg_version(void) { return "nsg 0.1 (gfx950)"; }

// The tuning variables are read when an evaluator is created; a value outside a variable's domain is an
// error there, not a silent "automatic" (a typo must not turn an A/B run into A/A).
static int checkTuningEnv() {
    struct Var { const char* name; long lo, hi; const char* what; };
    static const Var vars[] = {
        {"NSG_CONV_NB", 1, 2, "boards per workgroup"}, {"NSG_CONV_NWAVES", 1, 4, "waves per workgroup"},
        {"NSG_CONV_NFRAG", 1, 4, "fragments per wave (1, 2 or 4)"}, {"NSG_CONV_MSPLIT", 1, 2, "row split"},
        {"NSG_CHAINS", 1, nsg_evaluator::kMaxChains, "half-batch chains"}, {"NSG_TRUNK_KERNEL", 0, 1, "persistent trunk"},
        {"NSG_CHAIN_DELAY_US", -1, 1000000, "chain stagger"}, {"NSG_CHAIN_MIN_BATCH", 2, 65535, "smallest chained batch"},
        {"NSG_KSPLIT4_MAX_BATCH", 0, 65535, "largest batch of the four-way K split"},
        {"NSG_ROWSPLIT8_MAX_BATCH", 0, 65535, "largest batch of the four-way K split with two row groups"},
        {"NSG_SPLIT_BATCH", 0, 1, "full part + remainder batches"},
        {"NSG_SPLIT_BATCH_MAX", 0, 64, "largest batch (quarters of the CU count) that starts with a full chip of two-board tiles"}, {"NSG_ROCTX", 0, 1, "profiler markers"},
        {"NSG_SHARED_FORCE_COPY", 0, 1, "nsg_load_shared copies even on one device"},
        {"NSG_SLAB_SPLIT", 0, 1, "slab-split two-board tiles at mid batches"},
        {"NSG_KSPLIT3", 0, 1, "three-way K split of 192-channel nets at small and mid batches"},
        {"NSG_TEAM_TRUNK", 0, 1, "team trunk for the smallest batches"},
        {"NSG_COOP_TRUNK", 0, 1, "cooperative trunk for the two-way K split of the mid batches"},
        {"NSG_TEAM_MAX_BATCH", 0, 16, "largest batch that runs the team trunk"},
        {"NSG_TEAM_FAULT_LAUNCHES", 0, 1000000, "test hook: team launches made one workgroup short"},
        {"NSG_COOP_FAULT_XCC_LAUNCHES", 0, 1000000, "test hook: cooperative launches whose members claim different XCDs"},
        {"NSG_COOP_FLAG_BASE", 0, (1 << 24) - 1, "test hook: first flag value of the evaluator's first cooperative launch"},
        {"NSG_HEADS_SMALL_BOARDS", 0, 65535, "largest batch whose heads run four one-fragment waves per workgroup (read once per process)"},
        {"NSG_TEAM_MEMBERS", 16, 96, "most workgroups per board of the team trunk on a 256-channel net: 16, 32, 48 or 96 "
                                     "(= 1, 2, 3 or 6 row groups; a 192-channel net runs 12 per row group)"}};
    for (const Var& v : vars) {
        const char* e = getenv(v.name);
        if (!e) continue;
        char* end = nullptr;
        const long x = strtol(e, &end, 10);
        const bool bad = end == e || *end != 0 || x < v.lo || x > v.hi || (!strcmp(v.name, "NSG_CONV_NFRAG") && x == 3) ||
                         (!strcmp(v.name, "NSG_TEAM_MEMBERS") && x != 16 && x != 32 && x != 48 && x != 96);
        if (bad) return fail(NSG_E_INVALID, "%s=%s: expected an integer in [%ld, %ld] (%s)", v.name, e, v.lo, v.hi, v.what);
    }
    return NSG_OK;
}

// NSG_PRECISION: the arithmetic an evaluator starts with when the caller never calls
// nsg_set_precision -- the engine's executor ladders construct, load and run, so
// this is how an unmodified ladder reaches the benchmarked arithmetic.  A number 0..5 or a name.
static int precisionFromEnv(int* prec) {
    const char* e = getenv("NSG_PRECISION");
    if (!e || !*e) return NSG_OK;
    static const char* const names[] = {"fp32", "fp16", "bf16", "f16x3", "f16m8", "f16m6"};
    for (int i = 0; i <= NSG_PRECISION_F16M6; ++i) {
        const char digit[2] = {(char)('0' + i), 0};
        if (!strcasecmp(e, names[i]) || !strcmp(e, digit)) {
            *prec = i;
            return NSG_OK;
        }
    }
    return fail(NSG_E_INVALID, "NSG_PRECISION=%s: expected 0..5 or one of fp32 fp16 bf16 f16x3 f16m8 f16m6", e);
}

int nsg_create(int gpu_id, int batch_size_max, int num_channels, nsg_evaluator** out) {
    if (!out) return fail(NSG_E_INVALID, "null out pointer");
    *out = nullptr;
    if (int trc = checkTuningEnv()) return trc;
    int envPrec = NSG_PRECISION_FP32;
    if (int prc = precisionFromEnv(&envPrec)) return prc;
    if (batch_size_max <= 0 || batch_size_max > 65535 || num_channels <= 0 || num_channels > 1024)
        return fail(NSG_E_INVALID, "bad batch_size_max/num_channels");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(NSG_E_HIP, "no HIP device available (%s): this library has no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (gpu_id < 0 || gpu_id >= count) return fail(NSG_E_INVALID, "gpu_id %d out of range", gpu_id);
    std::unique_ptr<nsg_evaluator> ev(new nsg_evaluator());
    ev->gpu = gpu_id;
    ev->batchMax = batch_size_max;
    ev->numChannels = num_channels;
    ev->prec = envPrec;
    NSG_HIP(hipSetDevice(gpu_id));
    NSG_HIP(hipGetDeviceProperties(&ev->prop, gpu_id));
    int rc;
    // trt.cc:57-77: device buffers sized for BatchSizeMax, zero-initialised
    if ((rc = ev->input.alloc((size_t)batch_size_max * num_channels * NSG_BITBOARD_BYTES, true))) return rc;
    if ((rc = ev->policy.alloc((size_t)batch_size_max * NSG_MOVE_INDEX_MAX * 4, true))) return rc;
    if ((rc = ev->value.alloc((size_t)batch_size_max * 4, true))) return rc;
    if ((rc = ev->draw.alloc((size_t)batch_size_max * 4, true))) return rc;
    // trt.cc:79
    NSG_HIP(hipStreamCreateWithFlags(&ev->stream, hipStreamNonBlocking));
    for (auto& cs : ev->chainStream) NSG_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    NSG_HIP(hipEventCreateWithFlags(&ev->forkEvent, hipEventDisableTiming));
    for (auto& je : ev->joinEvent) NSG_HIP(hipEventCreateWithFlags(&je, hipEventDisableTiming));
    if (const char* e2 = getenv("NSG_CHAINS")) {
        const int v = atoi(e2);
        if (v >= 1 && v <= nsg_evaluator::kMaxChains) ev->numChains = v;
    }
    ev->tuning = nsg::readConvTuning();
    for (auto& ce : ev->calibEv) NSG_HIP(hipEventCreate(&ce));
    if (const char* e2 = getenv("NSG_CHAIN_DELAY_US")) ev->chainDelayUs = std::max(-1, atoi(e2));
    if (const char* e2 = getenv("NSG_CHAIN_MIN_BATCH")) ev->chainMinBatch = std::max(2, atoi(e2));
    if (const char* e2 = getenv("NSG_TEAM_MEMBERS")) ev->teamForceRowGroups = atoi(e2) / 16; // (validated above)
    if (const char* e2 = getenv("NSG_TEAM_FAULT_LAUNCHES")) ev->teamFaultLaunches = std::max(0, atoi(e2));
    if (const char* e2 = getenv("NSG_COOP_FAULT_XCC_LAUNCHES")) ev->coopFaultXccLaunches = std::max(0, atoi(e2));
    if (const char* e2 = getenv("NSG_COOP_FLAG_BASE")) ev->coopFlagBase = (unsigned)std::max(0, atoi(e2));
    if (const char* e2 = getenv("NSG_TEAM_MAX_BATCH")) ev->teamMaxBatch = std::min(std::max(0, atoi(e2)), (int)nsg::kTeamMaxBoards);
    *out = ev.release();
    return NSG_OK;
}

int nsg_destroy(nsg_evaluator* ev) {
    if (!ev) return NSG_OK;
    (void)hipSetDevice(ev->gpu);
    if (ev->stream) {
        (void)hipStreamSynchronize(ev->stream);
    }
    if (ev->teamStatusHost) *ev->teamStatusHost = 0;
    releaseTeamToken(ev);
    if (ev->teamLockHeld) teamDeviceUnlock(ev->gpu);
#ifdef TEAM_STAMPS
    if (ev->teamLayerCount) nsg::teamTrunkDumpStamps();
#endif
    if (ev->teamStatusHost) (void)hipHostFree(ev->teamStatusHost);
    if (ev->teamDone) (void)hipEventDestroy(ev->teamDone); // (a stream that waits for it keeps what it needs)
    for (hipEvent_t e : ev->ev) (void)hipEventDestroy(e);
    for (auto cs : ev->chainStream)
        if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); }
    if (ev->forkEvent) (void)hipEventDestroy(ev->forkEvent);
    for (auto je : ev->joinEvent)
        if (je) (void)hipEventDestroy(je);
    for (auto ce : ev->calibEv)
        if (ce) (void)hipEventDestroy(ce);
    if (ev->stream) (void)hipStreamDestroy(ev->stream);
    delete ev;
    return NSG_OK;
}

int nsg_set_precision(nsg_evaluator* ev, int precision) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (ev->loaded) return fail(NSG_E_INVALID, "precision must be chosen before nsg_load");
    if (precision < NSG_PRECISION_FP32 || precision > NSG_PRECISION_F16M6)
        return fail(NSG_E_INVALID, "unknown precision %d", precision);
    ev->prec = precision;
    return NSG_OK;
}

int nsg_convert_onnx(const void* onnx, size_t size, void* dst, size_t capacity, size_t* nsgw_size) {
    if (!onnx || !nsgw_size) return fail(NSG_E_INVALID, "null argument");
    std::vector<unsigned char> blob;
    std::string err;
    if (!nsg::onnx::convertToNsgw(onnx, size, &blob, &err)) return fail(NSG_E_FORMAT, "%s", err.c_str());
    *nsgw_size = blob.size();
    if (dst) {
        if (capacity < blob.size()) return fail(NSG_E_INVALID, "destination holds %zu bytes, %zu needed", capacity, blob.size());
        memcpy(dst, blob.data(), blob.size());
    }
    return NSG_OK;
}

int nsg_load_memory(nsg_evaluator* ev, const void* blob, size_t size) {
    if (!ev || !blob) return fail(NSG_E_INVALID, "null argument");
    if (!nsg::onnx::isNsgw(blob, size)) { // what the engine passes: an ONNX model (trt.cc:121-131)
        // the family matcher and the specialised loader first; what either refuses goes to the general graph planner
        std::string famErr = "not tried (graph mode 1)";
        if (ev->graphMode != NSG_GRAPH_FORCE) {
            std::vector<unsigned char> converted;
            if (nsg::onnx::convertToNsgw(blob, size, &converted, &famErr)) {
                const int rc = nsg_load_memory(ev, converted.data(), converted.size());
                if (rc == NSG_OK) ev->loadedNodes = nsg::graph::countNodes(blob, size);
                if (rc != NSG_E_FORMAT) return rc;
                famErr = gLastError;
            }
        }
        auto plan = std::make_shared<nsg::graph::GraphPlan>();
        std::string graphErr;
        if (!nsg::graph::buildPlan(blob, size, ev->numChannels, plan.get(), &graphErr))
            return fail(NSG_E_FORMAT, "Failed to parse the model: neither an NSGW v1 weight file nor an ONNX model that "
                                      "loads (specialised path: %s; general graph path: %s)", famErr.c_str(), graphErr.c_str());
        return uploadGraph(ev, std::move(plan));
    }
    int rc = bind(ev);
    if (rc) return rc;
    const int prec = ev->prec;
    const char* guard = getenv("NSG_M8_GUARD");
    nsg::PreparedNet P;
    std::string err;
    if ((rc = nsg::prepareNet(blob, size, prec, ev->numChannels, !(guard && guard[0] == '0'), &P, &err)))
        return fail(rc, "%s", err.c_str());

    ev->loaded = false;
    auto W = std::make_shared<NetWeights>();
    W->gpu = ev->gpu; W->prec = prec;
    W->F = P.F; W->blocks = P.blocks; W->vc = P.vc; W->vh = P.vh; W->cin = P.cin;
    W->cpad = P.cpad; W->headsCout = P.headsCout; W->fc1K = P.fc1K; W->params = P.params;
    W->actBound = P.actBound; W->outsideM8Window = P.outsideM8Window;
    // every layer in turn: its host image is released as soon as it is on the device
    const bool mx = nsg::isMx(prec); // ... holds the trunk in kF16x3 form too
    W->conv1.resize(P.blocks); W->conv2.resize(P.blocks);
    if (mx) { W->conv1X3.resize(P.blocks); W->conv2X3.resize(P.blocks); }
    if ((rc = commitLayer(P.stem, &W->stem)) || (mx && (rc = commitLayer(P.stemX3, &W->stemX3)))) return rc;
    for (int k = 0; k < P.blocks; ++k)
        if ((rc = commitLayer(P.conv1[k], &W->conv1[k])) || (mx && (rc = commitLayer(P.conv1X3[k], &W->conv1X3[k]))) ||
            (rc = commitLayer(P.conv2[k], &W->conv2[k])) || (mx && (rc = commitLayer(P.conv2X3[k], &W->conv2X3[k]))))
            return rc;
    if ((rc = commitLayer(P.heads, &W->heads)) || (rc = commitLayer(P.fc1, &W->fc1))) return rc;
    if ((rc = W->fc2W.alloc(P.fc2W.size() * 4, false))) return rc;
    if ((rc = W->fc2B.alloc(P.fc2B.size() * 4, false))) return rc;
    NSG_HIP(hipMemcpy(W->fc2W.p, P.fc2W.data(), P.fc2W.size() * 4, hipMemcpyHostToDevice));
    NSG_HIP(hipMemcpy(W->fc2B.p, P.fc2B.data(), P.fc2B.size() * 4, hipMemcpyHostToDevice));
    return finishLoad(ev, std::move(W));
}

// Loads `ev` with the network `src` already holds, without touching the model file again: the
// self-play driver's G x T executors (selfplay/main.cc:189-195, mcts/manager.cc:168-179 -- where
// every executor re-reads and re-builds the model) share ONE upload per device and one peer copy
// (hipMemcpyPeer over xGMI) per further device.
int nsg_load_shared(nsg_evaluator* ev, nsg_evaluator* src) {
    if (!ev || !src) return fail(NSG_E_INVALID, "null argument");
    if (!src->loaded || (!src->W && !src->G)) return fail(NSG_E_NOT_LOADED, "the source evaluator has no weights loaded");
    if (ev == src) return NSG_OK;
    if (src->G) { // a general graph: the same plan, shared on one device, uploaded again on another
        if (ev->numChannels != src->G->plan->numChannels)
            return fail(NSG_E_FORMAT, "network expects %d input planes, evaluator has %d", src->G->plan->numChannels, ev->numChannels);
        if (ev->gpu == src->gpu) {
            int rc = bind(ev);
            return rc ? rc : finishGraphLoad(ev, src->G);
        }
        return uploadGraph(ev, src->G->plan);
    }
    if (ev->prec != src->W->prec) return fail(NSG_E_INVALID, "precision differs from the source evaluator's");
    if (ev->numChannels != src->W->cin)
        return fail(NSG_E_FORMAT, "network expects %d input planes, evaluator has %d", src->W->cin, ev->numChannels);
    int rc = bind(ev);
    if (rc) return rc;
    ev->loaded = false;
    // NSG_SHARED_FORCE_COPY=1: take the other-device branch (own allocations + hipMemcpyPeer) for an evaluator of
    // the SAME device too, so the branch a multi-GPU process runs can be exercised on a one-GPU machine.
    static const bool forceCopy = [] { const char* e = getenv("NSG_SHARED_FORCE_COPY"); return e && atoi(e) == 1; }();
    if (ev->gpu == src->gpu && !forceCopy) return finishLoad(ev, src->W);
    const NetWeights& S = *src->W;
    auto W = std::make_shared<NetWeights>();
    W->gpu = ev->gpu; W->prec = S.prec;
    W->F = S.F; W->blocks = S.blocks; W->vc = S.vc; W->vh = S.vh; W->cin = S.cin; W->cpad = S.cpad;
    W->headsCout = S.headsCout; W->fc1K = S.fc1K; W->params = S.params;
    W->actBound = S.actBound; W->outsideM8Window = S.outsideM8Window;
    auto copyBuf = [&](const DevBuf& s, DevBuf* d) -> int {
        if (!s.p) return NSG_OK;
        int r = d->alloc(s.bytes, false);
        if (r) return r;
        NSG_HIP(hipMemcpyPeer(d->p, ev->gpu, s.p, S.gpu, s.bytes));
        return NSG_OK;
    };
    auto copyLayer = [&](const ConvLayer& s, ConvLayer* d) -> int {
        d->cin = s.cin; d->accScale = s.accScale;
        int r = copyBuf(s.w, &d->w);
        return r ? r : copyBuf(s.bias, &d->bias);
    };
    auto copyLayers = [&](const std::vector<ConvLayer>& s, std::vector<ConvLayer>* d) -> int {
        d->resize(s.size());
        for (size_t i = 0; i < s.size(); ++i) { int r = copyLayer(s[i], &(*d)[i]); if (r) return r; }
        return NSG_OK;
    };
    if ((rc = copyLayer(S.stem, &W->stem)) || (rc = copyLayer(S.stemX3, &W->stemX3)) ||
        (rc = copyLayers(S.conv1, &W->conv1)) || (rc = copyLayers(S.conv2, &W->conv2)) ||
        (rc = copyLayers(S.conv1X3, &W->conv1X3)) || (rc = copyLayers(S.conv2X3, &W->conv2X3)) ||
        (rc = copyLayer(S.heads, &W->heads)) || (rc = copyLayer(S.fc1, &W->fc1)) ||
        (rc = copyBuf(S.fc2W, &W->fc2W)) || (rc = copyBuf(S.fc2B, &W->fc2B)))
        return rc;
    NSG_HIP(hipDeviceSynchronize());
    return finishLoad(ev, std::move(W));
}

int nsg_load(nsg_evaluator* ev, const char* path) {
    if (!ev || !path) return fail(NSG_E_INVALID, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) return fail(NSG_E_IO, "Could not open the file: %s", path); // trt.cc:34-36
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (sz <= 0) {
        fclose(f);
        return fail(NSG_E_IO, "empty weight file: %s", path);
    }
    std::vector<unsigned char> blob((size_t)sz);
    const size_t got = fread(blob.data(), 1, (size_t)sz, f);
    fclose(f);
    if (got != (size_t)sz) return fail(NSG_E_IO, "short read on %s", path);
    return nsg_load_memory(ev, blob.data(), blob.size());
}

int nsg_load_device_blob(nsg_evaluator* ev, const void* device_blob, size_t size) {
    if (!ev || !device_blob) return fail(NSG_E_INVALID, "null argument");
    int rc = bind(ev);
    if (rc) return rc;
    std::vector<unsigned char> blob(size);
    NSG_HIP(hipMemcpy(blob.data(), device_blob, size, hipMemcpyDeviceToHost));
    return nsg_load_memory(ev, blob.data(), size);
}

int nsg_compute_nonblocking(nsg_evaluator* ev, const void* features, size_t batch_size,
                            float* dst_policy, float* dst_win_rate, float* dst_draw_rate) {
    int rc = checkCompute(ev, batch_size);
    if (rc) return rc;
    if (!features || !dst_policy || !dst_win_rate || !dst_draw_rate)
        return fail(NSG_E_INVALID, "null buffer");
    // trt.cc:237-238: exactly one batch in flight per executor
    if (hipStreamQuery(ev->stream) == hipErrorNotReady)
        return fail(NSG_E_BUSY, "computeNonBlocking called while a batch is in flight");
    // trt.cc:240-242
    {
        Range r("nsg.h2d");
        NSG_HIP(hipMemcpyAsync(ev->input.p, features,
                               batch_size * ev->numChannels * NSG_BITBOARD_BYTES,
                               hipMemcpyHostToDevice, ev->stream));
    }
    ev->pending = nsg_evaluator::Pending{1, batch_size, 0, 0, dst_policy, dst_win_rate, dst_draw_rate, nullptr};
    if ((rc = enqueueForward(ev, batch_size))) return rc;
    Range d2h("nsg.d2h");
    return enqueueOutputs(ev); // trt.cc:265-271
}

int nsg_compute_gather_nonblocking(nsg_evaluator* ev, const void* features, size_t batch_size,
                                   const uint16_t* move_indices, const uint32_t* move_offsets,
                                   int softmax, float* dst_values, float* dst_win_rate,
                                   float* dst_draw_rate) {
    int rc = checkCompute(ev, batch_size);
    if (rc) return rc;
    if (!features || !move_indices || !move_offsets || !dst_values || !dst_win_rate || !dst_draw_rate)
        return fail(NSG_E_INVALID, "null buffer");
    if (move_offsets[0] != 0) return fail(NSG_E_INVALID, "move_offsets[0] must be 0");
    for (size_t b = 0; b < batch_size; ++b)
        if (move_offsets[b + 1] < move_offsets[b] || move_offsets[b + 1] - move_offsets[b] > NSG_MAX_LEGAL_MOVES)
            return fail(NSG_E_INVALID, "move_offsets must be non-decreasing with at most %d moves per position",
                        NSG_MAX_LEGAL_MOVES);
    const size_t total = move_offsets[batch_size];
    if (hipStreamQuery(ev->stream) == hipErrorNotReady)
        return fail(NSG_E_BUSY, "compute called while a batch is in flight");
    if (!ev->moveIdx.p) {
        const size_t cap = (size_t)ev->batchMax * NSG_MAX_LEGAL_MOVES;
        if ((rc = ev->moveIdx.alloc(cap * sizeof(uint16_t), false))) return rc;
        if ((rc = ev->moveOff.alloc(((size_t)ev->batchMax + 1) * sizeof(uint32_t), false))) return rc;
        if ((rc = ev->gathered.alloc(cap * sizeof(float), false))) return rc;
    }
    NSG_HIP(hipMemcpyAsync(ev->input.p, features, batch_size * ev->numChannels * NSG_BITBOARD_BYTES,
                           hipMemcpyHostToDevice, ev->stream));
    NSG_HIP(hipMemcpyAsync(ev->moveOff.p, move_offsets, (batch_size + 1) * sizeof(uint32_t),
                           hipMemcpyHostToDevice, ev->stream));
    if (total)
        NSG_HIP(hipMemcpyAsync(ev->moveIdx.p, move_indices, total * sizeof(uint16_t), hipMemcpyHostToDevice,
                               ev->stream));
    ev->pending = nsg_evaluator::Pending{2, batch_size, total, softmax ? 1 : 0, nullptr, dst_win_rate, dst_draw_rate, dst_values};
    if ((rc = enqueueForward(ev, batch_size))) return rc;
    return enqueueOutputs(ev);
}

int nsg_compute_gather_blocking(nsg_evaluator* ev, const void* features, size_t batch_size,
                                const uint16_t* move_indices, const uint32_t* move_offsets,
                                int softmax, float* dst_values, float* dst_win_rate,
                                float* dst_draw_rate) {
    int rc = nsg_compute_gather_nonblocking(ev, features, batch_size, move_indices, move_offsets, softmax,
                                            dst_values, dst_win_rate, dst_draw_rate);
    if (rc) return rc;
    return nsg_await(ev);
}

int nsg_await(nsg_evaluator* ev) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    int rc = bind(ev);
    if (rc) return rc;
    // trt.cc:281-283; a team launch that gave up is re-run on the per-layer kernels before this returns (teamRecover):
    // the caller sees a slow batch, not a lost one
    return syncAndRecover(ev);
}

int nsg_compute_blocking(nsg_evaluator* ev, const void* features, size_t batch_size,
                         float* dst_policy, float* dst_win_rate, float* dst_draw_rate) {
    int rc = nsg_compute_nonblocking(ev, features, batch_size, dst_policy, dst_win_rate,
                                     dst_draw_rate); // trt.cc:274-279
    if (rc) return rc;
    return nsg_await(ev);
}

int nsg_is_computing(nsg_evaluator* ev) {
    if (!ev) return 0;
    return hipStreamQuery(ev->stream) == hipErrorNotReady ? 1 : 0; // trt.cc:285-287
}

int nsg_reset_gpu(nsg_evaluator* ev) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    return bind(ev); // trt.cc:289-291
}

int nsg_extract_bits(float* dst, const uint64_t* src, int batch_size, int num_channels,
                     int channels_first, void* hip_stream) {
    if (!dst || !src || batch_size <= 0 || num_channels <= 0)
        return fail(NSG_E_INVALID, "bad extract_bits argument"); // extractbit.cu:78 assert
    if (!channels_first && num_channels > 1024)
        return fail(NSG_E_INVALID, "NumChannels > 1024"); // extractbit.cu:91
    hipStream_t s = (hipStream_t)hip_stream;
    if (channels_first) {
        NSG_HIP(nsg::launchExtractBitsNCHW(dst, src, batch_size, num_channels, s));
    } else {
        NSG_HIP(nsg::launchExtractBitsNHWC(dst, src, batch_size, num_channels, s));
    }
    return NSG_OK;
}

int nsg_host_register(void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return fail(NSG_E_INVALID, "bad host_register argument");
    NSG_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return NSG_OK;
}

int nsg_host_unregister(void* ptr) {
    if (!ptr) return fail(NSG_E_INVALID, "null pointer");
    NSG_HIP(hipHostUnregister(ptr));
    return NSG_OK;
}

int nsg_upload_features(nsg_evaluator* ev, const void* features, size_t batch_size) {
    if (!ev || !features || batch_size == 0 || batch_size > (size_t)ev->batchMax)
        return fail(NSG_E_INVALID, "bad upload_features argument");
    int rc = bind(ev);
    if (rc) return rc;
    if ((rc = syncAndRecover(ev))) return rc; // (before the batch a forward in flight still reads is overwritten)
    ev->pending = nsg_evaluator::Pending{};
    NSG_HIP(hipMemcpyAsync(ev->input.p, features, batch_size * ev->numChannels * NSG_BITBOARD_BYTES,
                           hipMemcpyHostToDevice, ev->stream));
    NSG_HIP(hipStreamSynchronize(ev->stream));
    return NSG_OK;
}

int nsg_forward_resident(nsg_evaluator* ev, size_t batch_size) {
    int rc = checkCompute(ev, batch_size);
    if (rc) return rc;
    ev->pending = nsg_evaluator::Pending{3, batch_size, 0, 0, nullptr, nullptr, nullptr, nullptr};
    return enqueueForward(ev, batch_size);
}

int nsg_download_outputs(nsg_evaluator* ev, size_t batch_size, float* dst_policy,
                         float* dst_win_rate, float* dst_draw_rate) {
    int rc = checkCompute(ev, batch_size);
    if (rc) return rc;
    if ((rc = syncAndRecover(ev))) return rc;
    NSG_HIP(hipMemcpyAsync(dst_policy, ev->policy.p, batch_size * NSG_MOVE_INDEX_MAX * sizeof(float),
                           hipMemcpyDeviceToHost, ev->stream));
    NSG_HIP(hipMemcpyAsync(dst_win_rate, ev->value.p, batch_size * sizeof(float),
                           hipMemcpyDeviceToHost, ev->stream));
    NSG_HIP(hipMemcpyAsync(dst_draw_rate, ev->draw.p, batch_size * sizeof(float),
                           hipMemcpyDeviceToHost, ev->stream));
    NSG_HIP(hipStreamSynchronize(ev->stream));
    return NSG_OK;
}

int nsg_download_trunk(nsg_evaluator* ev, size_t batch_size, float* dst) {
    int rc = checkCompute(ev, batch_size);
    if (rc) return rc;
    if (ev->G) return fail(NSG_E_INVALID, "%s: the loaded network runs on the general graph path, which has no trunk or "
                                          "plane buffer of the specialised layout", "nsg_download_trunk");
    if (!ev->trunkOut) return fail(NSG_E_INVALID, "no forward has run yet");
    if ((rc = syncAndRecover(ev))) return rc;
    const size_t bytes = batch_size * ev->F * 81 * sizeof(float);
    if (ev->scratch.bytes < bytes && (rc = ev->scratch.alloc(bytes, false))) return rc;
    NSG_HIP(nsg::launchActToNCHW(ev->trunkOut, (float*)ev->scratch.p, (int)batch_size, ev->F,
                                 nsg::headPrecision(ev->prec), ev->stream));
    NSG_HIP(hipMemcpyAsync(dst, ev->scratch.p, bytes, hipMemcpyDeviceToHost, ev->stream));
    NSG_HIP(hipStreamSynchronize(ev->stream));
    return NSG_OK;
}

int nsg_download_planes_raw(nsg_evaluator* ev, size_t batch_size, void* dst, size_t capacity, size_t* row_bytes) {
    int rc = checkCompute(ev, batch_size);
    if (rc) return rc;
    if (ev->G) return fail(NSG_E_INVALID, "%s: the loaded network runs on the general graph path, which has no trunk or "
                                          "plane buffer of the specialised layout", "nsg_download_planes_raw");
    if (!ev->trunkOut) return fail(NSG_E_INVALID, "no forward has run yet");
    if ((rc = syncAndRecover(ev))) return rc;
    if (ev->teamLast && ev->lastPersistent == 1)
        return fail(NSG_E_INVALID, "the last forward ran the team trunk, which decodes the bitboards inside its first layer: "
                                   "there is no plane buffer for it (NSG_TEAM_TRUNK=0 keeps the per-layer kernels)");
    if (!dst || !row_bytes) return fail(NSG_E_INVALID, "null argument");
    const size_t es = nsg::elemSize(ev->lastTrunkPrec);
    const size_t rb = (size_t)ev->cpad * es;
    const size_t bytes = batch_size * 81 * rb;
    if (capacity < bytes) return fail(NSG_E_INVALID, "destination holds %zu bytes, %zu needed", capacity, bytes);
    NSG_HIP(hipMemcpyAsync(dst, ev->planes.p, bytes, hipMemcpyDeviceToHost, ev->stream));
    NSG_HIP(hipStreamSynchronize(ev->stream));
    *row_bytes = rb;
    return NSG_OK;
}

int nsg_time_planes(nsg_evaluator* ev, size_t batch_size, int iterations, float* avg_ms, double* bytes_per_launch) {
    int rc = checkCompute(ev, batch_size);
    if (rc) return rc;
    if (ev->G) return fail(NSG_E_INVALID, "%s: the loaded network runs on the general graph path, which has no trunk or "
                                          "plane buffer of the specialised layout", "nsg_time_planes");
    if (iterations < 1 || !avg_ms) return fail(NSG_E_INVALID, "bad time_planes argument");
    if ((rc = syncAndRecover(ev))) return rc;
    const int prec = ev->prec;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    NSG_HIP(hipEventCreate(&e0));
    NSG_HIP(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i)
        NSG_HIP(nsg::launchExtractBitsAct(ev->planes.p, (const uint64_t*)ev->input.p, (int)batch_size, ev->numChannels, ev->cpad, prec, ev->stream));
    NSG_HIP(hipEventRecord(e0, ev->stream));
    for (int i = 0; i < iterations; ++i)
        NSG_HIP(nsg::launchExtractBitsAct(ev->planes.p, (const uint64_t*)ev->input.p, (int)batch_size, ev->numChannels, ev->cpad, prec, ev->stream));
    NSG_HIP(hipEventRecord(e1, ev->stream));
    NSG_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    NSG_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_ms = ms / (float)iterations;
    // algorithmic bytes: the bitboards read + the trunk-input rows written ([81][cpad] elements per position)
    if (bytes_per_launch)
        *bytes_per_launch = (double)batch_size * ((double)ev->numChannels * NSG_BITBOARD_BYTES + 81.0 * ev->cpad * nsg::elemSize(prec));
    return NSG_OK;
}

int nsg_profile_enable(nsg_evaluator* ev, int enable) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    int rc = bind(ev);
    if (rc) return rc;
    if (enable && ev->ev.empty()) {
        ev->ev.resize(kMaxEventPairs * 4);
        for (auto& e : ev->ev) NSG_HIP(hipEventCreate(&e));
    }
    if (!enable && (rc = drainProfile(ev))) return rc;
    ev->profile = enable != 0;
    return NSG_OK;
}

int nsg_profile_read(nsg_evaluator* ev, double* trunk_ms_total, uint64_t* trunk_launches,
                     double* forward_ms_total, uint64_t* forwards) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    int rc = drainProfile(ev);
    if (rc) return rc;
    if (trunk_ms_total) *trunk_ms_total = ev->trunkMs;
    if (trunk_launches) *trunk_launches = ev->trunkLaunches;
    if (forward_ms_total) *forward_ms_total = ev->fwdMs;
    if (forwards) *forwards = ev->forwards;
    ev->trunkMs = ev->fwdMs = 0;
    ev->trunkLaunches = ev->forwards = 0;
    return NSG_OK;
}

int nsg_get_stats(nsg_evaluator* ev, uint64_t* batches, uint64_t* positions) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (batches) *batches = ev->statBatches;
    if (positions) *positions = ev->statPositions;
    return NSG_OK;
}

int nsg_get_team_stats(nsg_evaluator* ev, int* enabled, int* members_last, uint64_t* fallbacks) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (enabled) *enabled = (ev->teamLayerCount > 0 && ev->teamEnabled) ? 1 : (ev->teamLockedOut ? -1 : 0);
    if (members_last) *members_last = ev->teamLastMembers;
    if (fallbacks) *fallbacks = ev->teamFallbacks;
    return NSG_OK;
}

int nsg_get_last_launch_kind(nsg_evaluator* ev, int* kind, int* coop_enabled) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (kind) *kind = ev->lastPersistent;
    if (coop_enabled) *coop_enabled = ev->coopEnabled ? 1 : (ev->teamLockedOut ? -1 : 0);
    return NSG_OK;
}

int nsg_get_last_launch_form(nsg_evaluator* ev, int* whole_trunk, int* parts) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (whole_trunk) *whole_trunk = ev->lastWholeTrunk;
    if (parts) *parts = ev->lastParts;
    return NSG_OK;
}

int nsg_get_last_plan(nsg_evaluator* ev, int* nb, int* nfrag, int* nwaves, int* chains) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (nb) *nb = ev->lastPlan.nb;
    if (nfrag) *nfrag = ev->lastPlan.nfrag;
    if (nwaves) *nwaves = ev->lastPlan.nwaves;
    if (chains) *chains = ev->lastChains;
    return NSG_OK;
}

int nsg_get_last_split(nsg_evaluator* ev, int* row_split, int* k_split) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (row_split) *row_split = ev->lastPlan.nb ? ev->lastPlan.msplit : 0;
    if (k_split) *k_split = ev->lastPlan.nb ? ev->lastPlan.ksplit : 0;
    return NSG_OK;
}

int nsg_get_last_slab_split(nsg_evaluator* ev, int* slab_split) {
    if (!ev || !slab_split) return fail(NSG_E_INVALID, "null argument");
    *slab_split = ev->lastPlan.nb ? ev->lastPlan.sslab : 0;
    return NSG_OK;
}

int nsg_get_last_trunk_precision(nsg_evaluator* ev, int* precision) {
    if (!ev || !precision) return fail(NSG_E_INVALID, "null argument");
    *precision = ev->lastTrunkPrec;
    return NSG_OK;
}

int nsg_get_launch_form(nsg_evaluator* ev, int batch, int* kind, int* whole_trunk, int* parts, int* nb, int* nfrag,
                        int* nwaves, int* chains, int* row_split, int* k_split, int* slab_split, int* precision) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (!ev->loaded) return fail(NSG_E_NOT_LOADED, "no network loaded");
    if (batch <= 0 || batch > ev->batchMax) return fail(NSG_E_INVALID, "batch %d outside 1..%d", batch, ev->batchMax);
    nsg::LaunchForm f; // (the general graph path: what enqueueGraph reports)
    if (!ev->G) f = nsg::chooseLaunchForm(launchConfigOf(ev), batch);
    else f.chains = 0;
    if (kind) *kind = f.kind == nsg::LaunchForm::Team ? 1 : f.kind == nsg::LaunchForm::Coop ? 2 : 0;
    if (whole_trunk) *whole_trunk = f.kind == nsg::LaunchForm::WholeTrunk ? 1 : 0;
    if (parts) *parts = f.nParts;
    if (nb) *nb = f.plan.nb;
    if (nfrag) *nfrag = f.plan.nfrag;
    if (nwaves) *nwaves = f.plan.nwaves;
    if (chains) *chains = f.chains;
    if (row_split) *row_split = f.plan.nb ? f.plan.msplit : 0;
    if (k_split) *k_split = f.plan.nb ? f.plan.ksplit : 0;
    if (slab_split) *slab_split = f.plan.nb ? f.plan.sslab : 0;
    if (precision) *precision = f.trunkPrec;
    return NSG_OK;
}

int nsg_get_info(nsg_evaluator* ev, nsg_info* info) {
    if (!ev || !info) return fail(NSG_E_INVALID, "null argument");
    memset(info, 0, sizeof(*info));
    info->gpu_id = ev->gpu;
    info->batch_size_max = ev->batchMax;
    info->num_channels = ev->numChannels;
    info->channels = ev->F;
    info->blocks = ev->blocks;
    info->value_channels = ev->vc;
    info->value_hidden = ev->vh;
    info->precision = ev->prec;
    info->loaded = ev->loaded ? 1 : 0;
    info->compute_units = ev->prop.multiProcessorCount;
    info->clock_khz = ev->prop.clockRate;
    info->param_count = ev->params;
    const double F = ev->F, N = ev->blocks, C = ev->numChannels;
    // stem + trunk + 1x1 policy (value/draw heads excluded); a general graph: every conv and dense layer
    info->flops_per_position = ev->G ? ev->G->plan->flopsPerPosition
                                     : 2.0 * 81 * 9 * C * F + N * 2 * (2.0 * 81 * 9 * F * F) + 2.0 * 81 * 27 * F;
    info->trunk_conv_flops_per_position = 2.0 * 81 * 9 * F * F;
    info->activation_bound_estimate = ev->W ? ev->W->actBound : 0.0;
    info->f16m8_window_fallback = (ev->W && ev->W->outsideM8Window) ? 1 : 0;
    // (boxes without the amdgpu.ids table report an empty marketing name: fall back to the ISA name)
    snprintf(info->device_name, sizeof(info->device_name), "%s", ev->prop.name[0] ? ev->prop.name : ev->prop.gcnArchName);
    return NSG_OK;
}

int nsg_set_graph_mode(nsg_evaluator* ev, int mode) {
    if (!ev) return fail(NSG_E_INVALID, "null evaluator");
    if (ev->loaded) return fail(NSG_E_INVALID, "the graph mode must be chosen before nsg_load");
    if (mode != NSG_GRAPH_AUTO && mode != NSG_GRAPH_FORCE) return fail(NSG_E_INVALID, "unknown graph mode %d", mode);
    ev->graphMode = mode;
    return NSG_OK;
}

static void graphInfoFromPlan(const nsg::graph::GraphPlan& P, nsg_graph_info* info) {
    info->path = NSG_PATH_GRAPH;
    info->precision = NSG_PRECISION_FP32;
    info->nodes = P.nodes;
    info->launches = (int)P.launches.size() + 2; // + plane expansion + output scatter
    info->conv_launches = P.convLaunches;
    info->attention_launches = P.attentionLaunches;
    info->param_count = P.params;
    info->flops_per_position = P.flopsPerPosition;
    info->activation_bytes_per_position = P.activationBytesPerPosition;
}

static void graphInfoFamily(const nsg::NetView& nv, int nodes, int prec, nsg_graph_info* info) {
    info->path = NSG_PATH_SPECIALISED;
    info->precision = prec;
    info->nodes = nodes;
    info->param_count = nv.params;
    const double F = nv.F, N = nv.blocks, C = nv.cin;
    info->flops_per_position = 2.0 * 81 * 9 * C * F + N * 2 * (2.0 * 81 * 9 * F * F) + 2.0 * 81 * 27 * F;
}

int nsg_get_graph_info(nsg_evaluator* ev, nsg_graph_info* info) {
    if (!ev || !info) return fail(NSG_E_INVALID, "null argument");
    if (!ev->loaded) return fail(NSG_E_NOT_LOADED, "no network loaded");
    memset(info, 0, sizeof(*info));
    if (ev->G) {
        graphInfoFromPlan(*ev->G->plan, info);
        info->activation_bytes = ev->gPlanes.bytes;
        for (const DevBuf& b : ev->gAct) info->activation_bytes += b.bytes;
        return NSG_OK;
    }
    info->path = NSG_PATH_SPECIALISED;
    info->precision = ev->prec;
    info->nodes = ev->loadedNodes;
    info->param_count = ev->params;
    const double F = ev->F, N = ev->blocks, C = ev->numChannels;
    info->flops_per_position = 2.0 * 81 * 9 * C * F + N * 2 * (2.0 * 81 * 9 * F * F) + 2.0 * 81 * 27 * F;
    return NSG_OK;
}

int nsg_inspect_onnx(const void* onnx, size_t size, int num_channels, nsg_graph_info* info) {
    if (!onnx || !info || num_channels <= 0) return fail(NSG_E_INVALID, "bad argument");
    memset(info, 0, sizeof(*info));
    std::string famErr;
    std::vector<unsigned char> converted;
    if (nsg::onnx::convertToNsgw(onnx, size, &converted, &famErr)) {
        nsg::NetView nv;
        int rc = nsg::parseBlob(converted.data(), converted.size(), &nv, &famErr);
        if (rc == NSG_OK && (rc = nsg::checkSpecialised(nv, num_channels, &famErr)) == NSG_OK) {
            graphInfoFamily(nv, nsg::graph::countNodes(onnx, size), NSG_PRECISION_FP32, info);
            return NSG_OK;
        }
    }
    nsg::graph::GraphPlan plan;
    std::string graphErr;
    if (!nsg::graph::buildPlan(onnx, size, num_channels, &plan, &graphErr))
        return fail(NSG_E_FORMAT, "Failed to parse the model: neither an NSGW v1 weight file nor an ONNX model that "
                                  "loads (specialised path: %s; general graph path: %s)", famErr.c_str(), graphErr.c_str());
    graphInfoFromPlan(plan, info);
    return NSG_OK;
}

#ifdef NSG_DIAG_STAMPS
// Diagnostic library only (make diag): cycle stamps of every trunk-conv workgroup.
// layout: [layer][4096 workgroups][8 u64] = entry, prologue done, main loop done,
// epilogue done (s_memtime), -, -, s_memrealtime at epilogue done / at entry.
int nsg_debug_stamps_enable(nsg_evaluator* ev) {
    if (!ev || !ev->loaded) return fail(NSG_E_INVALID, "load first");
    if (int rc = ev->stamps.alloc((size_t)2 * ev->blocks * 4096 * 8 * 8, true)) return rc;
    // the persistent launches (trunk kernel, cooperative trunk) take their layers from the device list: layer l > 0 stamps
    // where the per-layer launch of that convolution would
    for (int l = 1; l < ev->trunkLayerCount; ++l) {
        unsigned long long* st = (unsigned long long*)ev->stamps.p + (size_t)(l - 1) * 4096 * 8;
        NSG_HIP(hipMemcpy((unsigned char*)ev->trunkLayers.p + (size_t)l * nsg::trunkLayerBytes() + nsg::trunkLayerStampsOffset(), &st,
                          sizeof(st), hipMemcpyHostToDevice));
    }
    return NSG_OK;
}
int nsg_debug_stamps_read(nsg_evaluator* ev, unsigned long long* dst) {
    if (!ev || !ev->stamps.p) return fail(NSG_E_INVALID, "stamps not enabled");
    NSG_HIP(hipDeviceSynchronize());
    NSG_HIP(hipMemcpy(dst, ev->stamps.p, ev->stamps.bytes, hipMemcpyDeviceToHost));
    return NSG_OK;
}
#endif

// (the CPU stand-in executors nsg_cpu_executor_* live in cpu_executor.cc: host-only code, built with the
// reference's release flags)

} // extern "C"
