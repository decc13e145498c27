// The per-device gate of the persistent recurrent kernels: the lane events, the ring-slot events with their CU accounting, the
// whole-device turn lock, the dense kernels' token and the cross-process lock file.  Which events a launch waits for and records is
// decided in gate_plan.h (host-only, tested on the CPU); this file holds the state and executes the decision.
#include "gate.h"
#include "gate_plan.h"

#include <fcntl.h>
#include <sys/file.h>
#include <unistd.h>

using namespace dsmi;

// Persistent kernels need every workgroup co-resident, so two of them must never share the device.
//  * Within the process: one gate per device.  wait(gate) -> launch -> record(gate) runs under the gate's mutex, so
//    two host threads with two handles / streams always chain their launches one behind the other.
//  * Across processes: the first handle of a process takes an exclusive flock on a per-device lock file (named by
//    the device's PCI bus id, so HIP_VISIBLE_DEVICES remapping does not matter); a process that cannot get it runs
//    its recurrent layers on the per-step path.  DSMI_PERSIST_SHARED=1 skips the lock (one process per GPU is
//    guaranteed by the caller).
//  * The device is four gate slots of a quarter of the CUs each (DSMI_PERSIST_LANES=1: one).  A persistent kernel whose grid
//    fits a quarter takes ONE slot (handle-affine: four batches in flight on four handles and streams run their recurrent
//    layers side by side), one that fits half takes a PAIR of slots (two batches in flight), anything else all four.
//    (kMaxLanes: rnn_plan.h, which also says which launch takes which slots)
//  * Launches that take the WHOLE device (the tile-walking kernel of H > 896, the paired-tile windows, the first generation) of
//    several handles take turns through a lock word IN DEVICE MEMORY, not through the events: an event wait orders a launch behind
//    whatever was recorded when the wait was ENQUEUED, and a forward is enqueued whole -- forward B's first recurrent layer then
//    waits for forward A's LAST one, the forwards' recurrent layers run strictly one forward after the other and B's x-projection
//    GEMMs have nothing to run beside (config 4, round 5: 40.2 ms per batch = the sum of a forward's kernels).  With the lock a
//    stream holds acquire (one wave spinning on an atomic compare-and-swap) -> the persistent launch -> release, so the turn goes to
//    whichever forward's layer is READY: A's layer l + 1 waits for its own GEMM while B's layer l runs.  Events still order the
//    whole-device launches against the slot-sized ones (two models of different widths in one process).  Two forwards in flight
//    is the count that pays: with three, every recurrent launch runs beside the dense kernels of two others and is slower for it
//    (config 4: 4.1 ms per layer against 3.85 beside one and 3.55 alone; 35.0 ms per batch against 33.7 -- also when the third
//    forward is kept out of the turns until one of the two has finished its layers: 35.3; profiles/r06_config4.txt).
// The ring kernel's windows (rnn_persist_ring.hip: H / 32 workgroups per direction, 50 CUs for cfgA) have slots of their own: as many as
// fit the device side by side, at most kRingSlots; a ring launch is ordered behind every launch of the other kernels and vice versa
// (the two families never share the device: the other kernels' grids are sized for halves and quarters of it).
// (kRingSlots: rnn_plan.h)
struct PersistGate { std::mutex mu; hipEvent_t ev[kMaxLanes] = {nullptr, nullptr, nullptr, nullptr}; hipEvent_t ring_ev[kRingSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr};
                     hipEvent_t full_ev = nullptr;      // the whole-device launch recorded last (the slot-sized launches wait for it)
                     unsigned* turn = nullptr;           // device word: 0 free, 1 a whole-device persistent launch is running
                     DeviceGateState st;                 // CUs of the window last recorded on each ring slot (gate_plan.h)
                     int lock_fd = -1; bool lock_tried = false; int next_lane = 0; };

// acquire: one wave spins until it has swapped the word from 0 to 1.  (Bounded: after a second or two it goes on regardless -- two persistent
// kernels that then share the device time out at their hand-offs and their batches are recomputed on the per-step path.)
// (Measured and not kept, profiles/r06_config4.txt: two forwards that alternate at the lock can fall into step -- both in their conv
// layers at the same time, with no recurrent launch to run beside.  Holding a forward's first acquire back until the other is half
// way through its layers keeps them apart, and the stream of batches takes the same time: 35.3 against 35.8 ms per batch over four
// runs each, inside their spread.)
__global__ void turn_acquire_kernel(unsigned* turn) {
    if (threadIdx.x != 0) return;
    unsigned spins = 0;
    while (atomicCAS(turn, 0u, 1u) != 0u && ++spins < (1u << 20)) __builtin_amdgcn_s_sleep(32);
}
__global__ void turn_release_kernel(unsigned* turn) {
    if (threadIdx.x == 0) __hip_atomic_store(turn, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// ONE forward at a time runs a dense kernel (the conv stack, an x-projection GEMM) when forwards are in flight (round 6).  Four
// lanes whose GEMMs share the chip fairly all get a quarter of what the ring windows leave, finish together and start their ring
// windows together: the lanes fall into step, and in step the chip alternates between four GEMMs crawling and four windows holding
// 200 CUs at half their MFMA rate with 56 idle.  With a token (a counter in device memory beside the turn lock: a one-wave kernel
// spins until it has taken it, a second gives it back behind the GEMM) a GEMM has everything the windows leave, is done in a
// quarter of the time, and the next lane's follows: the windows start one after the other and stay out of step.  cfgA, 64-clip
// forwards on four lanes: 5.30 -> 5.01 ms per 32-clip batch in steady state, 5.73 -> 5.45 over a 20-batch call; two forwards at
// a time 5.22, three 5.27 (profiles/r06_dense_token.txt).  On only where the caller has given the runtime a hardware queue per
// stream (GPU_MAX_HW_QUEUES >= 8 in the environment): on a shared queue a lane's give-back could stand behind
// another lane's spinning take until that gives up.  DSMI_DENSE_TOKENS=0 turns it off (A/B runs).
__global__ void dense_enter_kernel(unsigned* sem, unsigned limit) {
    if (threadIdx.x != 0) return;
    for (unsigned spins = 0; spins < (1u << 18); ++spins) {
        const unsigned c = __hip_atomic_load(sem, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c < limit && atomicCAS(sem, c, c + 1u) == c) return;
        __builtin_amdgcn_s_sleep(8);
    }
    atomicAdd(sem, 1u);      // (gave up waiting: goes on; counted, so that its give-back does not free somebody else's place)
}
__global__ void dense_leave_kernel(unsigned* sem) {
    if (threadIdx.x == 0) atomicSub(sem, 1u);
}
static int dense_tokens() {
    static const int k = [] {
        const char* e = std::getenv("DSMI_DENSE_TOKENS");
        if (e) return std::atoi(e);
        const char* q = std::getenv("GPU_MAX_HW_QUEUES");
        return q && std::atoi(q) >= 8 ? 1 : 0;
    }();
    return k;
}
int dense_token_limit() { return dense_tokens(); }
// (experiments: what runs behind the token -- 0 the conv stack as one and every GEMM, 1 the GEMMs only, 2 every conv layer by itself and every GEMM)
static int dense_scope() {
    static const int k = [] { const char* e = exp_env("DSMI_DEBUG_DENSE_SCOPE"); return e ? std::atoi(e) : 0; }();
    return k;
}

static PersistGate* persist_gate(int device) {
    static std::mutex mu;
    static std::map<int, PersistGate*> gates;
    std::lock_guard<std::mutex> lk(mu);
    auto it = gates.find(device);
    if (it != gates.end()) return it->second;
    PersistGate* g = new PersistGate();
    for (int i = 0; i < kMaxLanes; ++i)
        if (hipEventCreateWithFlags(&g->ev[i], hipEventDisableTiming) != hipSuccess) g->ev[i] = nullptr;
    for (int i = 0; i < kRingSlots; ++i)
        if (hipEventCreateWithFlags(&g->ring_ev[i], hipEventDisableTiming) != hipSuccess) g->ring_ev[i] = nullptr;
    if (hipEventCreateWithFlags(&g->full_ev, hipEventDisableTiming) != hipSuccess) g->full_ev = nullptr;
    // (without the word, or with DSMI_PERSIST_TURNS=events, the whole-device launches chain through the events as before: A/B runs)
    const char* turns = std::getenv("DSMI_PERSIST_TURNS");
    if (!(turns && std::string(turns) == "events") && g->full_ev) {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (hipSetDevice(device) != hipSuccess || hipMalloc((void**)&g->turn, 2 * sizeof(unsigned)) != hipSuccess ||          // [1]: the dense kernels' token
            hipMemset(g->turn, 0, 2 * sizeof(unsigned)) != hipSuccess) g->turn = nullptr;
        if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
    }
    gates[device] = g;
    return g;
}

static unsigned* dense_sem(int device) {
    PersistGate* g = persist_gate(device);
    return g->turn ? g->turn + 1 : nullptr;
}

// true when this process may run persistent kernels on `device`
bool persist_process_lock(int device) {
    const char* shared = std::getenv("DSMI_PERSIST_SHARED");
    if (shared && shared[0] == '1') return true;
    PersistGate* g = persist_gate(device);
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->lock_tried) return g->lock_fd >= 0 || g->lock_fd == -2;
    g->lock_tried = true;
    char bus[64] = "unknown";
    (void)hipDeviceGetPCIBusId(bus, sizeof(bus), device);
    for (char* c = bus; *c; ++c) if (*c == ':' || *c == '.' || *c == '/') *c = '_';
    const char* tmp = std::getenv("TMPDIR");
    const std::string path = std::string(tmp && tmp[0] ? tmp : "/tmp") + "/dsmi-persist-" + bus + ".lock";
    const int fd = open(path.c_str(), O_CREAT | O_RDWR, 0666);
    if (fd < 0) { g->lock_fd = -2; return true; }          // no lock directory: nothing to arbitrate with
    if (flock(fd, LOCK_EX | LOCK_NB) != 0) { close(fd); g->lock_fd = -1; return false; }
    g->lock_fd = fd;                                        // held until the process exits
    return true;
}

int persist_next_lane(int device) {
    PersistGate* g = persist_gate(device);
    std::lock_guard<std::mutex> lk(g->mu);
    return g->next_lane++;
}

// Under the gate's mutex: make the stream wait for the events gate_plan_wait names (the lock's acquire behind them) ...
void GateTurn::wait(int device, hipStream_t s, const RnnLaunch& L, int n_cus) {
    if (!g_) g_ = persist_gate(device);
    lk_ = std::unique_lock<std::mutex>(g_->mu);
    s_ = s; l_ = L;
    const DeviceGateWait w = gate_plan_wait(g_->st, L, n_cus, g_->turn != nullptr);
    for (int i = 0; i < kMaxLanes; ++i)
        if ((w.lanes >> i & 1) && g_->ev[i]) (void)hipStreamWaitEvent(s, g_->ev[i], 0);
    for (int i = 0; i < kRingSlots; ++i)
        if ((w.ring >> i & 1) && g_->ring_ev[i]) (void)hipStreamWaitEvent(s, g_->ring_ev[i], 0);
    if (w.full && g_->full_ev) (void)hipStreamWaitEvent(s, g_->full_ev, 0);
    if (w.acquire) hipLaunchKernelGGL(turn_acquire_kernel, dim3(1), dim3(64), 0, s, g_->turn);
}
// ... and publish the launch on the ones gate_plan_record names.
void GateTurn::record() {
    const DeviceGateRecord r = gate_plan_record(g_->st, l_, g_->turn != nullptr);
    if (r.release) hipLaunchKernelGGL(turn_release_kernel, dim3(1), dim3(64), 0, s_, g_->turn);
    for (int i = 0; i < kMaxLanes; ++i)
        if ((r.lanes >> i & 1) && g_->ev[i]) (void)hipEventRecord(g_->ev[i], s_);
    for (int i = 0; i < kRingSlots; ++i)
        if ((r.ring >> i & 1) && g_->ring_ev[i]) (void)hipEventRecord(g_->ring_ev[i], s_);
    if (r.full && g_->full_ev) (void)hipEventRecord(g_->full_ev, s_);
    g_->st = r.after;
    lk_.unlock();
}
void GateTurn::hold(int device) {
    if (!g_) g_ = persist_gate(device);
    lk_ = std::unique_lock<std::mutex>(g_->mu);
}

DenseHold::DenseHold(int device, int inflight, DenseScope scope, hipStream_t s) : s_(s) {
    const bool behind_token = scope == DENSE_GEMM || dense_scope() == (scope == DENSE_CONV_STACK ? 0 : 2);
    if (dense_tokens() > 0 && inflight >= 2 && behind_token) sem_ = dense_sem(device);
    if (sem_) hipLaunchKernelGGL(dense_enter_kernel, dim3(1), dim3(64), 0, s_, sem_, (unsigned)dense_tokens());
}
void DenseHold::leave() {
    if (sem_) hipLaunchKernelGGL(dense_leave_kernel, dim3(1), dim3(64), 0, s_, sem_);
}
