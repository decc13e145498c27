// Which kernel runs a recurrent layer, on which windows, tiles, tile pairs and gate slots: THE statement of that choice, as a pure
// function of the shape, the batch, what the caller said (dsmi_model_set_inflight / _set_ring_windows) and the DSMI_RNN_* switches.
// Host-only and without a HIP include, like host_logic.h: api.hip plans a layer here and then launches the plan; `make asan` builds
// the same header for the CPU (tools/asan/host_fuzz.cpp rnnplan, tests/test_rnn_plan_host.py: tests/rnn_plan_table.json row by row).
// The kernel files take their tile sizes, wave counts, LDS formulas and the table of their instantiations (rnn_*_form) from here, so
// a predicate and its launcher cannot disagree.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../include/dsmi.h"

namespace dsmi {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

struct RnnGeom {
    int kind;      // DSMI_RNN_*
    int G;         // gates per unit: 3 / 4 / 1
    int H;
    int U;         // hidden units per workgroup (8: its h granules are whole 16-byte groups of the packed state)
    int nwg;       // ceil(H / U) workgroups per direction
    int Kp;        // H rounded up to 8
    int nq;        // Kp / 8 k-blocks
    int D;         // directions
    int Np;        // D * nwg * G * U : permuted + padded gate columns of the x-projection
};
inline int rnn_gates(int kind) { return kind == DSMI_RNN_GRU ? 3 : (kind == DSMI_RNN_LSTM ? 4 : 1); }
inline RnnGeom make_rnn_geom_u(int kind, int H, int D, int U) {
    RnnGeom g;
    g.kind = kind;
    g.G = rnn_gates(kind);
    g.H = H;
    g.U = U;
    g.nwg = ceil_div(H, U);
    g.Kp = round_up(H, 8);
    g.nq = g.Kp / 8;
    g.D = D;
    g.Np = D * g.nwg * g.G * U;
    return g;
}
inline RnnGeom make_rnn_geom(int kind, int H, int D) { return make_rnn_geom_u(kind, H, D, 8); }

// ---- what the shape predicates share with the kernel files ------------------------------------------------------------------
constexpr int kCuLdsBytes = 160 * 1024;
// rnn_persist.hip (first generation)
constexpr int kPersistUnits = 8;        // hidden units per workgroup (rnn geometry U)
constexpr int kPersistWaves = 8;        // waves per workgroup
constexpr int kPersistMaxTiles = 8;     // 32-clip batch tiles per launch (B <= 256)
// rnn_persist16.hip, rnn_persist_duo.hip, rnn_persist_ring.hip, rnn_persist_ring4.hip: the 16-unit geometry
constexpr int kTileUnits = 16;          // hidden units per workgroup (ring kernels: per 16-unit group, two groups per workgroup)
constexpr int kTileClips = 16;          // clips per batch tile
constexpr int kPersist16Waves = 8;      // waves per workgroup (K-split) of the full-CU variants
constexpr int kPersist16MaxTiles = 8;   // batch tiles one workgroup can walk
constexpr int kRingThreads = 512;       // eight-wave ring: two halves of four waves
constexpr int kRingRedPitch = 20;       // row pitch (words) of its reduce buffers
constexpr int kRingMaxTiles = 4;        // its schedule length in tiles = tiles a window walks at most
constexpr int kRing4MaxTiles = 8;       // four-wave ring: tiles a window walks at most (more than four: experiments build)

// ---- which template instantiation runs a shape: THE table, read by the predicates below and by the launchers ----------------
// The predicates ask whether a shape has an instantiation; the launchers (rnn_launch.h: one `case` per instantiation) switch on the
// same answer.  tools/asan/host_fuzz.cpp rnnforms prints the table; tests/rnn_form_table.json holds it as the launchers' own
// if-ladders gave it before these functions existed.  `stamps`: the diagnostics build of a kernel (a launch with a dbg buffer).
// The experiments build's instantiations with parts removed are not here: their launchers pick them behind DSMI_EXPERIMENTS.
struct RnnForm {
    int n = 0;             // the kernel's width argument (NPW / NKW); 0: no instantiation runs this shape
    bool alt = false;      // persist8: MULTI, every workgroup walks several tiles; p16w8: the pipelined kernel; duo: TAIL
};
// v rounded up to a member of an ascending list (0: beyond the last)
inline int round_up_to(int v, std::initializer_list<int> widths) {
    for (int w : widths) if (v <= w) return w;
    return 0;
}
// rnn_persist.hip: npair pairs of 16 k over eight waves, `tiles` 32-clip tiles, carried: chains start from a carried state
inline RnnForm rnn_persist_form(int npair, int tiles, bool carried, bool stamps) {
    const int npw = ceil_div(npair, kPersistWaves);
    if (stamps) return {!carried && tiles == 1 && npw <= 7 ? 7 : 0, false};
    if (tiles > 1 && !carried) return {round_up_to(npw, {4, 7, 10}), true};
    return {round_up_to(npw, {2, 4, 7, 10}), tiles > 1};
}
// rnn_persist16.hip, whole-CU workgroups: nkb k-blocks of 32 over eight waves; the pipelined kernel where a workgroup walks more
// than two tiles (with two the next instance's producers were signalled a moment ago: nothing to overlap)
inline RnnForm rnn_persist16_form(int kind, int nkb, int tiles, bool stamps) {
    const int nkw = ceil_div(nkb, kPersist16Waves);
    if (stamps) return {nkw <= 4 ? 4 : 0, false};
    const int n = round_up_to(nkw, {2, 4, 5});
    return {n > 4 && kind == DSMI_RNN_LSTM ? 0 : n, tiles > 2};
}
// ... half-CU workgroups: four waves, at most two tiles per workgroup, no diagnostics build
inline int rnn_persist16_half_form(int kind, int nkb, int tiles, bool stamps) {
    if (stamps || tiles > 2) return 0;
    const int n = round_up_to(ceil_div(nkb, 4), {2, 4, 6, 7});
    return n > 4 && kind == DSMI_RNN_LSTM ? 0 : n;
}
// rnn_persist_duo.hip: four waves per half.  TAIL (see the kernel): every wave takes nkb / 4 whole k-blocks and the 1-3 left over
// are dealt out gate by gate, where that is at most one (block, gate) item per wave
inline RnnForm rnn_persist_duo_form(int kind, int nkb, bool stamps) {
    const bool lstm = kind == DSMI_RNN_LSTM;
    const int nkw = ceil_div(nkb, 4), kq = nkb / 4, kr = nkb % 4;
    if (stamps) return {kind == DSMI_RNN_GRU && nkw == 7 ? 7 : 0, false};
    if (kr > 0 && rnn_gates(kind) * kr <= 4 && kq >= 1 && kq <= (lstm ? 4 : 6)) return {round_up_to(kq, {2, 4, 6}), true};
    const int n = round_up_to(nkw, {2, 4, 6, 7});
    return {n > 4 && lstm ? 0 : n, false};
}
// rnn_persist_ring.hip: NKW exact (every wave of a half owns NKW or NKW - 1 k-blocks); a window of ntw tiles within its schedule
inline int rnn_persist_ring_form(int kind, int nkb, int ntw, bool stamps) {
    const int nkw = ceil_div(nkb, 4);
    if (ntw < 1 || ntw > kRingMaxTiles || nkw > (kind == DSMI_RNN_LSTM ? 4 : 7)) return 0;
    return !stamps || (kind == DSMI_RNN_GRU && nkw == 7) ? nkw : 0;
}
// rnn_persist_ring4.hip: NKW exact; more than four tiles per window run the eight-tile schedule (experiments build), which has
// eight tiles' state per thread and no registers left at 14 k-blocks
inline int rnn_persist_ring4_form(int kind, int nkb, int ntw, bool stamps) {
    const int nkw = ceil_div(nkb, 2);
    if (ntw < 1 || ntw > kRing4MaxTiles || nkw > (kind == DSMI_RNN_LSTM ? 8 : (ntw > 4 ? 13 : 14))) return 0;
    return !stamps || (kind == DSMI_RNN_GRU && nkw == 13) ? nkw : 0;
}
// Both ring kernels: a direction's output rows below 2 GiB (store offsets, see OOR).  A launcher's refusal: T is not in the plan.
inline bool rnn_ring_rows_fit(const RnnGeom& g16, int B, int T) { return (size_t)T * B * g16.Kp * 4 < (1ull << 31); }

// ---- shape predicates (pure: what some of them used to read from the environment is an argument) ---------------------------

// rnn_persist.hip: H up to 1280 (10 pairs of 16 k per wave: 80 + 80 operand VGPRs); every workgroup of a launch must own a CU, so
// a layer whose two directions do not fit together (H > 1024 on 256 CUs) runs them as two launches, one after the other.
inline bool rnn_persist_eligible(const RnnGeom& g, int B, int n_cus) {
    if (g.U != kPersistUnits || (g.H % 8) != 0) return false;
    if (!rnn_persist_form(ceil_div(g.nq, 2), ceil_div(B, 32), false, false).n) return false;
    if (ceil_div(B, 32) > kPersistMaxTiles) return false;
    return g.nwg <= n_cus;
}

// rnn_persist16.hip: H a multiple of 16, at most 4 k-blocks per wave (H <= 1024; 5 for GRU / RNN: H <= 1280), both directions of
// a tile group co-resident, no more tiles per workgroup than the carried-state arrays hold.
inline bool rnn_persist16_eligible(const RnnGeom& g16, int B, int n_cus, int* pgroups_out) {
    if (g16.U != kTileUnits || (g16.H % kTileUnits) != 0) return false;
    if (g16.nwg * g16.D > n_cus) return false;
    const int ntiles = ceil_div(B, kTileClips);
    const int pg = std::min(ntiles, n_cus / (g16.nwg * g16.D));
    if (ceil_div(ntiles, pg) > kPersist16MaxTiles) return false;
    if (!rnn_persist16_form(g16.kind, ceil_div(g16.H, 32), ceil_div(ntiles, pg), false).n) return false;
    if (pgroups_out) *pgroups_out = pg;
    return true;
}

// The half-CU (four-wave) variant: its register budget holds 6 + 1 k-blocks per wave for three gates (H <= 896), 4 for an
// LSTM (H <= 512); at most two tiles per workgroup; one workgroup slot per CU and lane.
inline bool rnn_persist16_half_eligible(const RnnGeom& g16, int B, int n_cus, int* pgroups_out) {
    if (g16.U != kTileUnits || (g16.H % kTileUnits) != 0) return false;
    if (g16.nwg * g16.D > n_cus) return false;
    const int ntiles = ceil_div(B, kTileClips);
    const int pg = std::min(ntiles, n_cus / (g16.nwg * g16.D));
    if (!rnn_persist16_half_form(g16.kind, ceil_div(g16.H, 32), ceil_div(ntiles, pg), false)) return false;
    if (pgroups_out) *pgroups_out = pg;
    return true;
}

// rnn_persist_duo.hip: tile pairs one launch can carry on n_cus CUs (0: not this shape).  At least two tiles (17+ clips), the
// half-CU register budget (GRU / RNN: H <= 896, LSTM: H <= 512), every tile pair of both directions co-resident on `n_cus` CUs
// (the caller passes one gate lane's CUs first, then the whole device).
inline int rnn_persist_duo_pairs(const RnnGeom& g16, int B, int n_cus) {
    if (g16.U != kTileUnits || (g16.H % kTileUnits) != 0) return 0;
    const int nkb = ceil_div(g16.H, 32);
    if (!rnn_persist_duo_form(g16.kind, nkb, false).n) return 0;
    // The launcher also has a TAIL instantiation for an LSTM of 17 k-blocks (H = 528, 544): past the budget above, never planned
    if (g16.kind == DSMI_RNN_LSTM && nkb > 16) return 0;
    const int ntiles = ceil_div(B, kTileClips);
    if (ntiles < 2) return 0;
    return std::min((ntiles + 1) / 2, n_cus / (g16.nwg * g16.D));
}
inline bool rnn_persist_duo_eligible(const RnnGeom& g16, int B, int n_cus) {
    return rnn_persist_duo_pairs(g16, B, n_cus) >= std::max(1, (ceil_div(B, kTileClips) + 1) / 2);
}

// rnn_persist_ring.hip: dynamic LDS of a workgroup -- ring slots, reduce buffers, cell tiles, x-projection zone, tile table, sync, stamps
inline size_t ring_lds_bytes(int kind, int nkb) {
    const int NG = rnn_gates(kind);
    return (size_t)2 * nkb * 2048 + (size_t)2 * 4 * NG * 16 * kRingRedPitch * 4 +
           (size_t)kRingMaxTiles * kRingThreads * 4 * (kind == DSMI_RNN_LSTM ? 2 : 1) + (size_t)2 * NG * 256 * 4 + kRingMaxTiles * 16 * 4 +
           32 * 4 + 8 * 16 * 8;
}
// Tiles one launch of the ring kernel can walk for this shape on `n_cus` CUs (0: not this shape): the 16-unit geometry,
// W_hh of a half in its four waves' registers (GRU / RNN: H <= 896, LSTM: H <= 512), ring + reduce buffers within the CU's LDS,
// both directions co-resident.
inline int rnn_persist_ring_tiles(const RnnGeom& g16, int B, int n_cus) {
    if (g16.U != kTileUnits || (g16.H % kTileUnits) != 0) return 0;
    const int nkb = ceil_div(g16.H, 32);
    if (!rnn_persist_ring_form(g16.kind, nkb, 1, false)) return 0;
    if (ring_lds_bytes(g16.kind, nkb) > (size_t)kCuLdsBytes) return 0;
    if (((g16.nwg + 1) / 2) * g16.D > n_cus) return 0;
    if ((size_t)g16.D * ceil_div(B, kTileClips) * nkb * 2048 * 2 >= (1ull << 31)) return 0;      // packed state below 2 GiB (store offsets, see OOR)
    return std::min(ceil_div(B, kTileClips), kRingMaxTiles);
}
// CUs one window of either ring kernel occupies
inline int rnn_persist_ring_cus(const RnnGeom& g16) { return ((g16.nwg + 1) / 2) * g16.D; }

// rnn_persist_ring4.hip: dynamic LDS of a workgroup -- ring slots, reduce buffers, x-projection zones, sync, stamps
inline size_t ring4_lds_bytes(int kind, int nkb) {
    const int NG = rnn_gates(kind);
    return (size_t)2 * nkb * 2048 + (size_t)2 * 2 * 2 * NG * 256 * 4 + (size_t)3 * 2 * NG * 256 * 4 + 32 * 4 + 4 * 8 * 8;
}
// Tiles one launch of the four-wave kernel can walk for this shape on `n_cus` CUs (0: not this shape): the 16-unit geometry, W_hh
// of a group's K half in one wave's registers (GRU / RNN: H <= 896, LSTM: H <= 512), ring + reduce buffers within the CU's LDS,
// both directions co-resident.
//   small_shapes: also fewer than four k-blocks per wave (H < 224).  NOT this kernel otherwise: round 6 found that in a pipeline
//     -- several windows of different handles running at once -- a GRU of 64..192 units comes out with the LAST tile of a window
//     wrong now and then (tools/exp/debug_short_forms.py: garbage transcripts for the clips of tile 3, nondeterministic, from the
//     third call of a process on; never alone on the chip, never with the eight-wave form, never from 256 units up in any test or
//     bench run).  The cause has not been found; the shapes are fenced off
//     (tests/test_gpu_recognizer.py::test_small_models_in_the_pipeline).  The eight-wave form takes them.  DSMI_RNN_KERNEL=ring4
//     (tests of the form alone on the chip) still reaches them: api.hip passes it here.
//   most: tiles per window at most: four (a 64-clip forward); DSMI_RING_TILES=6|8 in the experiments build lets a window walk more
//     (a chain's hand-off then lies under five or seven other phases instead of three)
inline int rnn_persist_ring4_tiles(const RnnGeom& g16, int B, int n_cus, bool small_shapes, int most = 4) {
    if (g16.U != kTileUnits || (g16.H % kTileUnits) != 0) return 0;
    const int nkb = ceil_div(g16.H, 32);
    const int nkw = rnn_persist_ring4_form(g16.kind, nkb, 1, false);
    if (!nkw || (nkw < 4 && !small_shapes)) return 0;
    if (ring4_lds_bytes(g16.kind, nkb) > (size_t)kCuLdsBytes) return 0;
    if (((g16.nwg + 1) / 2) * g16.D > n_cus) return 0;
    if ((size_t)g16.D * ceil_div(B, kTileClips) * nkb * 2048 * 2 >= (1ull << 31)) return 0;      // packed state below 2 GiB (store offsets, see OOR)
    if (most < 4 || most > kRing4MaxTiles) most = 4;
    return std::min(ceil_div(B, kTileClips), rnn_persist_ring4_form(g16.kind, nkb, most, false) ? most : 4);
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------

// The per-device gate (gate.hip, PersistGate; what a launch waits for there: gate_plan.h): four lane slots of a quarter of the CUs each for the kernels sized by halves and
// quarters of the device, and up to five slots of their own for the ring kernels' windows.
constexpr int kMaxLanes = 4;
constexpr int kRingSlots = 5;

enum RnnKernel {
    RNN_STEPS,        // rnn_step.hip: one launch per time step
    RNN_PERSIST8,     // rnn_persist.hip: the first-generation persistent kernel
    RNN_PERSIST16,    // rnn_persist16.hip, whole-CU workgroups (8 waves)
    RNN_PERSIST16_HALF,   // ... half-CU workgroups (4 waves): two batches in flight share every CU
    RNN_DUO,          // rnn_persist_duo.hip: paired tiles
    RNN_RING8,        // rnn_persist_ring.hip
    RNN_RING4,        // rnn_persist_ring4.hip
};
inline bool rnn_kernel_is16(int k) { return k >= RNN_PERSIST16; }
enum RnnGate { GATE_NONE, GATE_LANES, GATE_RING };

struct RnnLaunch {
    int kernel = RNN_STEPS;
    // the window of the layer this launch carries:
    //   ring kernels: nwin windows side by side of n tiles each, from tile `at`;   duo: n tile pairs from pair `at`;
    //   16-unit kernels: n tile groups side by side (pgroups), every tile;         first generation: n directions from direction `at`
    int at = 0, n = 0, nwin = 1;
    // the gate slots it waits on and records: [slot0, slot0 + nslots) of the lane or the ring gate; cus: CUs per ring window.
    // join: under the gate turn of the launch before it (the first generation's second direction): no wait, no record between them
    int gate = GATE_NONE, slot0 = 0, nslots = 0, cus = 0;
    bool join = false;
    int ticket = 0;         // ring kernels: offset (words) of this launch's direction tickets behind the hand-off counters
    double part = 1.0;      // its share of the layer's FLOPs and bytes
};

// One launch as text, "kernel at n nwin gate slot0 nslots cus ticket part;" (gate "held": under the previous launch's turn): what
// host_fuzz rnnplan prints per launch behind "x16|" or "x8|", and what dsmi_debug_last_rnn_plan reports of the launches a layer made.
// Returns the characters written (snprintf's count: at least `cap` when the buffer is too small).
inline int rnn_launch_text(const RnnLaunch& l, char* buf, size_t cap) {
    static const char* const names[] = {"steps", "persist8", "p16w8", "p16w4", "duo", "ring8", "ring4"};
    return std::snprintf(buf, cap, "%s %d %d %d %s %d %d %d %d %.17g;", names[l.kernel], l.at, l.n, l.nwin,
                         l.join ? "held" : (l.gate == GATE_RING ? "ring" : (l.gate == GATE_LANES ? "lane" : "none")), l.slot0, l.nslots, l.cus, l.ticket, l.part);
}

struct RnnPlanInput {
    RnnGeom geom{}, geom16{};
    bool have16 = false;        // the 16-unit weights were packed (H % 16 == 0)
    bool split16 = false;       // the x-projection GEMM runs split-fp16 and has the packed 16-unit weights
    int B = 1, n_cus = 0;
    int inflight = 1, ring_windows = 0, lane = 0;      // dsmi_model_set_inflight, _set_ring_windows; the handle's home slot
    int rnn_mode = 1, persist_gen = 2;                 // DSMI_RNN_MODE: steps -> rnn_mode 0, persist8 -> persist_gen 1
    int rnn_kernel = 0;                                // DSMI_RNN_KERNEL: 1 duo (never the ring kernels), 2 ring (also a lone batch <= 32 clips)
    bool ring8 = false, ring4 = false;                 // DSMI_RNN_KERNEL=ring8 / ring4: that form on every window
    bool ring4_small_shapes = false;                   // rnn_persist_ring4_tiles(small_shapes)
    int ring4_most = 4;                                // rnn_persist_ring4_tiles(most)        (experiments build: DSMI_RING_TILES)
    int ring_slot_cap = 0;                             // >= 2: at most so many ring slots      (experiments build: DSMI_DEBUG_RING_SLOTS)
};

// The launches of a layer in launch order: ceil(tiles / tiles per launch) of them, at most 4 up to 256 clips.  Held in place, so that
// planning a layer allocates nothing; a batch beyond that (the ABI sets no bound on B) spills into the vector.
struct RnnLaunchList {
    static constexpr int kInPlace = 8;
    RnnLaunch first[kInPlace];
    std::vector<RnnLaunch> more;
    int n = 0;
    void push_back(const RnnLaunch& l) { if (n < kInPlace) first[n] = l; else more.push_back(l); ++n; }
    const RnnLaunch& operator[](int i) const { return i < kInPlace ? first[i] : more[(size_t)(i - kInPlace)]; }
    int size() const { return n; }
};

struct RnnPlan {
    bool x16 = false;          // the x-projection is produced in the 16-unit column order
    RnnLaunchList launches;
};

// slots a lane-gate launch of `width` (1, 2 or kMaxLanes) takes for a handle whose home slot is `lane`: [first, first + width)
inline int gate_first(int lane, int width) { return width >= kMaxLanes ? 0 : (width == 2 ? 2 * (lane & 1) : (lane % kMaxLanes)); }

// The ring kernels (rnn_persist_ring.hip, rnn_persist_ring4.hip): a window = every tile of up to 4 on H / 32 workgroups per
// direction (cfgA: 50 CUs, ONE ring slot).  With batches in flight a handle's layer is one window on its own slot -- the other
// slots and the rest of the chip belong to the other batches; a lone batch of more than 32 clips spreads its tiles over as many
// windows side by side as the device holds.  (A lone batch of up to 32 clips keeps the whole-device kernel: the shortest step.)
// false: not the ring kernels for this input.
inline bool plan_ring(const RnnPlanInput& in, RnnPlan& plan) {
    if (in.rnn_kernel == 1 || !(in.inflight >= 2 || in.B > 32 || in.rnn_kernel == 2)) return false;
    const int rcus = rnn_persist_ring_cus(in.geom16);
    int ring_slots = rcus > 0 ? std::min(kRingSlots, in.n_cus / rcus) : 0;        // windows the device holds side by side
    if (in.ring_slot_cap >= 2 && ring_slots > in.ring_slot_cap) ring_slots = in.ring_slot_cap;
    const int cap8 = rnn_persist_ring_tiles(in.geom16, in.B, rcus);
    const int cap4 = in.ring8 ? 0 : rnn_persist_ring4_tiles(in.geom16, in.B, rcus, in.ring4_small_shapes, in.ring4_most);
    const bool only8 = cap4 == 0;       // the eight-wave form on every window: asked for, or a shape the four-wave form does not take
    const int cap = ring_slots >= 2 ? (only8 ? cap8 : cap4) : 0;
    if (cap <= 0) return false;
    const int ntiles = ceil_div(in.B, kTileClips);
    // windows side by side: one with batches in flight, up to four for a lone batch -- or what the caller said
    // (dsmi_model_set_ring_windows: two where only two forwards will share the chip)
    const int slots = in.ring_windows > 0 ? std::min(std::min(in.ring_windows, ring_slots), kMaxLanes)
                                          : (in.inflight >= 2 ? 1 : std::min(ring_slots, kMaxLanes));
    int ntw = std::min(std::max(ceil_div(ntiles, slots), 1), cap);
    if (in.inflight < 2 && in.ring_windows <= 0) ntw = std::max(ntw, std::min(ntiles, 2));
    const int nwin = std::min(ceil_div(ntiles, ntw), slots);
    for (int t0 = 0; t0 < ntiles; t0 += ntw * nwin) {
        RnnLaunch l;
        const int nw = std::min(nwin, ceil_div(ntiles - t0, ntw));
        // Which form.  Four waves (one per SIMD, the cell in the MFMAs' shadows) where a window walks three tiles or more: 6.4
        // against 7.2 us per step of four tiles (cfgA, alone on the chip).  The four-wave form multiplies phantom tiles like real
        // ones (its phase has no branch), the eight-wave form skips them: a window of one or two tiles -- a lone 32-clip batch at
        // the end of a stream -- is 4.3 / 5.4 us per step there against 5.8 / 6.0 (round 5, tools/exp/ring_layer_time.py).
        // DSMI_RNN_KERNEL=ring8 / ring4: one form everywhere (A/B runs, the forms' own tests).
        const bool eight = only8 || (!in.ring4 && std::min(ntw, ntiles - t0) <= 2 && cap8 > 0);
        l.kernel = eight ? RNN_RING8 : RNN_RING4;
        l.at = t0; l.nwin = nw;
        l.n = eight ? std::min(ntw, cap8) : ntw;      // (the eight-wave form's own cap: at most two real tiles are left)
        // a handle's own slot; a PAIR of windows with batches in flight: the handle's own pair of slots (consecutive forwards run
        // on consecutive handles: their pairs differ); a lone batch's windows: from slot 0
        l.gate = GATE_RING; l.nslots = nw; l.cus = rcus;
        l.slot0 = nw == 1 ? in.lane % ring_slots : ((nw == 2 && in.inflight >= 2 && ring_slots >= 4) ? 2 * (in.lane & 1) : 0);
        l.ticket = 2 * (t0 / ntw);
        l.part = (double)std::min(ntw * nw, ntiles - t0) / ntiles;
        plan.launches.push_back(l);
    }
    return true;
}

// The 16-unit kernels.  The caller says how many batches it keeps in flight (dsmi_model_set_inflight):
//   1 -> whole-CU workgroups on the whole device: the shortest step for a lone batch (2.7 us for cfgA at B = 32);
//   2 -> the ring kernels (plan_ring); where they do not run, the paired-tile pipeline on ONE gate lane's CUs when the batch fits
//        there (B = 17..32 for cfgA: 100 CUs), so that the second batch's recurrent layer runs on the other half of the chip;
//        failing that, half-CU workgroups (one lane, the two batches share every CU); failing that, whole-CU workgroups (both
//        lanes: the two batches take turns).
// false: none of them takes this shape.
inline bool plan_16(const RnnPlanInput& in, RnnPlan& plan) {
    if (plan_ring(in, plan)) return true;
    const RnnGeom& g16 = in.geom16;
    const int total_pairs = (ceil_div(in.B, kTileClips) + 1) / 2;
    const bool duo_lane = in.inflight >= 2 && rnn_persist_duo_eligible(g16, in.B, in.n_cus / 2);
    // Batches of more than one tile pair (B > 32): the paired-tile kernel in WINDOWS of as many tile pairs as the device holds,
    // one launch after the other (batches in flight take turns): 3.8 us per step and window against 2.3-2.9 us per 32 clips for
    // the kernel that walks the tiles.  (One pair per launch on the handle's own lane, the other batch's windows beside it, was
    // measured and is worse -- config 5: 169 against 128 ms per batch: four times as many persistent launches, each of which
    // waits for whole free CUs behind the other batch's small dense workgroups.)
    int window = 0;
    if (duo_lane || (in.inflight >= 2 && in.B <= 32 && rnn_persist_duo_eligible(g16, in.B, in.n_cus))) window = total_pairs;
    else if (in.B > 32) window = rnn_persist_duo_pairs(g16, in.B, in.n_cus);
    // a half-CU / half-chip kernel takes one lane (a pair of gate slots), anything else the device
    for (int p0 = 0; window >= 1 && p0 < total_pairs; p0 += window) {
        RnnLaunch l;
        l.kernel = RNN_DUO; l.at = p0; l.n = std::min(window, total_pairs - p0);
        l.gate = GATE_LANES; l.nslots = duo_lane ? 2 : kMaxLanes; l.slot0 = gate_first(in.lane, l.nslots);
        l.part = (double)l.n / total_pairs;
        plan.launches.push_back(l);
    }
    if (window >= 1) return true;
    RnnLaunch l;
    l.gate = GATE_LANES;
    if (in.inflight >= 2 && rnn_persist16_half_eligible(g16, in.B, in.n_cus, &l.n)) { l.kernel = RNN_PERSIST16_HALF; l.nslots = 2; }
    else if (rnn_persist16_eligible(g16, in.B, in.n_cus, &l.n)) { l.kernel = RNN_PERSIST16; l.nslots = kMaxLanes; }
    else return false;
    l.slot0 = gate_first(in.lane, l.nslots);
    plan.launches.push_back(l);
    return true;
}

// One recurrent layer.  With have16 = false it is the plan that follows a 16-unit launcher's refusal (first generation if
// eligible, else per step); with rnn_mode = 0 the one that follows the first generation's.
inline RnnPlan plan_rnn_layer(const RnnPlanInput& in) {
    RnnPlan plan;
    if (in.rnn_mode == 1 && in.persist_gen == 2 && in.split16 && in.have16 && plan_16(in, plan)) {
        plan.x16 = true;
        return plan;
    }
    RnnLaunch l;
    if (in.rnn_mode == 1 && rnn_persist_eligible(in.geom, in.B, in.n_cus)) {
        // whole layer in one launch, sized for the whole device; a layer too wide for both directions at once runs them one after
        // the other under one turn of the gate
        const int ny = in.geom.nwg * in.geom.D <= in.n_cus ? in.geom.D : 1;
        l.kernel = RNN_PERSIST8; l.n = ny; l.part = (double)ny / in.geom.D;
        l.gate = GATE_LANES; l.slot0 = 0; l.nslots = kMaxLanes;
        for (l.at = 0; l.at < in.geom.D; l.at += ny) {
            plan.launches.push_back(l);
            l.join = true;
        }
        return plan;
    }
    plan.launches.push_back(l);      // RNN_STEPS
    return plan;
}

}  // namespace dsmi
