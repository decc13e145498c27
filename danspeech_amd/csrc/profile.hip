// Profiling and diagnostics of dsmi_model (include/dsmi.h): the per-kernel dispatch timer, the stage times, the last layer's plan
// as text and the per-wave stamp entry points.  Host code only.
#include "common.h"
#include "model.h"
#include "gate.h"

#include <algorithm>
#include <cstring>

using namespace dsmi;

// Count one launch of `kind`; when profiling level 2 is on and `sample` is set, hand out an
// event pair for hipExtLaunchKernelGGL.
EvPair timer_arm(dsmi_model* m, int kind, bool sample, double flops, double bytes) {
    EvPair ev;
    if (m->profiling < 2) return ev;
    KernelTimer& t = m->kt;
    t.launches[kind] += 1;
    t.flops[kind] += flops;
    t.bytes[kind] += bytes;
    if (!sample) return ev;
    // Every launch of the recurrent kernels is stamped (bench.py's roofline kernel: its mean duration is over ALL its launches of the timed
    // region); of the other kinds every FIFTH -- a stamped launch is a hipExtLaunchKernelGGL with two events, and stamping all sixteen
    // launches of every forward costs the four-lane pipeline 2 - 4 % of a 20-batch call.  Five, not four: a kind's launches per
    // forward (layer GEMM: 4 for five layers, 6 for seven, 8 for nine) share no factor with it, so the stamped launch walks through
    // the layers instead of always being the same one; bench.py weights a kind's share by launches / samples.
    // (DSMI_DEBUG_SAMPLE_EVERY: experiments)
    static const int every = [] { const char* e = exp_env("DSMI_DEBUG_SAMPLE_EVERY"); const int v = e ? std::atoi(e) : 5; return v < 1 ? 1 : v; }();
    if (kind != KK_PERSIST && kind != KK_STEP && (t.launches[kind] - 1) % every != 0) return ev;
    static const int ring_every = [] { const char* e = exp_env("DSMI_DEBUG_SAMPLE_RING_EVERY"); const int v = e ? std::atoi(e) : 1; return v < 1 ? 1 : v; }();
    if (kind == KK_PERSIST && (t.launches[kind] - 1) % ring_every != 0) return ev;
    hipEvent_t e[2];
    for (int i = 0; i < 2; ++i) {
        if (!t.free_events.empty()) { e[i] = t.free_events.back(); t.free_events.pop_back(); }
        else if (hipEventCreate(&e[i]) != hipSuccess) return EvPair();
    }
    ev.start = e[0]; ev.stop = e[1];
    t.pending[kind].push_back({e[0], e[1]});
    return ev;
}

void timer_resolve(dsmi_model* m) {
    KernelTimer& t = m->kt;
    for (int k = 0; k < KK_COUNT; ++k) {
        for (auto& pr : t.pending[k]) {
            float ms = 0.f;
            if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                t.sum_us[k] += ms * 1e3;
                t.samples[k] += 1;
            }
            t.free_events.push_back(pr.first);
            t.free_events.push_back(pr.second);
        }
        t.pending[k].clear();
    }
}

extern "C" int dsmi_debug_last_rnn_plan(const dsmi_model* m, char* buf, int64_t capacity) {
    if (!m || !buf || capacity < 1) return DSMI_ERR_INVALID;
    buf[0] = 0;
    if (m->last_plan_n == 0) return 0;
    std::string text = m->last_plan_x16 ? "x16|" : "x8|";
    for (int i = 0; i < std::min(m->last_plan_n, (int)dsmi_model::kLastPlanKept); ++i) {
        char one[160];
        rnn_launch_text(m->last_plan[i], one, sizeof one);
        text += one;
    }
    if ((int64_t)text.size() + 1 > capacity) return DSMI_ERR_INVALID;
    std::memcpy(buf, text.c_str(), text.size() + 1);
    return m->last_plan_n;
}

extern "C" int dsmi_debug_xproj(dsmi_model* m, float* xp_host, int64_t capacity, int32_t* rows, int32_t* cols, int32_t* workgroups) {
    if (!m) return DSMI_ERR_INVALID;
    const int64_t n = (int64_t)m->last_xp_rows * m->last_xp_cols;
    if (!xp_host || !rows || !cols || !workgroups || n == 0 || !m->xp || capacity < n) return fail(m, DSMI_ERR_INVALID, "dsmi_debug_xproj: no layer has run, or the buffer is too small");
    HIP_OK(m, hipSetDevice(m->device));
    HIP_OK(m, hipDeviceSynchronize());
    HIP_OK(m, hipMemcpy(xp_host, m->xp, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    *rows = m->last_xp_rows; *cols = m->last_xp_cols; *workgroups = m->last_xp_wgs;
    return DSMI_OK;
}

extern "C" int dsmi_debug_conv_workgroups(const dsmi_model* m, int32_t* workgroups, int32_t capacity) {
    if (!m || !workgroups || capacity < m->desc.conv_layers) return DSMI_ERR_INVALID;
    for (int l = 0; l < m->desc.conv_layers; ++l) workgroups[l] = m->last_conv_wgs[l];
    return m->desc.conv_layers;
}

extern "C" int dsmi_set_profiling(dsmi_model* m, int level) {
    if (!m) return DSMI_ERR_INVALID;
    m->profiling = level < 0 ? 0 : (level > 2 ? 2 : level);
    // the events of the stamped launches are made HERE, not at the launches: an event's first creation is tens of microseconds of
    // the caller's thread, and a region that is being timed would pay for a hundred of them (bench.py: 20 steps = 80 stamped launches)
    if (m->profiling == 2 && hipSetDevice(m->device) == hipSuccess)
        while (m->kt.free_events.size() < 256) {
            hipEvent_t e;
            if (hipEventCreate(&e) != hipSuccess) break;
            m->kt.free_events.push_back(e);
        }
    return DSMI_OK;
}

extern "C" int dsmi_kernel_stats(dsmi_model* m, int kind, int64_t* launches, int64_t* samples, double* avg_us,
                                 double* flops_per_launch, double* bytes_per_launch) {
    if (!m || kind < 0 || kind >= KK_COUNT) return DSMI_ERR_INVALID;
    (void)hipSetDevice(m->device);
    timer_resolve(m);
    const KernelTimer& t = m->kt;
    if (launches) *launches = t.launches[kind];
    if (samples) *samples = t.samples[kind];
    if (avg_us) *avg_us = t.samples[kind] ? t.sum_us[kind] / t.samples[kind] : 0.0;
    if (flops_per_launch) *flops_per_launch = t.launches[kind] ? t.flops[kind] / t.launches[kind] : 0.0;
    if (bytes_per_launch) *bytes_per_launch = t.launches[kind] ? t.bytes[kind] / t.launches[kind] : 0.0;
    return DSMI_OK;
}

extern "C" int dsmi_reset_kernel_stats(dsmi_model* m) {
    if (!m) return DSMI_ERR_INVALID;
    timer_resolve(m);
    for (int k = 0; k < KK_COUNT; ++k) { m->kt.sum_us[k] = 0; m->kt.samples[k] = 0; m->kt.launches[k] = 0; m->kt.flops[k] = 0; m->kt.bytes[k] = 0; }
    return DSMI_OK;
}

extern "C" double dsmi_stage_time_us(const dsmi_model* m, int stage) {
    if (!m || stage < 0 || stage > 4) return -1.0;
    return m->stage_us[stage];
}

extern "C" int dsmi_last_forward_stats(const dsmi_model* m, int64_t* n_step, double* step_flops, double* total_flops) {
    if (!m) return DSMI_ERR_INVALID;
    if (n_step) *n_step = m->n_step_launches;
    if (step_flops) *step_flops = m->step_flops;
    if (total_flops) *total_flops = m->total_flops;
    return DSMI_OK;
}

// The stamp entry points' common beginning: workspaces for (B, To); for a persistent kernel the same rules as the product path --
// one process per GPU, and the per-device gate held to the end of the call on a drained device (every launch is followed by a
// device synchronise before the lock is released); then a zeroed stamp buffer of `need` words, full-length clips and a zero
// x-projection.  The buffer is freed and the gate released when the StampRun goes out of scope, on every return path.
struct StampRun {
    GateTurn gate;
    unsigned long long* dbg = nullptr;
    ~StampRun() { if (dbg) (void)hipFree(dbg); }
};
static int stamp_begin(dsmi_model* m, int B, int To, bool persistent, int64_t need, int64_t n_words, StampRun& r) {
    int Tin = To;
    while (seq_len(m, Tin) < To) Tin += 1;
    int rc;
    if ((rc = dsmi_reserve(m, B, Tin))) return rc;
    HIP_OK(m, hipSetDevice(m->device));
    if (persistent) {
        if (!persist_process_lock(m->device)) return fail(m, DSMI_ERR_INVALID, "another process holds this GPU's persistent-kernel lock");
        r.gate.hold(m->device);      // (no other launch of this process can start)
        HIP_OK(m, hipDeviceSynchronize());
    }
    if (n_words < need) return fail(m, DSMI_ERR_INVALID, "stamp buffer too small");
    HIP_OK(m, hipMalloc((void**)&r.dbg, sizeof(unsigned long long) * need));
    HIP_OK(m, hipMemset(r.dbg, 0, sizeof(unsigned long long) * need));
    std::vector<int32_t> lens(B, To);
    HIP_OK(m, hipMemcpy(m->lens_dev, lens.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice));
    HIP_OK(m, hipMemset(m->xp, 0, sizeof(float) * (size_t)To * B * std::max(m->geom.Np, m->have16 ? m->geom16.Np : 0)));
    return DSMI_OK;
}

// ---- diagnostics: per-wave phase timestamps (s_memrealtime, 100 MHz) of ONE recurrent step launch.
// Runs steps 0..step of `layer` on whatever the workspaces hold (timing only) and returns
// stamps[D*nwg][8 waves][8] for the last one.  GRU, B <= 32.
extern "C" int dsmi_debug_step_stamps(dsmi_model* m, int layer, int B, int To, int step, uint64_t* stamps_host, int64_t n_words) {
    if (!m || !m->finalized || m->desc.rnn_type != DSMI_RNN_GRU || B > 32 || layer < 0 || layer >= m->desc.rnn_layers) return DSMI_ERR_INVALID;
    const int64_t need = (int64_t)m->geom.D * m->geom.nwg * 8 * 8;
    StampRun run;
    int rc;
    if ((rc = stamp_begin(m, B, To, false, need, n_words, run))) return rc;
    for (int dd = 0; dd < m->geom.D; ++dd) HIP_OK(m, hipMemset(m->hbuf[0][dd], 0, sizeof(float) * (size_t)To * B * m->Hs));
    RnnStepLaunch st = rnn_step_launch(m, layer, B, To, 0);
    for (int s2 = 0; s2 <= step; ++s2) {
        st.step = s2;
        st.dbg = s2 == step ? run.dbg : nullptr;
        launch_rnn_step(st, nullptr);
    }
    HIP_OK(m, hipDeviceSynchronize());
    HIP_OK(m, hipMemcpy(stamps_host, run.dbg, sizeof(unsigned long long) * need, hipMemcpyDeviceToHost));
    return DSMI_OK;
}

// ---- diagnostics: accumulated per-wave phase times (100 MHz ticks) of one persistent layer launch;
// stamps_host[workgroups][8 waves][8]: 0 loop head, 1 wait, 2 h load + MFMA, 3 LDS + barrier, 4 cell (+ publish stores),
// 5 drain + signal.  Returns the number of workgroups stamped (> 0) or a DSMI_ERR_* code (< 0).
// DSMI_STAMP_RING=1: the ring kernel (one window of every tile of B <= 64 clips; <= 128 with DSMI_RING_TILES=8): the four-wave form stamps[workgroup][4 waves][8] (Ring4Args::dbg) = phase work,
// wait for the wave's requests, poll spin, barrier ([7] phases); DSMI_RNN_KERNEL=ring8, the eight-wave form: stamps[workgroup][8 waves][16] (RingArgs::dbg) = M work, M-end waits,
// C work, barrier behind M, barrier behind C, poll spin (100 MHz ticks), shader cycles in M work, slots.
static int ring_stamps(dsmi_model* m, int layer, int B, int To, uint64_t* stamps_host, int64_t n_words);

extern "C" int dsmi_debug_persist_stamps(dsmi_model* m, int layer, int B, int To, uint64_t* stamps_host, int64_t n_words) {
    if (m && m->finalized && std::getenv("DSMI_STAMP_RING")) return ring_stamps(m, layer, B, To, stamps_host, n_words);
    if (!m || !m->finalized || B > 32 || layer < 0 || layer >= m->desc.rnn_layers || !rnn_persist_eligible(m->geom, B, m->n_cus) ||
        m->geom.nwg * m->geom.D > m->n_cus) return DSMI_ERR_INVALID;
    // which kernel: DSMI_STAMP_DUO: the paired-tile kernel, stamps[workgroup][8 waves][8] = time in slots 0..3 and at the barrier
    // behind each; else the 16-unit kernel with one tile per workgroup (the plain single-tile path is what is stamped); else the
    // first generation
    int pgroups = 0;
    const bool duo = std::getenv("DSMI_STAMP_DUO") && m->have16 && rnn_persist_duo_eligible(m->geom16, B, m->n_cus);
    const bool use16 = duo || (m->persist_gen == 2 && m->have16 && rnn_persist16_eligible(m->geom16, B, m->n_cus, &pgroups) && ceil_div(B, 16) <= pgroups);
    const int64_t need = duo ? (int64_t)m->geom16.D * ceil_div(ceil_div(B, 16), 2) * m->geom16.nwg * 8 * 8
                             : (use16 ? (int64_t)m->geom16.D * pgroups * m->geom16.nwg * 8 * 8 : (int64_t)m->geom.D * m->geom.nwg * 8 * 8);
    StampRun run;
    int rc;
    if ((rc = stamp_begin(m, B, To, true, need, n_words, run))) return rc;
    RnnPersist16Launch p16 = persist16_launch(m, layer, B, To, 0);
    p16.pgroups = pgroups;
    RnnPersistLaunch p8 = persist_launch(m, layer, B, To, 0);
    p8.d0 = 0; p8.ny = m->geom.D;
    for (int rep = 0; rep < 2; ++rep) {     // first pass warms up, second is stamped
        HIP_OK(m, hipMemset(m->pcnt, 0, sizeof(unsigned) * persist_cnt_words(m, B, To, use16, false)));
        p16.dbg = p8.dbg = rep ? run.dbg : nullptr;
        if (duo) launch_rnn_persist_duo(p16, nullptr);
        else if (use16) launch_rnn_persist16(p16, nullptr);
        else launch_rnn_persist(p8, nullptr);
        HIP_OK(m, hipDeviceSynchronize());
    }
    HIP_OK(m, hipMemcpy(stamps_host, run.dbg, sizeof(unsigned long long) * need, hipMemcpyDeviceToHost));
    return (int)(need / 64);          // number of workgroups stamped
}

static int ring_stamps(dsmi_model* m, int layer, int B, int To, uint64_t* stamps_host, int64_t n_words) {
    if (B < 1 || B > 128 || layer < 0 || layer >= m->desc.rnn_layers || !m->have16) return DSMI_ERR_INVALID;
    const int cap = m->ring8 ? rnn_persist_ring_tiles(m->geom16, B, m->n_cus)
                             : rnn_persist_ring4_tiles(m->geom16, B, m->n_cus, ring_env().small_shapes, ring_env().most);
    if (cap < ceil_div(B, 16)) return DSMI_ERR_INVALID;
    // per workgroup: the eight-wave form 8 waves x 16 words, the four-wave form 4 waves x 8 words (in the first 32 of the 128)
    const int64_t need = (int64_t)rnn_persist_ring_cus(m->geom16) * 8 * 16;
    StampRun run;
    int rc;
    if ((rc = stamp_begin(m, B, To, true, need, n_words, run))) return rc;
    RnnPersist16Launch pl = persist16_launch(m, layer, B, To, 0);
    pl.tile0 = 0; pl.ntw = ceil_div(B, 16); pl.nwin = 1;
    bool ok = true;
    for (int rep = 0; rep < 2 && ok; ++rep) {
        HIP_OK(m, hipMemset(m->pcnt, 0, sizeof(unsigned) * persist_cnt_words(m, B, To, true, false)));
        pl.dbg = rep ? run.dbg : nullptr;
        ok = m->ring8 ? launch_rnn_persist_ring(pl, nullptr) : launch_rnn_persist_ring4(pl, nullptr);
        HIP_OK(m, hipDeviceSynchronize());
    }
    HIP_OK(m, hipMemcpy(stamps_host, run.dbg, sizeof(unsigned long long) * need, hipMemcpyDeviceToHost));
    return ok ? (int)(need / 128) : DSMI_ERR_INVALID;
}
