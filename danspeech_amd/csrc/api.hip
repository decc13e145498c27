// The forward pass of libdsmi.so (include/dsmi.h): its orchestration on the handle's workspaces, the ring of forwards whose status
// has not been collected, and the stage entry points (conv stack, one recurrent layer, the head).  Host code only; kernels live in
// conv.hip / conv_split.hip / conv1_split.hip / gemm.hip / rnn_step.hip / rnn_persist*.hip / head.hip, the per-device gate in gate.hip,
// handle creation and workspaces in model_build.hip, profiling and diagnostics in profile.hip.
#include "common.h"
#include "model.h"
#include "gate.h"

#include <algorithm>
#include <cstring>

using namespace dsmi;

// ------------------------------------------------------------------------------------------
static int check_lens(dsmi_model* m, const int32_t* lens, int B, int T) {
    for (int i = 0; i < B; ++i) {
        if (lens[i] < 1 || lens[i] > T) return fail(m, DSMI_ERR_INVALID, "length outside 1..T");
        // pack_padded_sequence(enforce_sorted=True), model.py:117
        if (i && lens[i] > lens[i - 1]) return fail(m, DSMI_ERR_UNSORTED, "`lengths` array must be sorted in decreasing order");
    }
    return DSMI_OK;
}

static int check_batch(dsmi_model* m, const int32_t* lens, int B, int T) {
    if (!m->finalized) return fail(m, DSMI_ERR_NOT_READY, "dsmi_model_finalize has not been called");
    if (!lens || B < 1 || T < 1) return fail(m, DSMI_ERR_INVALID, "bad batch arguments");
    return check_lens(m, lens, B, T);
}

static int run_conv(dsmi_model* m, const float* feat, int B, int T, int To, int ys, hipStream_t s, const float** out) {
    const float* x = feat;
    const uint16_t* x_sp = nullptr;
    int ti = T, xs = T;
    const int L = m->desc.conv_layers;
    for (int l = 0; l < L; ++l) {
        const ConvSpec& sp = kConvSpecs[l];
        double fl = 0;
        for (int i = 0; i < B; ++i) fl += 2.0 * sp.co * m->conv_fo[l] * (double)m->host_out_lens[i] * sp.ci * sp.kf * sp.kt;
        const double by = 4.0 * B * ((double)sp.ci * m->conv_fi[l] * ti + (double)sp.co * m->conv_fo[l] * To);
        const bool next_split = m->conv_mode == 1 && l + 1 < L;       // the consumer is a split-fp16 conv layer
        DenseHold hold(m->device, m->inflight, DENSE_CONV_LAYER, s);
        if (x_sp) {
            ConvSplitLaunch c;
            c.x_sp = x_sp; c.wp_sp = m->conv[l].wp_sp; c.bias = m->conv[l].bias; c.bn_a = m->conv[l].bn_a; c.bn_b = m->conv[l].bn_b;
            c.out_lens_dev = m->lens_dev; c.y = next_split ? nullptr : m->conv_buf[l & 1]; c.y_sp = next_split ? m->conv_buf_sp[l] : nullptr;
            c.B = B; c.co = sp.co; c.fi = m->conv_fi[l]; c.fo = m->conv_fo[l]; c.ti = ti; c.to = To; c.ys = ys;
            c.ev = timer_arm(m, KK_CONV1 + l, true, fl, by);
            c.tile_cnt = m->conv_tiles ? m->tile_counters(dsmi_model::kTileCntConv0 + l) : nullptr; c.n_cus = m->n_cus;
            m->last_conv_wgs[l] = launch_conv_split(c, s);
            x = c.y; x_sp = c.y_sp;
        } else {
            ConvLaunch c;
            c.x = x; c.y = m->conv_buf[l & 1]; c.wp = m->conv[l].wp; c.bias = m->conv[l].bias;
            c.bn_a = m->conv[l].bn_a; c.bn_b = m->conv[l].bn_b; c.out_lens_dev = m->lens_dev;
            c.B = B; c.ci = sp.ci; c.co = sp.co; c.fi = m->conv_fi[l]; c.fo = m->conv_fo[l];
            c.ti = ti; c.to = To; c.xs = xs; c.ys = ys; c.layer = l;
            c.y_sp = next_split ? m->conv_buf_sp[l] : nullptr;
            c.ev = timer_arm(m, KK_CONV1 + l, true, fl, by);
            // layer 0 on the split-fp16 MFMA (features are z-normalised log magnitudes: far inside fp16's range)
            c.tile_cnt = m->conv_tiles ? m->tile_counters(dsmi_model::kTileCntConv0 + l) : nullptr; c.n_cus = m->n_cus;
            m->last_conv_wgs[l] = 0;      // (conv.hip, the fp32 statement: not reported)
            if (l == 0 && m->conv_mode == 1 && m->conv1_split) m->last_conv_wgs[l] = launch_conv1_split(c, m->conv[0].wp_sp, s);
            else launch_conv(c, s);
            x = c.y; x_sp = c.y_sp;
        }
        hold.leave();
        ti = To; xs = ys;
    }
    *out = x;
    return DSMI_OK;
}

// The launch descriptions of layer l's recurrent kernels on the internal buffers (output to hbuf[dst]); which window of the layer a
// launch carries is the caller's to fill in (rnn_plan.h).  The spin-limit and drop-signal test hooks of every persistent launch are
// set here and nowhere else.
RnnPersist16Launch persist16_launch(const dsmi_model* m, int l, int B, int To, int dst) {
    RnnPersist16Launch pl;
    pl.g = m->geom16;
    for (int dd = 0; dd < 2; ++dd) { pl.whh16[dd] = m->rnn[l].whh16_sp[dd]; pl.bhh[dd] = m->rnn[l].bhh[dd]; pl.out[dd] = m->hbuf[dst][dd]; }
    pl.xp = m->xp; pl.lens_dev = m->lens_dev; pl.hpack16 = m->hpack16; pl.counters = m->pcnt; pl.err = m->perr;
    pl.B = B; pl.T = To; pl.pgroups = 0;
    pl.spin_limit = m->spin_limit;
    if (m->drop_layer == l) { pl.drop_wg = m->drop_wg; pl.drop_step = m->drop_step; }
    return pl;
}
RnnPersistLaunch persist_launch(const dsmi_model* m, int l, int B, int To, int dst) {
    RnnPersistLaunch pl;
    pl.g = m->geom;
    for (int dd = 0; dd < 2; ++dd) { pl.whh_sp[dd] = m->rnn[l].whh_sp[dd]; pl.bhh[dd] = m->rnn[l].bhh[dd]; pl.out[dd] = m->hbuf[dst][dd]; }
    pl.xp = m->xp; pl.lens_dev = m->lens_dev; pl.hpack_sp = m->hpack_sp; pl.counters = m->pcnt; pl.err = m->perr; pl.B = B; pl.T = To;
    pl.spin_limit = m->spin_limit;
    if (m->drop_layer == l) { pl.drop_wg = m->drop_wg; pl.drop_step = m->drop_step; }
    return pl;
}
RnnStepLaunch rnn_step_launch(const dsmi_model* m, int l, int B, int To, int dst) {
    RnnStepLaunch st;
    st.g = m->geom;
    for (int dd = 0; dd < 2; ++dd) {
        st.whh_packed[dd] = m->rnn[l].whh[dd]; st.bhh[dd] = m->rnn[l].bhh[dd];
        st.out[dd] = m->hbuf[dst][dd]; st.cstate[dd] = m->cst[dd];
    }
    st.xp = m->xp; st.lens_dev = m->lens_dev; st.B = B; st.T = To; st.hpack = m->hpack;
    return st;
}

// What the ring kernels' predicates and plan take from the environment (rnn_plan.h keeps them pure).  DSMI_RNN_KERNEL=ring4 also
// lifts the fence around the four-wave form's small shapes (rnn_persist_ring4_tiles) -- and THAT is read once per process, here,
// not per handle like dsmi_model::ring4 (dsmi_model_create): a handle created under the variable in a process started without it
// runs the four-wave form on every window of the shapes it takes anyway, and the fenced shapes on the eight-wave form.  An oddity
// kept from when the predicate read the variable itself -- with ONE difference: the predicate read it at its first call (the first
// layer that reached the ring kernels without ring8, or the ring stamps), this is read when the first recurrent layer of any kind
// is planned.  A process whose first layers are lone batches of up to 32 clips and which only THEN sets the variable used to get the
// fence lifted and no longer does.  A process started with the variable, or one that never sets it, sees no difference.  The other
// two inputs exist in the experiments build only.
const RingEnv& ring_env() {
    static const RingEnv env = [] {
        const char *k = std::getenv("DSMI_RNN_KERNEL"), *t = exp_env("DSMI_RING_TILES"), *c = exp_env("DSMI_DEBUG_RING_SLOTS");
        return RingEnv{k && std::string(k) == "ring4", t ? std::atoi(t) : 4, c ? std::atoi(c) : 0};
    }();
    return env;
}

static RnnPlanInput rnn_plan_input(const dsmi_model* m, int B, bool split16) {
    RnnPlanInput in;
    in.geom = m->geom; in.geom16 = m->geom16; in.have16 = m->have16; in.split16 = split16;
    in.B = B; in.n_cus = m->n_cus; in.inflight = m->inflight; in.ring_windows = m->ring_windows; in.lane = m->lane;
    in.rnn_mode = m->rnn_mode; in.persist_gen = m->persist_gen; in.rnn_kernel = m->rnn_kernel; in.ring8 = m->ring8; in.ring4 = m->ring4;
    in.ring4_small_shapes = ring_env().small_shapes; in.ring4_most = ring_env().most; in.ring_slot_cap = ring_env().slot_cap;
    return in;
}

// Launch a layer's plan on the internal buffers.  Per launch: arm the timer, take the gate slots, launch, record -- wait -> launch
// -> record is one GateTurn, atomic against other host threads (two persistent kernels must never share CUs: see gate.hip).
// false: a launcher refused its shape and the layer has not run.
static bool run_rnn_plan(dsmi_model* m, const RnnPlan& plan, int l, int B, int To, int dst, double sumlen, hipStream_t s) {
    const double H = m->desc.rnn_hidden_size, GH = (double)m->geom.G * m->desc.rnn_hidden_size, Dd = m->geom.D;
    if (plan.launches[0].kernel == RNN_STEPS) {
        RnnStepLaunch st = rnn_step_launch(m, l, B, To, dst);
        for (int step = 0; step < To; ++step) {
            st.step = step;
            // algorithmic FLOPs of this launch: clips still running at this step (both directions)
            int act = 0;
            for (int i = 0; i < B; ++i) act += step < m->host_out_lens[i] ? 1 : 0;
            st.ev = timer_arm(m, KK_STEP, (step & 7) == 3, 2.0 * Dd * GH * H * act, 4.0 * Dd * (GH * H + (double)B * (GH + 2.0 * H)));
            launch_rnn_step(st, s);
        }
        m->last_plan_x16 = false; m->last_plan_n = 1; m->last_plan[0] = plan.launches[0];
        return true;
    }
    RnnPersist16Launch p16;      // a plan's launches are of one family: the 16-unit kernels or the first generation
    RnnPersistLaunch p8;
    if (plan.x16) p16 = persist16_launch(m, l, B, To, dst);
    else p8 = persist_launch(m, l, B, To, dst);
    // counters are single-use per step, zeroed right before (the 16-unit kernels': with the ring kernels' direction tickets behind
    // them, two words per window)
    const size_t cnt_words = persist_cnt_words(m, B, To, true, false);
    (void)hipMemsetAsync(m->pcnt, 0, sizeof(unsigned) * persist_cnt_words(m, B, To, plan.x16, true), s);
    // the four-wave ring kernel's directions by XCD half (its prologue; profiles/r06_ring_experiments.txt: 2.29 -> 1.56 GB fetched per
    // launch); DSMI_DEBUG_RING_XCD=0 in the experiments build: by blockIdx
    static const bool ring_xcd = [] { const char* e = exp_env("DSMI_DEBUG_RING_XCD"); return !(e && e[0] == '0'); }();
    GateTurn turn;
    bool ok = true;
    for (int i = 0; i < plan.launches.size() && ok; ++i) {
        const RnnLaunch& L = plan.launches[i];
        const EvPair ev = timer_arm(m, KK_PERSIST, true, L.part * 2.0 * Dd * GH * H * sumlen, L.part * 4.0 * Dd * (GH * H + (double)To * B * (GH + 2.0 * H)));
        if (!L.join) turn.wait(m->device, s, L, m->n_cus);
        p16.ev = ev;
        switch (L.kernel) {
            case RNN_PERSIST8: p8.ev = ev; p8.d0 = L.at; p8.ny = L.n; ok = launch_rnn_persist(p8, s); break;
            case RNN_PERSIST16: p16.pgroups = L.n; p16.waves = 8; ok = launch_rnn_persist16(p16, s); break;
            case RNN_PERSIST16_HALF: p16.pgroups = L.n; p16.waves = 4; ok = launch_rnn_persist16(p16, s); break;
            case RNN_DUO: p16.pair0 = L.at; p16.npairs = L.n; ok = launch_rnn_persist_duo(p16, s); break;
            default:
                p16.tile0 = L.at; p16.ntw = L.n; p16.nwin = L.nwin;
                p16.tickets = ring_xcd ? m->pcnt + cnt_words + L.ticket : nullptr;
                ok = L.kernel == RNN_RING8 ? launch_rnn_persist_ring(p16, s) : launch_rnn_persist_ring4(p16, s);
        }
        if (!ok || i + 1 == plan.launches.size() || !plan.launches[i + 1].join) turn.record();
    }
    if (ok) {      // what dsmi_debug_last_rnn_plan reports: only a plan that ran whole
        m->last_plan_x16 = plan.x16; m->last_plan_n = plan.launches.size();
        for (int i = 0; i < std::min(m->last_plan_n, (int)dsmi_model::kLastPlanKept); ++i) m->last_plan[i] = plan.launches[i];
    }
    return ok;
}

// One BatchRNN layer on the internal buffers: plan it (rnn_plan.h), x-projection GEMM in the column order the plan's kernels read,
// launch the plan.
static void run_rnn_layer(dsmi_model* m, int l, GemmLaunch gl, int B, int To, int dst, hipStream_t s) {
    double sumlen = 0;
    for (int i = 0; i < B; ++i) sumlen += m->host_out_lens[i];
    const double GH = (double)m->geom.G * m->desc.rnn_hidden_size, Dd = m->geom.D;
    RnnPlanInput in = rnn_plan_input(m, B, m->gemm_mode == 1 && gl.w_sp);
    RnnPlan plan = plan_rnn_layer(in);
    if (plan.x16) {      // the second-generation kernels read the x-projection in their own column order
        gl.w_sp = m->rnn[l].wih16_sp; gl.bias = m->rnn[l].bih16; gl.N = m->geom16.Np; gl.ldc = m->geom16.Np;
    }
    gl.ev = timer_arm(m, gl.mode == GEMM_A_CONV ? KK_GEMM0 : KK_GEMM, true, 2.0 * Dd * GH * gl.K * sumlen,
                      4.0 * ((double)gl.M * gl.K * (gl.a2 ? 2 : 1) + (double)gl.N * gl.K + (double)gl.M * gl.N));
    DenseHold hold(m->device, m->inflight, DENSE_GEMM, s);      // one forward's dense kernel at a time
    m->last_xp_wgs = launch_gemm(gl, s);
    m->last_xp_rows = gl.M; m->last_xp_cols = gl.ldc;
    hold.leave();
    if (run_rnn_plan(m, plan, l, B, To, dst, sumlen, s)) return;
    // The predicates and the launchers read one table of instantiations (rnn_plan.h: rnn_*_form), so what a launcher can still
    // refuse is what the plan does not see: a ring launch whose T puts a direction's output rows past 2 GiB (rnn_ring_rows_fit),
    // a stamp build asked for a shape without a stamp instantiation, the carried-state preconditions of launch_rnn_persist
    // (tools/asan/host_fuzz.cpp rnn_plan_check holds every planned launch of its grid to the table).  The layer still runs.
    if (plan.x16) {
        // first: the x-projection is in the 16-unit column order, so redo it in the other, and plan without the 16-unit kernels
        // (the first-generation kernel if eligible)
        gl.w_sp = m->rnn[l].wih_sp; gl.bias = m->rnn[l].bih; gl.N = m->geom.Np; gl.ldc = m->geom.Np; gl.ev = EvPair{};
        m->last_xp_wgs = launch_gemm(gl, s);
        m->last_xp_cols = gl.ldc;
        in.have16 = false;
        plan = plan_rnn_layer(in);
        if (run_rnn_plan(m, plan, l, B, To, dst, sumlen, s)) return;
    }
    in.rnn_mode = 0;      // then: per step (never refused: dsmi_debug_last_rnn_plan always holds THIS layer's launches, not the one before's)
    (void)run_rnn_plan(m, plan_rnn_layer(in), l, B, To, dst, sumlen, s);
}

static GemmLaunch xproj_gemm(dsmi_model* m, int l, int B, int To) {
    GemmLaunch gl{};
    const RnnW& r = m->rnn[l];
    gl.w = r.wih; gl.bias = r.bih; gl.c = m->xp;
    gl.w_sp = m->gemm_mode == 1 ? r.wih_sp : nullptr;
    gl.a_sp = m->a_sp; gl.tile_cnt = m->dense_tiles ? m->tile_counters(dsmi_model::kTileCntGemm) : nullptr; gl.n_cus = m->n_cus;
    gl.M = To * B; gl.N = m->geom.Np; gl.K = r.K; gl.ldw = r.ldw; gl.ldc = m->geom.Np;
    gl.B = B; gl.T = To;
    return gl;
}

// host_out_lens -> lens_dev through a small ring of pinned staging slots (an async copy must not read pageable
// memory that the next call overwrites); a slot is reused only after the copy that read it has completed.
static int stage_lens(dsmi_model* m, int B, hipStream_t s) {
    if (B > m->stage_cap) {
        HIP_OK(m, hipDeviceSynchronize());
        if (m->lens_stage) (void)hipHostFree(m->lens_stage);
        m->lens_stage = nullptr;
        const int cap = std::max(B, 64);
        HIP_OK(m, hipHostMalloc((void**)&m->lens_stage, sizeof(int32_t) * (size_t)cap * dsmi_model::kStage, hipHostMallocDefault));
        m->stage_cap = cap;
        for (int i = 0; i < dsmi_model::kStage; ++i) {
            if (!m->stage_ev[i]) HIP_OK(m, hipEventCreateWithFlags(&m->stage_ev[i], hipEventDisableTiming));
            m->stage_used[i] = false;
        }
    }
    const int slot = m->stage_next++ % dsmi_model::kStage;
    if (m->stage_used[slot]) HIP_OK(m, hipEventSynchronize(m->stage_ev[slot]));
    int32_t* h = m->lens_stage + (size_t)slot * m->stage_cap;
    std::memcpy(h, m->host_out_lens.data(), sizeof(int32_t) * B);
    HIP_OK(m, hipMemcpyAsync(m->lens_dev, h, sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    HIP_OK(m, hipEventRecord(m->stage_ev[slot], s));
    m->stage_used[slot] = true;
    return DSMI_OK;
}

static int forward_enqueue(dsmi_model* m, const float* feat, int B, int T, float* probs, hipStream_t s);

// After a hand-off timeout: clear the error word and keep this handle on the per-step path from now on.
static int persist_give_up(dsmi_model* m, hipStream_t s) {
    m->rnn_mode = 0;
    HIP_OK(m, hipMemsetAsync(m->perr, 0, sizeof(unsigned), s));
    return DSMI_OK;
}

// Collect the oldest uncollected forward (its event has completed or `wait`): DSMI_OK, DSMI_RECOMPUTED or < 0.
static int collect_oldest(dsmi_model* m, bool recompute) {
    dsmi_model::FwdSlot& f = m->fwd[m->fwd_head];
    HIP_OK(m, hipEventSynchronize(f.done));
    m->fwd_head = (m->fwd_head + 1) % dsmi_model::kFwdRing;
    m->fwd_count -= 1;
    if (*f.err_host == 0) return DSMI_OK;
    *f.err_host = 0;
    hipStream_t s = (hipStream_t)f.stream;
    int rc;
    if ((rc = persist_give_up(m, s))) return rc;
    if (!recompute)
        return fail(m, DSMI_ERR_TIMEOUT, "the persistent recurrent kernel timed out in an earlier forward whose status was never "
                                         "collected with dsmi_forward_status: those results were invalid; this handle now runs "
                                         "one launch per step");
    m->host_out_lens.resize(f.B);
    for (int i = 0; i < f.B; ++i) m->host_out_lens[i] = seq_len(m, f.lens[i]);
    if ((rc = forward_enqueue(m, f.feat, f.B, f.T, f.probs, s))) return rc;
    HIP_OK(m, hipStreamSynchronize(s));
    m->recomputed += 1;
    m->err = "a hand-off wait of the persistent recurrent kernel timed out; the batch was recomputed with one launch per step";
    return DSMI_RECOMPUTED;
}

extern "C" int dsmi_forward(dsmi_model* m, const float* feat, const int32_t* lens, int B, int T, float* probs,
                            int32_t* out_lens, void* stream) {
    if (!m) return DSMI_ERR_INVALID;
    int rc = check_batch(m, lens, B, T);
    if (rc) return rc;
    if (!feat || !probs || !out_lens) return fail(m, DSMI_ERR_INVALID, "null buffer");
    if ((rc = dsmi_reserve(m, B, T))) return rc;
    HIP_OK(m, hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    // Forwards whose status the caller has not collected: drop the finished good ones, fail loudly on a finished bad one
    // (its results were invalid and may have been consumed), and never keep more than the ring holds in flight.
    while (m->fwd_count > 0) {
        const bool full = m->fwd_count == dsmi_model::kFwdRing;
        if (!full && hipEventQuery(m->fwd[m->fwd_head].done) != hipSuccess) break;
        if ((rc = collect_oldest(m, false)) < 0) return rc;
    }
    for (int i = 0; i < B; ++i) out_lens[i] = seq_len(m, lens[i]);
    m->host_out_lens.assign(out_lens, out_lens + B);
    if ((rc = forward_enqueue(m, feat, B, T, probs, s))) return rc;
    dsmi_model::FwdSlot& f = m->fwd[(m->fwd_head + m->fwd_count) % dsmi_model::kFwdRing];
    f.feat = feat; f.probs = probs; f.lens.assign(lens, lens + B); f.B = B; f.T = T; f.stream = stream;
    HIP_OK(m, hipMemcpyAsync(f.err_host, m->perr, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    HIP_OK(m, hipEventRecord(f.done, s));
    m->fwd_count += 1;
    return DSMI_OK;
}

// See include/dsmi.h.  Collects the OLDEST dsmi_forward of this handle whose status has not been collected yet.
extern "C" int dsmi_forward_status(dsmi_model* m) {
    if (!m) return DSMI_ERR_INVALID;
    if (m->fwd_count == 0) return DSMI_OK;
    HIP_OK(m, hipSetDevice(m->device));
    return collect_oldest(m, true);
}

// See include/dsmi.h: has the handle's oldest uncollected forward finished?  Never blocks.
extern "C" int dsmi_forward_ready(dsmi_model* m) {
    if (!m) return DSMI_ERR_INVALID;
    if (m->fwd_count == 0) return 1;
    (void)hipSetDevice(m->device);
    const hipError_t e = hipEventQuery(m->fwd[m->fwd_head].done);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    m->err = std::string("hipEventQuery: ") + hipGetErrorString(e);
    return DSMI_ERR_HIP;
}

// The output head on the last layer's rows in hbuf[src]; a unidirectional model's lookahead is launched here, in front of it.
static HeadLaunch head_launch(const dsmi_model* m, int src, int B, int To, float* probs, hipStream_t s) {
    const dsmi_model_desc& d = m->desc;
    HeadLaunch h;
    h.bn_a = m->fc_a; h.bn_b = m->fc_b; h.w_packed = m->fc_wp; h.H = d.rnn_hidden_size; h.C = d.n_labels;
    h.T = To; h.B = B; h.probs = probs;
    if (!d.bidirectional) {   // model.py:508-509
        launch_lookahead(m->hbuf[src][0], m->look_w, m->look_buf, To, B, d.rnn_hidden_size, d.context, s);
        h.x1 = m->look_buf; h.x2 = nullptr;
    } else {
        h.x1 = m->hbuf[src][0]; h.x2 = m->hbuf[src][1];
    }
    return h;
}

static int forward_enqueue(dsmi_model* m, const float* feat, int B, int T, float* probs, hipStream_t s) {
    int rc;
    const dsmi_model_desc& d = m->desc;
    const int To = seq_len(m, T), ys = round_up(To, 4);
    const int32_t* out_lens = m->host_out_lens.data();
    if ((rc = stage_lens(m, B, s))) return rc;
    if (m->Hs != d.rnn_hidden_size)
        for (int i = 0; i < 2; ++i)
            for (int dd = 0; dd < m->geom.D; ++dd)
                HIP_OK(m, hipMemsetAsync(m->hbuf[i][dd], 0, sizeof(float) * (size_t)To * B * m->Hs, s));

    if (m->profiling) HIP_OK(m, hipEventRecord(m->ev[0], s));
    const float* cx;
    DenseHold hold(m->device, m->inflight, DENSE_CONV_STACK, s);     // (gate.hip: dense_enter_kernel)
    run_conv(m, feat, B, T, To, ys, s, &cx);
    hold.leave();
    if (m->profiling) HIP_OK(m, hipEventRecord(m->ev[1], s));

    for (int l = 0; l < d.rnn_layers; ++l) {
        GemmLaunch gl = xproj_gemm(m, l, B, To);
        if (l == 0) {
            gl.mode = GEMM_A_CONV; gl.a = cx; gl.ys = ys;
        } else {
            gl.mode = GEMM_A_SUM_BN;
            gl.a = m->hbuf[(l - 1) & 1][0]; gl.a2 = m->geom.D == 2 ? m->hbuf[(l - 1) & 1][1] : nullptr;
            gl.alpha = m->rnn[l].bn_a; gl.beta = m->rnn[l].bn_b; gl.lda = m->Hs;
        }
        run_rnn_layer(m, l, gl, B, To, l & 1, s);
    }
    if (m->profiling) HIP_OK(m, hipEventRecord(m->ev[2], s));
    HeadLaunch h = head_launch(m, (d.rnn_layers - 1) & 1, B, To, probs, s);
    {
        double sumlen = 0;
        for (int i = 0; i < B; ++i) sumlen += out_lens[i];
        h.ev = timer_arm(m, KK_HEAD, true, 2.0 * sumlen * d.rnn_hidden_size * d.n_labels,
                         4.0 * To * B * ((d.bidirectional ? 2.0 : 1.0) * m->Hs + d.n_labels));
    }
    launch_head(h, s);
    if (m->profiling) HIP_OK(m, hipEventRecord(m->ev[3], s));
    HIP_OK(m, hipGetLastError());

    // bookkeeping for roofline maths: recurrent and total algorithmic FLOPs
    m->n_step_launches = (int64_t)To * d.rnn_layers;
    double rec = 0, tot = 0;
    for (int i = 0; i < B; ++i) {
        const double t = out_lens[i];
        double conv = 0;
        for (int l = 0; l < d.conv_layers; ++l) {
            const ConvSpec& sp = kConvSpecs[l];
            conv += (double)sp.co * m->conv_fo[l] * t * sp.ci * sp.kf * sp.kt;
        }
        const double H = d.rnn_hidden_size, G = m->geom.G, D = m->geom.D;
        double r = 0, ip = 0;
        for (int l = 0; l < d.rnn_layers; ++l) {
            r += D * t * G * H * H;
            ip += D * t * G * H * (l == 0 ? m->I0 : H);
        }
        rec += 2 * r;
        tot += 2 * (conv + r + ip + t * H * d.n_labels);
    }
    m->step_flops = rec;
    m->total_flops = tot;
    if (m->profiling == 1) {
        HIP_OK(m, hipStreamSynchronize(s));
        float ms;
        HIP_OK(m, hipEventElapsedTime(&ms, m->ev[0], m->ev[1])); m->stage_us[0] = ms * 1e3;
        HIP_OK(m, hipEventElapsedTime(&ms, m->ev[1], m->ev[2])); m->stage_us[2] = ms * 1e3;  // GEMMs + steps
        HIP_OK(m, hipEventElapsedTime(&ms, m->ev[2], m->ev[3])); m->stage_us[3] = ms * 1e3;
        HIP_OK(m, hipEventElapsedTime(&ms, m->ev[0], m->ev[3])); m->stage_us[4] = ms * 1e3;
        m->stage_us[1] = 0;
    }
    return DSMI_OK;
}

extern "C" int dsmi_conv_stack(dsmi_model* m, const float* feat, const int32_t* lens, int B, int T, float* out, void* stream) {
    if (!m) return DSMI_ERR_INVALID;
    int rc = check_batch(m, lens, B, T);
    if (rc) return rc;
    if ((rc = dsmi_reserve(m, B, T))) return rc;
    HIP_OK(m, hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int To = seq_len(m, T), ys = round_up(To, 4);
    m->host_out_lens.resize(B);
    for (int i = 0; i < B; ++i) m->host_out_lens[i] = seq_len(m, lens[i]);
    if ((rc = stage_lens(m, B, s))) return rc;
    const float* cx;
    run_conv(m, feat, B, T, To, ys, s, &cx);
    // strip the time-stride padding: [B][C*F][ys] -> [B][C*F][To]
    const int cl = m->desc.conv_layers - 1;
    const size_t rows = (size_t)B * kConvSpecs[cl].co * m->conv_fo[cl];
    HIP_OK(m, hipMemcpy2DAsync(out, sizeof(float) * To, cx, sizeof(float) * ys, sizeof(float) * To, rows, hipMemcpyDeviceToDevice, s));
    HIP_OK(m, hipStreamSynchronize(s));
    HIP_OK(m, hipGetLastError());
    return DSMI_OK;
}

extern "C" int dsmi_rnn_layer(dsmi_model* m, int layer, const float* x, const int32_t* out_lens, int B, int To, float* y, void* stream) {
    if (!m) return DSMI_ERR_INVALID;
    if (!m->finalized) return fail(m, DSMI_ERR_NOT_READY, "dsmi_model_finalize has not been called");
    if (layer < 0 || layer >= m->desc.rnn_layers || !x || !y || !out_lens || B < 1 || To < 1) return fail(m, DSMI_ERR_INVALID, "bad rnn_layer arguments");
    int rc;
    if ((rc = check_lens(m, out_lens, B, To))) return rc;
    const int Tin = frames_for(To);      // workspaces are sized by input frames
    if ((rc = dsmi_reserve(m, B, Tin))) return rc;
    HIP_OK(m, hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int H = m->desc.rnn_hidden_size;
    m->host_out_lens.assign(out_lens, out_lens + B);
    if ((rc = stage_lens(m, B, s))) return rc;
    const RnnW& r = m->rnn[layer];
    const int I = layer == 0 ? m->I0 : H;
    for (int attempt = 0; attempt < 2; ++attempt) {
        for (int dd = 0; dd < m->geom.D; ++dd)
            HIP_OK(m, hipMemsetAsync(m->hbuf[0][dd], 0, sizeof(float) * (size_t)To * B * m->Hs, s));
        launch_pad_rows(x, m->xin, (size_t)To * B, I, r.ldw, s);
        GemmLaunch gl = xproj_gemm(m, layer, B, To);
        if (layer == 0) {
            gl.mode = GEMM_A_ROWMAJOR; gl.a = m->xin; gl.lda = r.ldw;
        } else {
            gl.mode = GEMM_A_SUM_BN; gl.a = m->xin; gl.a2 = nullptr; gl.alpha = r.bn_a; gl.beta = r.bn_b; gl.lda = r.ldw;
        }
        run_rnn_layer(m, layer, gl, B, To, 0, s);
        launch_add2(m->hbuf[0][0], m->geom.D == 2 ? m->hbuf[0][1] : nullptr, y, (size_t)To * B, H, m->Hs, s);
        HIP_OK(m, hipStreamSynchronize(s));
        HIP_OK(m, hipGetLastError());
        // a hand-off timeout of the persistent kernel: recompute this layer with one launch per step, in this call
        unsigned e = 0;
        HIP_OK(m, hipMemcpy(&e, m->perr, sizeof(unsigned), hipMemcpyDeviceToHost));
        if (!e) return DSMI_OK;
        if (attempt == 1) return fail(m, DSMI_ERR_TIMEOUT, "recurrent layer timed out on the per-step path");
        HIP_OK(m, hipMemset(m->perr, 0, sizeof(unsigned)));
        m->rnn_mode = 0;
        m->recomputed += 1;
    }
    return DSMI_OK;
}

// See include/dsmi.h: the output head by itself, on rows the caller supplies (the last layer's outputs per direction).
extern "C" int dsmi_head(dsmi_model* m, const float* x_fwd, const float* x_rev, int B, int To, float* probs, void* stream) {
    if (!m) return DSMI_ERR_INVALID;
    if (!m->finalized) return fail(m, DSMI_ERR_NOT_READY, "dsmi_model_finalize has not been called");
    const dsmi_model_desc& d = m->desc;
    if (!x_fwd || !probs || B < 1 || To < 1) return fail(m, DSMI_ERR_INVALID, "bad head arguments");
    if ((x_rev != nullptr) != (d.bidirectional != 0))
        return fail(m, DSMI_ERR_INVALID, d.bidirectional ? "a bidirectional model's head needs the reverse direction's rows"
                                                         : "a unidirectional model's head takes no reverse direction");
    if ((int64_t)To * B > (int64_t)1 << 24) return fail(m, DSMI_ERR_INVALID, "more than 2^24 rows");      // (head_kernel counts rows in an int)
    const int Tin = frames_for(To);      // workspaces are sized by input frames
    int rc;
    if ((rc = dsmi_reserve(m, B, Tin))) return rc;
    HIP_OK(m, hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    const int H = d.rnn_hidden_size;
    const size_t rows = (size_t)To * B;
    launch_pad_rows(x_fwd, m->hbuf[0][0], rows, H, m->Hs, s);
    if (x_rev) launch_pad_rows(x_rev, m->hbuf[0][1], rows, H, m->Hs, s);
    HeadLaunch h = head_launch(m, 0, B, To, probs, s);
    h.ev = timer_arm(m, KK_HEAD, true, 2.0 * rows * H * d.n_labels, 4.0 * rows * ((d.bidirectional ? 2.0 : 1.0) * m->Hs + d.n_labels));
    launch_head(h, s);
    HIP_OK(m, hipStreamSynchronize(s));
    HIP_OK(m, hipGetLastError());
    return DSMI_OK;
}

// stream.hip's batched pass (dsmi_stream_forward_many): one carried-state launch of the first-generation persistent layer.  Sized
// for the whole device like the offline first-generation launch, so it takes every gate slot and never shares the chip with another
// persistent kernel of the process; the launch description comes from persist_launch: the same test hooks apply.
bool stream_persist_layer(dsmi_model* m, const RnnPersistLaunch& pl, hipStream_t s) {
    RnnLaunch whole;
    whole.gate = GATE_LANES; whole.slot0 = 0; whole.nslots = kMaxLanes;
    GateTurn turn;
    turn.wait(m->device, s, whole, m->n_cus);
    const bool ok = launch_rnn_persist(pl, s);
    turn.record();
    return ok;
}

extern "C" int dsmi_recompute_count(const dsmi_model* m) { return m ? m->recomputed : DSMI_ERR_INVALID; }

extern "C" int dsmi_model_set_inflight(dsmi_model* m, int batches) {
    if (!m || batches < 1) return DSMI_ERR_INVALID;
    m->inflight = batches;
    return DSMI_OK;
}

extern "C" int dsmi_model_set_ring_windows(dsmi_model* m, int windows) {
    if (!m || windows < 0) return DSMI_ERR_INVALID;
    m->ring_windows = windows;
    return DSMI_OK;
}
