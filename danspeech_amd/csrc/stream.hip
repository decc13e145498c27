// Chunked unidirectional inference on the GPU (gfx950): the handle behind dsmi_stream*.
//
// Replaces DeepSpeech(streaming_inference_model=True).streaming_forward of the reference
// (danspeech/deepspeech/model.py:517-537) together with the state its modules carry between calls:
//   MaskConvStream   (model.py:156-201)  the last 10 input frames of each conv layer (after the chunk's
//                                        own first/last padding), glued in front of the next chunk;
//   BatchRNNStream   (model.py:204-238)  h (and c) of every unidirectional layer;
//   LookaheadStream  (model.py:241-283)  the frames whose right context has not arrived yet; the first
//                                        pass only fills this buffer and yields no output.
// The arithmetic runs on the same kernels as the offline path in their fp32-MFMA form: conv_kernel<L>
// on explicitly assembled inputs (full-length mask), gemm_f32 for the x-projection, rnn_step_kernel with
// its carried-state entry (hcarry / parity offset), lookahead_kernel and head_kernel.  One utterance
// (B = 1) per stream; a model can serve any number of streams, each owns its buffers, and
// dsmi_stream_forward_many (below) advances many of them in one batched pass.
// Only 2-conv models: the reference's streaming_init sizes the first RNN layer for two conv layers
// whatever conv_layers says (model.py:476-484) and builds a non-streaming MaskConv for one.
#include "model.h"
#include "stream_host.h"

#include <algorithm>
#include <cstring>
#include <mutex>

using namespace dsmi;

struct dsmi_stream {
    dsmi_model* m = nullptr;
    std::string err;
    // carried state
    StreamFlags f;                           // which of the buffers below hold something (stream_host.h)
    float* left[2] = {nullptr, nullptr};     // [ci*fi][10] per conv layer
    std::vector<float*> hpack;               // per layer [2][nq][64][4]
    std::vector<float*> hcarry, ccarry;      // per layer [Hs]
    std::vector<int> pbase;
    float* la_buf = nullptr;                 // [la_cap][Hs]
    int la_cap = 0;
    int32_t* lens_dev = nullptr;             // [2]: full-length masks of the two conv launches; [2] = INT_MAX for the RNN
    // per-call workspaces (grow only)
    int cap_T = 0;
    float *xin1 = nullptr, *y1 = nullptr, *xin2 = nullptr, *y2 = nullptr, *xp = nullptr, *hb[2] = {nullptr, nullptr};
    float *cat = nullptr, *la_out = nullptr;
    int cat_cap = 0;
};

static thread_local std::string g_stream_error;

// `err`: where the message goes, a handle's err (the single call) or g_stream_error (the batched call)
#define S_HIP(err, expr)                                                                                          \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess) { (err) = std::string(#expr) + ": " + hipGetErrorString(e_); return DSMI_ERR_HIP; } \
    } while (0)

static int sfail(dsmi_stream* st, int code, const char* msg) { st->err = msg; return code; }

static void free_p(float*& p) { if (p) (void)hipFree(p); p = nullptr; }

extern "C" int dsmi_stream_create(dsmi_model* m, dsmi_stream** out) {
    if (!m || !out) { g_stream_error = "null argument"; return DSMI_ERR_INVALID; }
    if (!m->finalized) { g_stream_error = "dsmi_model_finalize has not been called"; return DSMI_ERR_NOT_READY; }
    if (m->desc.bidirectional || m->desc.conv_layers != 2) {
        g_stream_error = "streaming needs a unidirectional 2-conv model (reference model.py:427-494)";
        return DSMI_ERR_INVALID;
    }
    if (hipSetDevice(m->device) != hipSuccess) { g_stream_error = "hipSetDevice failed"; return DSMI_ERR_HIP; }
    dsmi_stream* st = new dsmi_stream();
    st->m = m;
    const int L = m->desc.rnn_layers;
    st->hpack.assign(L, nullptr); st->hcarry.assign(L, nullptr); st->ccarry.assign(L, nullptr); st->pbase.assign(L, 0);
    bool ok = true;
    for (int l = 0; l < 2 && ok; ++l)
        ok = hipMalloc((void**)&st->left[l], sizeof(float) * kConvSpecs[l].ci * m->conv_fi[l] * 10) == hipSuccess;
    for (int l = 0; l < L && ok; ++l) {
        const size_t np = (size_t)2 * m->geom.nq * 256;
        ok = hipMalloc((void**)&st->hpack[l], sizeof(float) * np) == hipSuccess &&
             hipMemset(st->hpack[l], 0, sizeof(float) * np) == hipSuccess &&
             hipMalloc((void**)&st->hcarry[l], sizeof(float) * m->Hs) == hipSuccess &&
             hipMalloc((void**)&st->ccarry[l], sizeof(float) * m->Hs) == hipSuccess &&
             hipMemset(st->ccarry[l], 0, sizeof(float) * m->Hs) == hipSuccess;
    }
    ok = ok && hipMalloc((void**)&st->lens_dev, sizeof(int32_t) * 4) == hipSuccess;
    if (!ok) { g_stream_error = "stream: HIP allocation failed"; dsmi_stream_destroy(st); return DSMI_ERR_NOMEM; }
    *out = st;
    return DSMI_OK;
}

extern "C" void dsmi_stream_destroy(dsmi_stream* st) {
    if (!st) return;
    (void)hipSetDevice(st->m->device);
    (void)hipDeviceSynchronize();
    for (int l = 0; l < 2; ++l) free_p(st->left[l]);
    for (float*& p : st->hpack) free_p(p);
    for (float*& p : st->hcarry) free_p(p);
    for (float*& p : st->ccarry) free_p(p);
    free_p(st->la_buf);
    if (st->lens_dev) (void)hipFree(st->lens_dev);
    for (float** p : {&st->xin1, &st->y1, &st->xin2, &st->y2, &st->xp, &st->hb[0], &st->hb[1], &st->cat, &st->la_out}) free_p(*p);
    delete st;
}

extern "C" const char* dsmi_stream_last_error(const dsmi_stream* st) { return st ? st->err.c_str() : g_stream_error.c_str(); }

// What is_last does to every module (model.py:234-236, 279-281; MaskConvStream simply stops storing).
extern "C" int dsmi_stream_reset(dsmi_stream* st) {
    if (!st) return DSMI_ERR_INVALID;
    st->f = StreamFlags();
    std::fill(st->pbase.begin(), st->pbase.end(), 0);
    return DSMI_OK;
}

// What dsmi_debug_last_rnn_plan reports of a streaming pass: the launch of the recurrent layer that ran last.  persist8: the
// carried-state launch of stream_persist_layer (direction 0, one direction, every lane slot of the gate, one CU per workgroup);
// steps: rnn_step_kernel per step -- not eligible, DSMI_RNN_MODE=steps, refused, or the recomputation of a timed-out pass.
static void record_stream_plan(dsmi_model* m, bool persisted) {
    RnnLaunch l;
    if (persisted) {
        l.kernel = RNN_PERSIST8; l.at = 0; l.n = 1;
        l.gate = GATE_LANES; l.slot0 = 0; l.nslots = kMaxLanes; l.cus = m->geom.nwg;
    }
    m->last_plan_x16 = false; m->last_plan_n = 1; m->last_plan[0] = l;
}

static int ensure(dsmi_stream* st, int T) {
    if (T <= st->cap_T) return DSMI_OK;
    dsmi_model* m = st->m;
    S_HIP(st->err, hipDeviceSynchronize());
    for (float** p : {&st->xin1, &st->y1, &st->xin2, &st->y2, &st->xp, &st->hb[0], &st->hb[1]}) free_p(*p);
    const int cap = std::max(T, 64) * 2;
    const int tin1 = cap + 15, to1 = conv_t1(tin1), tin2 = to1 + 15, to2 = tin2;
    const size_t f = m->n_freq;
    S_HIP(st->err, hipMalloc((void**)&st->xin1, sizeof(float) * f * tin1));
    S_HIP(st->err, hipMalloc((void**)&st->y1, sizeof(float) * 32 * m->conv_fo[0] * round_up(to1, 4)));
    S_HIP(st->err, hipMalloc((void**)&st->xin2, sizeof(float) * 32 * m->conv_fo[0] * tin2));
    S_HIP(st->err, hipMalloc((void**)&st->y2, sizeof(float) * 32 * m->conv_fo[1] * round_up(to2, 4)));
    S_HIP(st->err, hipMalloc((void**)&st->xp, sizeof(float) * (size_t)to2 * m->geom.Np));
    for (int i = 0; i < 2; ++i) S_HIP(st->err, hipMalloc((void**)&st->hb[i], sizeof(float) * (size_t)to2 * m->Hs));
    st->cap_T = cap;
    return DSMI_OK;
}

// [rows][w] sub-matrix copy between row strides
static hipError_t copy2d(float* dst, int dst_stride, const float* src, int src_stride, int rows, int w, hipStream_t s) {
    if (w <= 0 || rows <= 0) return hipSuccess;
    return hipMemcpy2DAsync(dst, sizeof(float) * dst_stride, src, sizeof(float) * src_stride, sizeof(float) * w, rows,
                            hipMemcpyDeviceToDevice, s);
}

// Room for `rows` rows in the handle's lookahead buffer; the rows it holds are kept.  Allocation only.  `err` as for S_HIP.
static int grow_la(dsmi_stream* st, int rows, hipStream_t s, std::string& err) {
    if (rows <= st->la_cap) return DSMI_OK;
    const int Hs = st->m->Hs;
    float* nb = nullptr;
    S_HIP(err, hipMalloc((void**)&nb, sizeof(float) * (size_t)rows * 2 * Hs));
    if (st->la_buf) {
        S_HIP(err, hipMemcpyAsync(nb, st->la_buf, sizeof(float) * (size_t)st->f.la_rows * Hs, hipMemcpyDeviceToDevice, s));
        S_HIP(err, hipStreamSynchronize(s));
        (void)hipFree(st->la_buf);
    }
    st->la_buf = nb; st->la_cap = rows * 2;
    return DSMI_OK;
}

// ---- the launches both executors make, from the model, the layer and what differs between them: the batch, the frames, the buffers
static ConvLaunch conv_launch(const dsmi_model* m, int l, int B, const float* x, float* y, const int32_t* lens, int ti, int to,
                              int ys) {
    const ConvSpec& sp = kConvSpecs[l];
    ConvLaunch c;
    c.x = x; c.y = y; c.wp = m->conv[l].wp; c.bias = m->conv[l].bias; c.bn_a = m->conv[l].bn_a; c.bn_b = m->conv[l].bn_b;
    c.out_lens_dev = lens;
    c.B = B; c.ci = sp.ci; c.co = sp.co; c.fi = m->conv_fi[l]; c.fo = m->conv_fo[l];
    c.ti = ti; c.to = to; c.xs = ti; c.ys = ys; c.layer = l; c.y_sp = nullptr;
    return c;
}

// layer l's x-projection of T frames of B sessions into xp; a: conv2's output (time stride ys) for layer 0, else layer l - 1's output
static GemmLaunch xproj_launch(const dsmi_model* m, int l, int B, int T, const float* a, int ys, float* xp) {
    const RnnW& r = m->rnn[l];
    GemmLaunch gl{};
    gl.w = r.wih; gl.bias = r.bih; gl.c = xp; gl.w_sp = nullptr; gl.a_sp = nullptr; gl.a = a;
    gl.M = T * B; gl.N = m->geom.Np; gl.K = r.K; gl.ldw = r.ldw; gl.ldc = m->geom.Np; gl.B = B; gl.T = T;
    if (l == 0) { gl.mode = GEMM_A_CONV; gl.ys = ys; }
    else { gl.mode = GEMM_A_SUM_BN; gl.a2 = nullptr; gl.alpha = r.bn_a; gl.beta = r.bn_b; gl.lda = m->Hs; }
    return gl;
}

// layer l per step from the carried state (hcarry null: zero); the caller sets .step
static RnnStepLaunch step_launch(const dsmi_model* m, int l, int B, int T, const float* xp, const int32_t* lens, float* out,
                                 float* cstate, float* hpack, const float* hcarry, int pbase) {
    const RnnW& r = m->rnn[l];
    RnnStepLaunch sl;
    sl.g = m->geom;
    sl.whh_packed[0] = r.whh[0]; sl.whh_packed[1] = nullptr; sl.bhh[0] = r.bhh[0]; sl.bhh[1] = nullptr;
    sl.out[0] = out; sl.out[1] = nullptr; sl.cstate[0] = cstate; sl.cstate[1] = nullptr;
    sl.xp = xp; sl.lens_dev = lens; sl.B = B; sl.T = T; sl.hpack = hpack; sl.hcarry = hcarry; sl.pbase = pbase;
    return sl;
}

// fc + softmax (model.py:531-536) of T rows of B sessions of the lookahead's output
static HeadLaunch head_launch(const dsmi_model* m, int B, int T, const float* x, float* probs) {
    HeadLaunch h;
    h.bn_a = m->fc_a; h.bn_b = m->fc_b; h.w_packed = m->fc_wp; h.H = m->desc.rnn_hidden_size; h.C = m->desc.n_labels;
    h.T = T; h.B = B; h.probs = probs; h.x1 = x; h.x2 = nullptr;
    return h;
}

// The pass is planned (stream_host.h) before anything is allocated or enqueued: a refused call changes nothing.  The handle's flags and
// parities are committed once, where the whole pass, a buffering one included, has been enqueued without error.  After a HIP error
// mid-pass they are as before while the device buffers may be partly overwritten: the carried state is undefined until dsmi_stream_reset.
extern "C" int dsmi_stream_forward(dsmi_stream* st, const float* feat, int T, int is_first, int is_last, float* probs,
                                   int T_out_cap, int32_t* T_out, void* stream) {
    if (!st) return DSMI_ERR_INVALID;
    if (!feat || !T_out || T < 1) return sfail(st, DSMI_ERR_INVALID, "bad stream arguments");
    dsmi_model* m = st->m;
    const dsmi_model_desc& d = m->desc;
    S_HIP(st->err, hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    *T_out = 0;
    StreamPass p;
    const char* why = nullptr;
    int rc = stream_pass_plan(st->f, T, is_first != 0, is_last != 0, d.context, probs != nullptr, T_out_cap, &p, &why);
    if (rc) return sfail(st, rc, why);
    if ((rc = ensure(st, T))) return rc;

    // ---- MaskConvStream (model.py:171-201): per conv layer, pad / glue the left context, remember the tail
    const int Tc = p.to[1], ys[2] = {round_up(p.to[0], 4), round_up(Tc, 4)};
    const int32_t lens_host[4] = {p.to[0], Tc, 0x7fffffff, 0};
    S_HIP(st->err, hipMemcpyAsync(st->lens_dev, lens_host, sizeof(lens_host), hipMemcpyHostToDevice, s));
    const float* src[2] = {feat, st->y1};
    const int src_stride[2] = {T, ys[0]}, src_w[2] = {T, p.to[0]};
    float* xin[2] = {st->xin1, st->xin2};
    float* yv[2] = {st->y1, st->y2};
    for (int l = 0; l < 2; ++l) {
        const int rows = kConvSpecs[l].ci * m->conv_fi[l], tin = p.tin[l];
        if (p.padl || p.padr) S_HIP(st->err, hipMemsetAsync(xin[l], 0, sizeof(float) * (size_t)rows * tin, s));
        if (p.ctxl) S_HIP(st->err, copy2d(xin[l], tin, st->left[l], 10, rows, 10, s));
        S_HIP(st->err, copy2d(xin[l] + p.ctxl + p.padl, tin, src[l], src_stride[l], rows, src_w[l], s));
        if (!is_last) S_HIP(st->err, copy2d(st->left[l], 10, xin[l] + tin - 10, tin, rows, 10, s));
        launch_conv(conv_launch(m, l, 1, xin[l], yv[l], st->lens_dev + l, tin, p.to[l], ys[l]), s);
    }

    // ---- BatchRNNStream x layers (model.py:219-238): x-projection of the chunk, then Tc steps from the carried state
    const int Hs = m->Hs;
    for (int l = 0; l < d.rnn_layers; ++l) {
        launch_gemm(xproj_launch(m, l, 1, Tc, l == 0 ? st->y2 : st->hb[(l - 1) & 1], ys[1], st->xp), s);
        float* out = st->hb[l & 1];
        if (Hs != d.rnn_hidden_size) S_HIP(st->err, hipMemsetAsync(out, 0, sizeof(float) * (size_t)Tc * Hs, s));
        RnnStepLaunch sl = step_launch(m, l, 1, Tc, st->xp, st->lens_dev + 2, out, st->ccarry[l], st->hpack[l],
                                       st->f.has_hidden ? st->hcarry[l] : nullptr, st->pbase[l]);
        for (int step = 0; step < Tc; ++step) { sl.step = step; launch_rnn_step(sl, s); }
        record_stream_plan(m, false);
        S_HIP(st->err, hipMemcpyAsync(st->hcarry[l], out + (size_t)(Tc - 1) * Hs, sizeof(float) * Hs, hipMemcpyDeviceToDevice, s));
    }
    const float* x = st->hb[(d.rnn_layers - 1) & 1];

    // ---- LookaheadStream (model.py:256-283), then fc + softmax
    const int la_rows = st->f.la_rows;
    if (p.buffering) {                           // buffer the whole first chunk, no output yet
        if ((rc = grow_la(st, Tc, s, st->err))) return rc;
        S_HIP(st->err, hipMemcpyAsync(st->la_buf, x, sizeof(float) * (size_t)Tc * Hs, hipMemcpyDeviceToDevice, s));
    } else {
        if (p.ncat > st->cat_cap) {
            S_HIP(st->err, hipStreamSynchronize(s));
            free_p(st->cat); free_p(st->la_out);
            st->cat_cap = p.ncat * 2;
            S_HIP(st->err, hipMalloc((void**)&st->cat, sizeof(float) * (size_t)st->cat_cap * Hs));
            S_HIP(st->err, hipMalloc((void**)&st->la_out, sizeof(float) * (size_t)st->cat_cap * Hs));
        }
        S_HIP(st->err, hipMemcpyAsync(st->cat, st->la_buf, sizeof(float) * (size_t)la_rows * Hs, hipMemcpyDeviceToDevice, s));
        S_HIP(st->err, hipMemcpyAsync(st->cat + (size_t)la_rows * Hs, x, sizeof(float) * (size_t)Tc * Hs, hipMemcpyDeviceToDevice, s));
        if ((rc = grow_la(st, p.keep, s, st->err))) return rc;
        S_HIP(st->err, hipMemcpyAsync(st->la_buf, x + (size_t)(Tc - p.keep) * Hs, sizeof(float) * (size_t)p.keep * Hs,
                                      hipMemcpyDeviceToDevice, s));
        // rows past ncat count as zeros in the kernel: the is_last right padding; otherwise only the first nout rows are kept
        launch_lookahead(st->cat, m->look_w, st->la_out, p.ncat, 1, d.rnn_hidden_size, d.context, s);
        launch_head(head_launch(m, 1, p.nout, st->la_out, probs), s);
    }
    S_HIP(st->err, hipGetLastError());
    stream_pass_commit(st->f, st->pbase.data(), d.rnn_layers, p, is_last != 0);
    *T_out = p.nout;
    return DSMI_OK;
}

// ================================================================================================================================
// dsmi_stream_forward_many: N sessions (handles) of ONE model advance by one chunk each in one batched pass.  The sessions may be
// anywhere in their utterances and their chunks may differ in length; every step of the single call above runs once for all of
// them, so the number of launches depends on the longest chunk, never on N:
//   gather    stream_conv_in_kernel builds each conv layer's input, row by row: the session's left context, padding, its chunk
//             (conv1 output for conv2), padding, and zeros past the session's own length -- so the conv kernel's shared implicit
//             padding means what it means in the single call; conv_kernel<L> masks each session's outputs at its own length;
//   recurrent stream_seed_kernel gathers every session's carried h (natural and packed forms) and c into batch buffers; each
//             layer is ONE launch of rnn_persist.hip's carried-state variant (all steps, all sessions, tiles of 32 walked by
//             every workgroup) behind the whole-device gate, or -- not eligible, DSMI_RNN_MODE=steps, or its error word set --
//             rnn_step_kernel per step at B = N from the same seeded state.  Per-session lengths mask the steps past a session's
//             own last frame (h 0, c held), so each session's final state is that of its own last frame;
//   lookahead stream_cat_kernel concatenates each session's buffered rows with its new rows (zeros past its own row count: the
//             is_last right padding), then lookahead_kernel and head_kernel at B = N, and one 2-D copy into the caller's slots;
//   commit    stream_commit_kernel writes every session's new left tails, h (both forms, at its parity), c and lookahead rows
//             back to its handle -- only after the pass has succeeded (a timed-out persistent launch is recomputed first).
// Everything that can be refused is refused before any of this runs.  The call returns when the pass is complete.
constexpr int kMaxMany = 256;        // rnn_persist.hip's PMAXZ batch tiles of 32 sessions; the Python layer splits longer lists

struct SessDev {
    const float* feat; float* left[2]; float* la_buf;
    int T, ctxl, padl, is_last, seed, buffering, la_rows, ncat, keep;
    int tin[2], to[2];
};
struct LayerDev { float* hpack; float* hcarry; float* ccarry; int pbase; int pad; };

struct StreamBatch {
    std::mutex mu;
    std::vector<std::pair<void**, size_t>> bufs;       // (buffer, bytes) of everything below, for stream_batch_free
    char* tab_host = nullptr; size_t tab_host_cap = 0;
    void* tab = nullptr; size_t tab_cap = 0;
    float *xin[2] = {nullptr, nullptr}, *y[2] = {nullptr, nullptr}, *xp = nullptr, *hb = nullptr, *hseed = nullptr, *cwork = nullptr;
    float *hpack = nullptr, *cat = nullptr, *la_out = nullptr, *probs = nullptr;
    uint16_t* hpack_sp = nullptr;
    unsigned *cnt = nullptr, *err = nullptr;
    size_t cap[16] = {0};
};

void stream_batch_free(dsmi_model* m) {
    StreamBatch* b = m->sbatch;
    if (!b) return;
    for (void* p : {(void*)b->tab, (void*)b->xin[0], (void*)b->xin[1], (void*)b->y[0], (void*)b->y[1], (void*)b->xp, (void*)b->hb,
                    (void*)b->hseed, (void*)b->cwork, (void*)b->hpack, (void*)b->cat, (void*)b->la_out, (void*)b->probs,
                    (void*)b->hpack_sp, (void*)b->cnt, (void*)b->err})
        if (p) (void)hipFree(p);
    if (b->tab_host) (void)hipHostFree(b->tab_host);
    delete b;
    m->sbatch = nullptr;
}

// grow-only device buffer; `zero`: cleared when (re)allocated
template <typename T>
static bool grow_dev(T*& p, size_t& cap, size_t bytes, bool zero = false) {
    if (bytes <= cap) return true;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    if (hipMalloc((void**)&p, bytes) != hipSuccess) return false;
    if (zero && hipMemset(p, 0, bytes) != hipSuccess) return false;
    cap = bytes;
    return true;
}

// grid (blocks, N): conv layer l's input [N][rows][tinmax] of every session (see above)
__global__ __launch_bounds__(256) void stream_conv_in_kernel(const SessDev* sd, int l, const float* y1, int ys1, int rows, int tinmax, float* xin) {
    const int i = blockIdx.y;
    const SessDev& S = sd[i];
    const int w = l == 0 ? S.T : S.to[0];
    const size_t n = (size_t)rows * tinmax;
    float* dst = xin + (size_t)i * n;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < n; idx += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(idx / tinmax), t = (int)(idx % tinmax);
        float v = 0.f;
        if (t < S.ctxl) v = S.left[l][(size_t)r * 10 + t];
        else {
            const int u = t - S.ctxl - S.padl;
            if (u >= 0 && u < w) v = l == 0 ? S.feat[(size_t)r * S.T + u] : y1[((size_t)i * rows + r) * ys1 + u];
        }
        dst[idx] = v;
    }
}

// packed-state index of (unit u, batch row bl) in one [nq][64][4] tile (rnn_step.hip's B-operand lane order)
__device__ __forceinline__ size_t pk_idx(int u, int bl) { return ((size_t)(u >> 3) * 64 + ((u >> 2) & 1) * 32 + bl) * 4 + (u & 3); }

// grid (blocks, L): the carried state of every session and layer -> hseed / cwork [L][N][Hs] and parity 1 of the batch's packed
// state [L][2][nz][nq][256] (padding rows of the last tile zero)
__global__ __launch_bounds__(256) void stream_seed_kernel(const SessDev* sd, const LayerDev* ld, int n, int Hs, int nq, int nz,
                                                          float* hseed, float* cwork, float* hpack) {
    const int l = blockIdx.y;
    const size_t items = (size_t)nz * 32 * Hs;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < items; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx / Hs), u = (int)(idx % Hs);
        float hp = 0.f;
        if (i < n) {
            const LayerDev& L = ld[(size_t)l * n + i];
            const bool seed = sd[i].seed != 0;
            hseed[((size_t)l * n + i) * Hs + u] = seed ? L.hcarry[u] : 0.f;
            cwork[((size_t)l * n + i) * Hs + u] = seed ? L.ccarry[u] : 0.f;
            if (seed) hp = L.hpack[(size_t)((L.pbase ^ 1) * nq) * 256 + pk_idx(u, 0)];
        }
        hpack[(((size_t)l * 2 + 1) * nz + i / 32) * nq * 256 + pk_idx(u, i & 31)] = hp;
    }
}

// grid-stride over [ncatmax][N][Hs]: buffered rows, then the new rows of the last layer's output x [Tc][N][Hs], then zeros
__global__ __launch_bounds__(256) void stream_cat_kernel(const SessDev* sd, const float* x, int n, int Hs, int ncatmax, float* cat) {
    const size_t items = (size_t)ncatmax * n * Hs;
    for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < items; idx += (size_t)gridDim.x * blockDim.x) {
        const int h = (int)(idx % Hs);
        const int i = (int)((idx / Hs) % n);
        const int t = (int)(idx / ((size_t)Hs * n));
        const SessDev& S = sd[i];
        float v = 0.f;
        if (t < S.la_rows) v = S.la_buf[(size_t)t * Hs + h];
        else if (t < S.ncat) v = x[((size_t)(t - S.la_rows) * n + i) * Hs + h];
        cat[idx] = v;
    }
}

// grid (blocks, N): session i's new carried state back into its handle (what dsmi_stream_forward leaves there)
__global__ __launch_bounds__(256) void stream_commit_kernel(const SessDev* sd, const LayerDev* ld, int n, int L, int Hs, int nq,
                                                            const float* xin0, int rows0, int tin0, const float* xin1, int rows1, int tin1,
                                                            const float* hb, int tcmax, const float* cwork) {
    const int i = blockIdx.y;
    const SessDev& S = sd[i];
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    const int Tc = S.to[1];
    if (!S.is_last) {
        for (int k = tid; k < rows0 * 10; k += nth)
            S.left[0][k] = xin0[((size_t)i * rows0 + k / 10) * tin0 + S.tin[0] - 10 + k % 10];
        for (int k = tid; k < rows1 * 10; k += nth)
            S.left[1][k] = xin1[((size_t)i * rows1 + k / 10) * tin1 + S.tin[1] - 10 + k % 10];
    }
    for (int k = tid; k < L * Hs; k += nth) {
        const int l = k / Hs, u = k % Hs;
        const LayerDev& Ld = ld[(size_t)l * n + i];
        const float* out = hb + (size_t)l * tcmax * n * Hs;
        const float h = out[((size_t)(Tc - 1) * n + i) * Hs + u];
        Ld.hcarry[u] = h;
        Ld.ccarry[u] = cwork[((size_t)l * n + i) * Hs + u];
        const int par = (Tc - 1 + Ld.pbase) & 1;           // the parity the single call's last step writes
        Ld.hpack[(size_t)par * nq * 256 + pk_idx(u, 0)] = h;
        if (Tc >= 2) Ld.hpack[(size_t)(par ^ 1) * nq * 256 + pk_idx(u, 0)] = out[((size_t)(Tc - 2) * n + i) * Hs + u];
    }
    const float* x = hb + (size_t)(L - 1) * tcmax * n * Hs;
    const int rows = S.buffering ? Tc : S.keep, t0 = S.buffering ? 0 : Tc - S.keep;
    for (int k = tid; k < rows * Hs; k += nth)
        S.la_buf[k] = x[((size_t)(t0 + k / Hs) * n + i) * Hs + k % Hs];
}

static int many_fail(int code, const std::string& msg) { g_stream_error = msg; return code; }

extern "C" int dsmi_stream_forward_many(dsmi_stream* const* streams, int n, const float* const* feat, const int* T, const int* is_first,
                                        const int* is_last, float* probs, int T_out_cap, int32_t* T_out, void* stream) {
    // ---- refusals: arguments, then every session's protocol and capacity, before any device work or state change
    if (!streams || !feat || !T || !is_first || !is_last || !T_out) return many_fail(DSMI_ERR_INVALID, "null argument array");
    if (n < 1 || n > kMaxMany) return many_fail(DSMI_ERR_INVALID, "n outside 1.." + std::to_string(kMaxMany));
    auto sess_fail = [](int code, int i, const char* msg) { return many_fail(code, "session " + std::to_string(i) + ": " + msg); };
    for (int i = 0; i < n; ++i) {
        if (!streams[i]) return sess_fail(DSMI_ERR_INVALID, i, "null handle");
        if (streams[i]->m != streams[0]->m) return sess_fail(DSMI_ERR_INVALID, i, "a handle of another model than session 0's");
        if (!feat[i] || T[i] < 1) return sess_fail(DSMI_ERR_INVALID, i, "bad chunk (null features or T < 1)");
    }
    for (int j = 1; j < n; ++j)          // n <= 256: the quadratic scan names the repeat, not the first occurrence
        for (int k = 0; k < j; ++k)
            if (streams[k] == streams[j]) return sess_fail(DSMI_ERR_INVALID, j, "the same handle appears twice in one call");
    dsmi_model* m = streams[0]->m;
    const dsmi_model_desc& d = m->desc;
    const int L = d.rnn_layers, Hs = m->Hs, ctx = d.context, C = d.n_labels;
    std::vector<SessDev> sd(n);
    std::vector<StreamPass> pass(n);
    int tin1max = 1, to1max = 1, tin2max = 1, ncatmax = 0, noutmax = 0;
    bool any_out = false;
    for (int i = 0; i < n; ++i) {
        const dsmi_stream* st = streams[i];
        const bool last = is_last[i] != 0;
        StreamPass& p = pass[i];
        const char* why = nullptr;
        const int rc = stream_pass_plan(st->f, T[i], is_first[i] != 0, last, ctx, probs != nullptr, T_out_cap, &p, &why);
        if (rc) return sess_fail(rc, i, why);
        SessDev& S = sd[i];
        S.feat = feat[i]; S.left[0] = st->left[0]; S.left[1] = st->left[1]; S.la_buf = st->la_buf;
        S.T = T[i]; S.ctxl = p.ctxl; S.padl = p.padl; S.is_last = last; S.seed = st->f.has_hidden; S.buffering = p.buffering;
        S.la_rows = p.buffering ? 0 : st->f.la_rows; S.ncat = p.buffering ? 0 : p.ncat; S.keep = p.keep;
        for (int l = 0; l < 2; ++l) { S.tin[l] = p.tin[l]; S.to[l] = p.to[l]; }
        tin1max = std::max(tin1max, p.tin[0]);
        to1max = std::max(to1max, p.to[0]);
        tin2max = std::max(tin2max, p.tin[1]);
        if (!p.buffering) { any_out = true; ncatmax = std::max(ncatmax, p.ncat); noutmax = std::max(noutmax, p.nout); }
    }
    for (int i = 0; i < n; ++i) T_out[i] = 0;

    S_HIP(g_stream_error, hipSetDevice(m->device));
    hipStream_t s = (hipStream_t)stream;
    {
        static std::mutex create_mu;          // two threads' first batched calls on one model
        std::lock_guard<std::mutex> lk(create_mu);
        if (!m->sbatch) m->sbatch = new StreamBatch();
    }
    StreamBatch& b = *m->sbatch;
    std::lock_guard<std::mutex> lk(b.mu);
    // ---- capacity (allocation only; no session's state is touched)
    for (int i = 0; i < n; ++i) {
        if (int rc = grow_la(streams[i], pass[i].buffering ? pass[i].to[1] : pass[i].keep, s, g_stream_error)) return rc;
        sd[i].la_buf = streams[i]->la_buf;
    }
    const int rows0 = kConvSpecs[0].ci * m->conv_fi[0], rows1 = kConvSpecs[1].ci * m->conv_fi[1];
    const int ys1 = round_up(to1max, 4), tcmax = tin2max, ys2 = round_up(tcmax, 4);
    const int nz = ceil_div(n, 32), nq = m->geom.nq, npair = ceil_div(nq, 2);
    const size_t tab_bytes = sizeof(SessDev) * n + sizeof(LayerDev) * (size_t)L * n + sizeof(int32_t) * 2 * n + 64;
    if (tab_bytes > b.tab_host_cap) {
        S_HIP(g_stream_error, hipStreamSynchronize(s));
        if (b.tab_host) (void)hipHostFree(b.tab_host);
        b.tab_host = nullptr; b.tab_host_cap = 0;
        S_HIP(g_stream_error, hipHostMalloc((void**)&b.tab_host, tab_bytes * 2, hipHostMallocDefault));
        b.tab_host_cap = tab_bytes * 2;
    }
    bool ok = grow_dev(b.tab, b.cap[0], tab_bytes) &&
              grow_dev(b.xin[0], b.cap[1], sizeof(float) * (size_t)n * rows0 * tin1max) &&
              grow_dev(b.y[0], b.cap[2], sizeof(float) * (size_t)n * 32 * m->conv_fo[0] * ys1) &&
              grow_dev(b.xin[1], b.cap[3], sizeof(float) * (size_t)n * rows1 * tin2max) &&
              grow_dev(b.y[1], b.cap[4], sizeof(float) * (size_t)n * 32 * m->conv_fo[1] * ys2) &&
              grow_dev(b.xp, b.cap[5], sizeof(float) * (size_t)tcmax * n * m->geom.Np) &&
              grow_dev(b.hb, b.cap[6], sizeof(float) * (size_t)L * tcmax * n * Hs) &&
              grow_dev(b.hseed, b.cap[7], sizeof(float) * (size_t)L * n * Hs) &&
              grow_dev(b.cwork, b.cap[8], sizeof(float) * (size_t)L * n * Hs) &&
              grow_dev(b.hpack, b.cap[9], sizeof(float) * (size_t)L * 2 * nz * nq * 256) &&
              grow_dev(b.cat, b.cap[10], sizeof(float) * (size_t)std::max(ncatmax, 1) * n * Hs) &&
              grow_dev(b.la_out, b.cap[11], sizeof(float) * (size_t)std::max(ncatmax, 1) * n * Hs) &&
              grow_dev(b.probs, b.cap[12], sizeof(float) * (size_t)n * std::max(noutmax, 1) * C) &&
              grow_dev(b.hpack_sp, b.cap[13], (size_t)2 * nz * npair * 2048, true) &&     // the half pair past an odd nq is never written
              grow_dev(b.cnt, b.cap[14], sizeof(unsigned) * (size_t)nz * (tcmax + 1)) &&
              grow_dev(b.err, b.cap[15], sizeof(unsigned) * 4, true);
    if (!ok) return many_fail(DSMI_ERR_NOMEM, "stream_forward_many: HIP allocation failed");

    // ---- the session table: [n] SessDev, [L][n] LayerDev, lens [2][n] (conv1 outputs, then Tc)
    char* th = b.tab_host;
    std::memcpy(th, sd.data(), sizeof(SessDev) * n);
    LayerDev* ldh = reinterpret_cast<LayerDev*>(th + sizeof(SessDev) * n);
    for (int l = 0; l < L; ++l)
        for (int i = 0; i < n; ++i) {
            const dsmi_stream* st = streams[i];
            ldh[(size_t)l * n + i] = LayerDev{st->hpack[l], st->hcarry[l], st->ccarry[l], st->pbase[l], 0};
        }
    int32_t* lh = reinterpret_cast<int32_t*>(th + sizeof(SessDev) * n + sizeof(LayerDev) * (size_t)L * n);
    for (int i = 0; i < n; ++i) { lh[i] = sd[i].to[0]; lh[n + i] = sd[i].to[1]; }
    char* tdev = (char*)b.tab;
    const SessDev* sd_dev = reinterpret_cast<const SessDev*>(tdev);
    const LayerDev* ld_dev = reinterpret_cast<const LayerDev*>(tdev + sizeof(SessDev) * n);
    const int32_t* lens_dev = reinterpret_cast<const int32_t*>(tdev + sizeof(SessDev) * n + sizeof(LayerDev) * (size_t)L * n);
    S_HIP(g_stream_error, hipMemcpyAsync(tdev, th, tab_bytes - 64, hipMemcpyHostToDevice, s));

    // ---- MaskConvStream for all sessions
    const int tinl[2] = {tin1max, tin2max}, toutl[2] = {to1max, tcmax}, ysl[2] = {ys1, ys2}, rowsl[2] = {rows0, rows1};
    for (int l = 0; l < 2; ++l) {
        const int blocks = std::min(ceil_div(rowsl[l] * tinl[l], 256), 256);
        hipLaunchKernelGGL(stream_conv_in_kernel, dim3(blocks, n), dim3(256), 0, s, sd_dev, l, (const float*)b.y[0], ys1, rowsl[l], tinl[l], b.xin[l]);
        launch_conv(conv_launch(m, l, n, b.xin[l], b.y[l], lens_dev + l * n, tinl[l], toutl[l], ysl[l]), s);
    }

    // ---- recurrent layers (attempt 0 may use the persistent kernel; attempt 1 recomputes a timed-out pass per step), lookahead, head
    S_HIP(g_stream_error, hipMemsetAsync(b.err, 0, sizeof(unsigned), s));
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool persisted = false;
        const int sblocks = std::min(ceil_div(nz * 32 * Hs, 256), 512);
        hipLaunchKernelGGL(stream_seed_kernel, dim3(sblocks, L), dim3(256), 0, s, sd_dev, ld_dev, n, Hs, nq, nz, b.hseed, b.cwork, b.hpack);
        for (int l = 0; l < L; ++l) {
            const RnnW& r = m->rnn[l];
            float* out = b.hb + (size_t)l * tcmax * n * Hs;
            launch_gemm(xproj_launch(m, l, n, tcmax, l == 0 ? b.y[1] : out - (size_t)tcmax * n * Hs, ys2, b.xp), s);
            if (Hs != d.rnn_hidden_size) S_HIP(g_stream_error, hipMemsetAsync(out, 0, sizeof(float) * (size_t)tcmax * n * Hs, s));
            float* h0 = b.hseed + (size_t)l * n * Hs;
            float* cw = b.cwork + (size_t)l * n * Hs;
            bool done = false;
            if (attempt == 0 && m->rnn_mode == 1 && r.whh_sp[0] && rnn_persist_eligible(m->geom, n, m->n_cus)) {
                RnnPersistLaunch pl = persist_launch(m, l, n, tcmax, 0);      // geometry, weights, test hooks; the pass has buffers of its own:
                pl.whh_sp[1] = nullptr; pl.bhh[1] = nullptr; pl.out[0] = out; pl.out[1] = nullptr;
                pl.xp = b.xp; pl.lens_dev = lens_dev + n; pl.hpack_sp = b.hpack_sp; pl.counters = b.cnt; pl.err = b.err;
                pl.h0 = h0; pl.cst = cw;
                S_HIP(g_stream_error, hipMemsetAsync(b.cnt, 0, sizeof(unsigned) * (size_t)nz * (tcmax + 1), s));
                done = stream_persist_layer(m, pl, s);
                persisted = persisted || done;
            }
            if (!done) {
                float* hp = b.hpack + (size_t)l * 2 * nz * nq * 256;
                RnnStepLaunch sl = step_launch(m, l, n, tcmax, b.xp, lens_dev + n, out, cw, hp, h0, 0);
                for (int step = 0; step < tcmax; ++step) { sl.step = step; launch_rnn_step(sl, s); }
            }
            record_stream_plan(m, done);
        }
        if (any_out) {
            const float* x = b.hb + (size_t)(L - 1) * tcmax * n * Hs;
            const size_t items = (size_t)ncatmax * n * Hs;
            hipLaunchKernelGGL(stream_cat_kernel, dim3((unsigned)std::min<size_t>((items + 255) / 256, 2048)), dim3(256), 0, s,
                               sd_dev, x, n, Hs, ncatmax, b.cat);
            launch_lookahead(b.cat, m->look_w, b.la_out, ncatmax, n, d.rnn_hidden_size, ctx, s);
            launch_head(head_launch(m, n, noutmax, b.la_out, b.probs), s);
        }
        S_HIP(g_stream_error, hipGetLastError());
        if (!persisted) break;
        unsigned e = 0;
        S_HIP(g_stream_error, hipMemcpyAsync(&e, b.err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        S_HIP(g_stream_error, hipStreamSynchronize(s));
        if (!e) break;
        // a hand-off wait timed out: the pass is recomputed on the per-step path from the same seeded state, and this model
        // stays there (as dsmi_rnn_layer does)
        S_HIP(g_stream_error, hipMemsetAsync(b.err, 0, sizeof(unsigned), s));
        m->rnn_mode = 0;
        m->recomputed += 1;
    }
    if (any_out)
        S_HIP(g_stream_error, hipMemcpy2DAsync(probs, sizeof(float) * (size_t)T_out_cap * C, b.probs, sizeof(float) * (size_t)noutmax * C,
                               sizeof(float) * (size_t)noutmax * C, n, hipMemcpyDeviceToDevice, s));

    // ---- commit every session's new state
    hipLaunchKernelGGL(stream_commit_kernel, dim3(16, n), dim3(256), 0, s, sd_dev, ld_dev, n, L, Hs, nq, (const float*)b.xin[0], rows0,
                       tin1max, (const float*)b.xin[1], rows1, tin2max, (const float*)b.hb, tcmax, (const float*)b.cwork);
    S_HIP(g_stream_error, hipGetLastError());
    S_HIP(g_stream_error, hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        stream_pass_commit(streams[i]->f, streams[i]->pbase.data(), L, pass[i], is_last[i] != 0);
        T_out[i] = pass[i].nout;
    }
    return DSMI_OK;
}
