// Handle lifecycle of dsmi_model (include/dsmi.h): creation, weight repacking (dsmi_model_finalize), workspace sizing (dsmi_reserve)
// and the frame arithmetic of the conv stack.  Host code only.
#include "common.h"
#include "model.h"
#include "gate.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace dsmi;

static thread_local std::string g_create_error;

constexpr float kF16Safe = 60000.f;    // below fp16's 65504 with room for rounding

// ------------------------------------------------------------------------------------------
extern "C" int dsmi_model_create(const dsmi_model_desc* d, int device, dsmi_model** out) {
    if (!d || !out) { g_create_error = "null argument"; return DSMI_ERR_INVALID; }
    // reference model.py:344-348
    if (d->conv_layers == 0) { g_create_error = "0 convolutional layers configuration not supported by DanSpeech"; return DSMI_ERR_CONV; }
    if (d->conv_layers > 3 || d->conv_layers < 0) { g_create_error = "Maximum amount of convolutional layers supported by DanSpeech is 3"; return DSMI_ERR_CONV; }
    if (d->rnn_type < 0 || d->rnn_type > 2 || d->rnn_hidden_size < 1 || d->rnn_layers < 1 || d->n_labels < 1 ||
        d->n_labels > 128 || (!d->bidirectional && d->context < 1)) {
        g_create_error = "invalid model description";
        return DSMI_ERR_INVALID;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        g_create_error = "no such HIP device";
        return DSMI_ERR_HIP;
    }
    dsmi_model* m = new dsmi_model();
    m->desc = *d;
    m->device = device;
    m->n_fft = (int)(d->sample_rate * d->window_size);      // model.py:354: int(floor(rate * size / 2) + 1) below
    m->n_freq = m->n_fft / 2 + 1;                            // model.py:354
    int f = m->n_freq;
    for (int l = 0; l < d->conv_layers; ++l) {
        const ConvSpec& s = kConvSpecs[l];
        m->conv_fi[l] = f;
        f = (f + 2 * s.pf - s.kf) / s.sf + 1;
        m->conv_fo[l] = f;
    }
    m->I0 = kConvSpecs[d->conv_layers - 1].co * f;           // model.py:365,379,396
    m->geom = make_rnn_geom(d->rnn_type, d->rnn_hidden_size, d->bidirectional ? 2 : 1);
    m->Hs = m->geom.Kp;
    m->geom16 = make_rnn_geom_u(d->rnn_type, d->rnn_hidden_size, d->bidirectional ? 2 : 1, 16);
    m->have16 = d->rnn_hidden_size % 16 == 0;
    m->rnn.resize(d->rnn_layers);
    {
        hipDeviceProp_t prop;
        m->n_cus = hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.multiProcessorCount : 0;
        // DSMI_DENSE_TILES / DSMI_CONV_TILES: read once per process, when its first model is made, like DSMI_DENSE_TOKENS
        static const TileSwitches tiles = tile_switches(std::getenv("DSMI_DENSE_TILES"), std::getenv("DSMI_CONV_TILES"), dense_token_limit() > 0);
        m->dense_tiles = tiles.gemm;
        m->conv_tiles = tiles.convs;
        const char* mode = std::getenv("DSMI_RNN_MODE");      // "steps": one launch per time step; "persist8": first-generation persistent kernel
        m->rnn_mode = (mode && std::string(mode) == "steps") ? 0 : 1;
        m->persist_gen = (mode && std::string(mode) == "persist8") ? 1 : 2;
        // DSMI_RNN_KERNEL=duo: the paired-tile / tile-walking kernels where the ring kernel would run (A/B measurements and the
        // parity tests of those kernels); =ring: the ring kernel also for a lone batch of up to 32 clips
        const char* rk = std::getenv("DSMI_RNN_KERNEL");
        m->rnn_kernel = (rk && std::string(rk) == "duo") ? 1 : ((rk && std::string(rk) == "ring") ? 2 : 0);
        m->ring8 = rk && std::string(rk) == "ring8";      // the eight-wave form of the ring kernel everywhere (A/B runs)
        m->ring4 = rk && std::string(rk) == "ring4";      // the four-wave form everywhere (also for windows of one or two tiles)
        // DSMI_DENSE_MODE=f32: GEMM and conv layers on the plain fp32-MFMA kernels (the round-1 path, and where a model whose
        // weights leave fp16's range ends up by itself); with DSMI_RNN_MODE=steps the whole forward is the second, independent
        // implementation the parity tests compare the default one with
        const char* dm = std::getenv("DSMI_DENSE_MODE");
        const bool dense_f32 = dm && std::string(dm) == "f32";
        m->gemm_mode = dense_f32 ? 0 : 1;
        m->conv_mode = dense_f32 ? 0 : 1;
        m->conv1_split = !dense_f32;
        // test hooks for the hand-off timeout path (tests/test_gpu_timeout.py)
        if (const char* sl = std::getenv("DSMI_DEBUG_SPIN_LIMIT")) m->spin_limit = (unsigned)std::max(1L, std::atol(sl));
        if (const char* ds = std::getenv("DSMI_DEBUG_DROP_SIGNAL"))
            if (std::sscanf(ds, "%d:%d:%d", &m->drop_layer, &m->drop_wg, &m->drop_step) != 3) m->drop_layer = -1;
        m->lane = persist_next_lane(device);
        if (m->rnn_mode == 1 && !persist_process_lock(device)) {
            m->rnn_mode = 0;
            m->err = "another process holds this GPU's persistent-kernel lock: recurrent layers run one launch per step";
        }
    }
    *out = m;
    return DSMI_OK;
}

extern "C" const char* dsmi_last_error(const dsmi_model* m) { return m ? m->err.c_str() : g_create_error.c_str(); }

extern "C" int dsmi_model_info(const dsmi_model* m, dsmi_model_desc* desc, int* device) {
    if (!m) return DSMI_ERR_INVALID;
    if (desc) *desc = m->desc;
    if (device) *device = m->device;
    return DSMI_OK;
}

extern "C" int dsmi_model_load_tensor(dsmi_model* m, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!m || !name || !data || ndim < 0 || ndim > 4) return m ? fail(m, DSMI_ERR_INVALID, "bad tensor argument") : DSMI_ERR_INVALID;
    if (m->finalized) return fail(m, DSMI_ERR_INVALID, "model already finalized");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(data, data + n);
    // LookaheadStream is a direct attribute of a streaming model (model.py:490), the first module of a
    // Sequential otherwise (model.py:407-411): one weight, two names
    const std::string key = std::string(name) == "lookahead.conv.weight" ? "lookahead.0.conv.weight" : name;
    m->tensors[key] = std::move(t);
    return DSMI_OK;
}

static const HostTensor* need(dsmi_model* m, const std::string& name, std::initializer_list<int64_t> shape) {
    auto it = m->tensors.find(name);
    if (it == m->tensors.end()) { m->err = "missing tensor " + name; return nullptr; }
    if (it->second.shape != std::vector<int64_t>(shape)) { m->err = "bad shape for tensor " + name; return nullptr; }
    return &it->second;
}

template <typename T>
static int upload(dsmi_model* m, const std::vector<T>& h, T** dev) {
    HIP_OK(m, hipMalloc((void**)dev, std::max<size_t>(h.size(), 1) * sizeof(T)));
    m->owned.push_back(*dev);
    if (!h.empty()) HIP_OK(m, hipMemcpy(*dev, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return DSMI_OK;
}

// eval-mode BatchNorm as y = x*a + b, computed as ATen's CPU kernel does:
// invstd = 1/sqrt(var+eps); a = weight*invstd; b = bias - mean*a.
static bool bn_affine(dsmi_model* m, const std::string& prefix, int n, int n_pad, std::vector<float>& a, std::vector<float>& b) {
    const HostTensor *w = need(m, prefix + ".weight", {n}), *bi = need(m, prefix + ".bias", {n}),
                     *mu = need(m, prefix + ".running_mean", {n}), *var = need(m, prefix + ".running_var", {n});
    if (!w || !bi || !mu || !var) return false;
    a.assign(n_pad, 0.f); b.assign(n_pad, 0.f);
    for (int i = 0; i < n; ++i) {
        const float invstd = 1.f / std::sqrt(var->data[i] + 1e-5f);
        a[i] = w->data[i] * invstd;
        b[i] = bi->data[i] - mu->data[i] * a[i];
    }
    return true;
}

extern "C" int dsmi_model_finalize(dsmi_model* m) {
    if (!m) return DSMI_ERR_INVALID;
    if (m->finalized) return DSMI_OK;
    HIP_OK(m, hipSetDevice(m->device));
    const dsmi_model_desc& d = m->desc;
    const RnnGeom& g = m->geom;
    const int H = d.rnn_hidden_size, G = g.G;
    // ---- conv stack
    for (int l = 0; l < d.conv_layers; ++l) {
        const ConvSpec& s = kConvSpecs[l];
        const std::string p = "conv.seq_module." + std::to_string(3 * l);
        const HostTensor* w = need(m, p + ".weight", {s.co, s.ci, s.kf, s.kt});
        const HostTensor* b = need(m, p + ".bias", {s.co});
        std::vector<float> a, bb;
        if (!w || !b || !bn_affine(m, "conv.seq_module." + std::to_string(3 * l + 1), s.co, s.co, a, bb)) return DSMI_ERR_NOT_READY;
        int rc;
        if ((rc = upload(m, pack_conv_weights(w->data.data(), l), &m->conv[l].wp))) return rc;
        for (float v : w->data) if (!(std::fabs(v) < kF16Safe / 64.f)) m->conv_mode = 0;    // split-fp16 operand range (packed times 2^6: conv_split.hip)
        if (l > 0) {
            if ((rc = upload(m, pack_conv_w_split(w->data.data(), s.co), &m->conv[l].wp_sp))) return rc;
        } else {
            if ((rc = upload(m, pack_conv1_w_split(w->data.data()), &m->conv[l].wp_sp))) return rc;
        }
        if ((rc = upload(m, b->data, &m->conv[l].bias))) return rc;
        if ((rc = upload(m, a, &m->conv[l].bn_a))) return rc;
        if ((rc = upload(m, bb, &m->conv[l].bn_b))) return rc;
    }
    // ---- recurrent layers
    for (int l = 0; l < d.rnn_layers; ++l) {
        RnnW& r = m->rnn[l];
        const int I = l == 0 ? m->I0 : H;
        r.K = l == 0 ? I : m->Hs;
        r.ldw = round_up(r.K, 4);
        std::vector<float> wih((size_t)g.Np * r.ldw, 0.f), bih(g.Np, 0.f);
        const std::string p = "rnns." + std::to_string(l) + ".rnn.";
        const HostTensor *wi[2], *wh[2], *bi[2], *bh[2];
        for (int dd = 0; dd < g.D; ++dd) {
            const std::string sfx = dd ? "_reverse" : "";
            wi[dd] = need(m, p + "weight_ih_l0" + sfx, {G * H, I});
            wh[dd] = need(m, p + "weight_hh_l0" + sfx, {G * H, H});
            bi[dd] = need(m, p + "bias_ih_l0" + sfx, {G * H});
            bh[dd] = need(m, p + "bias_hh_l0" + sfx, {G * H});
            if (!wi[dd] || !wh[dd] || !bi[dd] || !bh[dd]) return DSMI_ERR_NOT_READY;
        }
        for (int col = 0; col < g.Np; ++col) {
            int dd;
            const int src = rnn_src_row(g, col, &dd);
            if (src < 0) continue;
            std::memcpy(&wih[(size_t)col * r.ldw], &wi[dd]->data[(size_t)src * I], sizeof(float) * I);
            bih[col] = bi[dd]->data[src];
        }
        int rc;
        for (float v : wih) if (!(std::fabs(v) < kF16Safe / 64.f)) m->gemm_mode = 0;     // split-fp16 operand range (packed times 2^6: gemm.hip)
        if ((rc = upload(m, wih, &r.wih))) return rc;
        if ((rc = upload(m, pack_gemm_w_split(wih.data(), g.Np, r.K, r.ldw), &r.wih_sp))) return rc;
        if ((rc = upload(m, bih, &r.bih))) return rc;
        for (int dd = 0; dd < g.D; ++dd) {
            // the split-fp16 operands hold |x| < 65504 only: a model beyond that stays on the fp32 kernels
            for (float v : wh[dd]->data) if (!(std::fabs(v) < kF16Safe)) m->rnn_mode = 0;
            if ((rc = upload(m, pack_whh(g, wh[dd]->data.data()), &r.whh[dd]))) return rc;
            if ((rc = upload(m, pack_whh_split(g, wh[dd]->data.data()), &r.whh_sp[dd]))) return rc;
            if ((rc = upload(m, bh[dd]->data, &r.bhh[dd]))) return rc;
        }
        if (m->have16) {
            const RnnGeom& g16 = m->geom16;
            std::vector<float> w16((size_t)g16.Np * r.ldw, 0.f), b16(g16.Np, 0.f);
            for (int col = 0; col < g16.Np; ++col) {
                int dd;
                const int src = rnn_src_row(g16, col, &dd);
                if (src < 0) continue;
                std::memcpy(&w16[(size_t)col * r.ldw], &wi[dd]->data[(size_t)src * I], sizeof(float) * I);
                b16[col] = bi[dd]->data[src];
            }
            if ((rc = upload(m, pack_gemm_w_split(w16.data(), g16.Np, r.K, r.ldw), &r.wih16_sp))) return rc;
            if ((rc = upload(m, b16, &r.bih16))) return rc;
            for (int dd = 0; dd < g.D; ++dd)
                if ((rc = upload(m, pack_whh16(g16, wh[dd]->data.data()), &r.whh16_sp[dd]))) return rc;
        }
        if (l > 0) {  // model.py:403-404: BatchNorm1d(H) in front of layers >= 1
            std::vector<float> a, b;
            if (!bn_affine(m, "rnns." + std::to_string(l) + ".batch_norm.module", H, m->Hs, a, b)) return DSMI_ERR_NOT_READY;
            // the GEMM's A operand is (h_fwd + h_bwd) * a + b with |h| <= 1: bounded by 2|a| + |b|
            for (size_t k = 0; k < a.size(); ++k) if (!(2.f * std::fabs(a[k]) + std::fabs(b[k]) < kF16Safe)) m->gemm_mode = 0;
            if ((rc = upload(m, a, &r.bn_a))) return rc;
            if ((rc = upload(m, b, &r.bn_b))) return rc;
        }
    }
    int rc;
    if (!d.bidirectional) {
        const HostTensor* lw = need(m, "lookahead.0.conv.weight", {H, 1, d.context});
        if (!lw) return DSMI_ERR_NOT_READY;
        if ((rc = upload(m, lw->data, &m->look_w))) return rc;
    }
    {
        std::vector<float> a, b;
        const HostTensor* fw = need(m, "fc.0.module.1.weight", {d.n_labels, H});
        if (!fw || !bn_affine(m, "fc.0.module.0", H, m->Hs, a, b)) return DSMI_ERR_NOT_READY;
        if ((rc = upload(m, a, &m->fc_a))) return rc;
        if ((rc = upload(m, b, &m->fc_b))) return rc;
        if ((rc = upload(m, pack_fc(fw->data.data(), d.n_labels, H), &m->fc_wp))) return rc;
    }
    m->tensors.clear();
    for (int i = 0; i < 8; ++i) HIP_OK(m, hipEventCreate(&m->ev[i]));
    // every slot of the forward-status ring now, not on the first four forwards (a pinned allocation can take ~100 ms)
    for (auto& f : m->fwd) {
        if (f.done) continue;
        HIP_OK(m, hipEventCreateWithFlags(&f.done, hipEventDisableTiming));
        HIP_OK(m, hipHostMalloc((void**)&f.err_host, sizeof(unsigned), hipHostMallocDefault));
        *f.err_host = 0;
    }
    m->finalized = true;
    return DSMI_OK;
}

int seq_len(const dsmi_model* m, int L) {  // model.py:540-551
    for (int l = 0; l < m->desc.conv_layers; ++l) {
        const ConvSpec& s = kConvSpecs[l];
        L = (L + 2 * s.pt - (s.kt - 1) - 1) / s.st + 1;
    }
    return L;
}

// The fewest input frames whose seq_len is To: only the first conv layer strides in time, by 2 ((L - 1) / 2 + 1).
int frames_for(int To) { return 2 * To - 1; }

extern "C" int dsmi_seq_lens(const dsmi_model* m, const int32_t* lens, int n, int32_t* out) {
    if (!m || !lens || !out) return DSMI_ERR_INVALID;
    for (int i = 0; i < n; ++i) out[i] = seq_len(m, lens[i]);
    return DSMI_OK;
}

static void free_ws(dsmi_model* m) {
    for (void* p : m->ws) (void)hipFree(p);
    m->ws.clear();
    m->cap_B = m->cap_T = 0;
}

template <typename T>
static int ws_alloc(dsmi_model* m, T** p, size_t n) {
    HIP_OK(m, hipMalloc((void**)p, std::max<size_t>(n, 1) * sizeof(T)));
    m->ws.push_back(*p);
    return DSMI_OK;
}

extern "C" int dsmi_reserve(dsmi_model* m, int max_B, int max_T) {
    if (!m || max_B < 1 || max_T < 1) return m ? fail(m, DSMI_ERR_INVALID, "bad reserve size") : DSMI_ERR_INVALID;
    if (!m->finalized) return fail(m, DSMI_ERR_NOT_READY, "dsmi_model_finalize has not been called");
    if (max_B <= m->cap_B && max_T <= m->cap_T) return DSMI_OK;
    HIP_OK(m, hipSetDevice(m->device));
    HIP_OK(m, hipDeviceSynchronize());
    max_B = std::max(max_B, m->cap_B);
    max_T = std::max(max_T, m->cap_T);
    free_ws(m);
    const dsmi_model_desc& d = m->desc;
    const int To = seq_len(m, max_T);
    const int ys = round_up(std::max(To, 1), 4);
    size_t conv_max = 0;
    for (int l = 0; l < d.conv_layers; ++l)
        conv_max = std::max(conv_max, (size_t)max_B * kConvSpecs[l].co * m->conv_fo[l] * ys);
    int rc;
    if ((rc = ws_alloc(m, &m->conv_buf[0], conv_max))) return rc;
    if ((rc = ws_alloc(m, &m->conv_buf[1], d.conv_layers > 1 ? conv_max : 1))) return rc;
    for (int i = 0; i < 2; ++i) {   // split intermediates: layer 0 -> buf3[0], layer 1 -> buf3[1] (3-conv models)
        const size_t n = i < d.conv_layers - 1 ? (size_t)max_B * m->conv_fo[i] * 2 * std::max(To, 1) * 32 : 1;
        if ((rc = ws_alloc(m, &m->conv_buf_sp[i], n))) return rc;
    }
    const size_t rows = (size_t)To * max_B;
    if ((rc = ws_alloc(m, &m->xp, rows * std::max(m->geom.Np, m->have16 ? m->geom16.Np : 0)))) return rc;
    for (int i = 0; i < 2; ++i)
        for (int dd = 0; dd < 2; ++dd) {
            m->hbuf[i][dd] = nullptr;
            if (dd < m->geom.D && (rc = ws_alloc(m, &m->hbuf[i][dd], rows * m->Hs))) return rc;
        }
    for (int dd = 0; dd < 2; ++dd) {
        m->cst[dd] = nullptr;
        if (d.rnn_type == DSMI_RNN_LSTM && dd < m->geom.D && (rc = ws_alloc(m, &m->cst[dd], (size_t)max_B * m->Hs))) return rc;
    }
    {
        // zero once: operand slots of padding units (k in [H, Hs)) are never written and must stay finite
        const size_t n = (size_t)2 * m->geom.D * ceil_div(max_B, 32) * m->geom.nq * 256;
        if ((rc = ws_alloc(m, &m->hpack, n))) return rc;
        HIP_OK(m, hipMemset(m->hpack, 0, n * sizeof(float)));
    }
    {
        const size_t n = (size_t)2 * m->geom.D * ceil_div(max_B, 32) * ceil_div(m->geom.nq, 2) * 2 * 64 * 8;
        if ((rc = ws_alloc(m, &m->hpack_sp, n))) return rc;
        HIP_OK(m, hipMemset(m->hpack_sp, 0, n * sizeof(uint16_t)));
    }
    {
        const size_t mt = (size_t)max_B * ceil_div(std::max(To, 1), 128) + ceil_div((int)rows, 128) + 1;
        const size_t kt = (size_t)ceil_div(std::max(m->I0, m->Hs), 32);
        if ((rc = ws_alloc(m, &m->a_sp, mt * kt * 2 * 4096))) return rc;
        const size_t cnt_words = (size_t)dsmi_model::kTileCntBlocks * kDenseCntWords;
        if ((rc = ws_alloc(m, &m->tile_cnt, cnt_words))) return rc;
        HIP_OK(m, hipMemset(m->tile_cnt, 0, cnt_words * sizeof(unsigned)));
    }
    if (m->have16) {
        const size_t n = rnn_persist16_state_halfs(m->geom16, max_B);
        if ((rc = ws_alloc(m, &m->hpack16, n))) return rc;
        HIP_OK(m, hipMemset(m->hpack16, 0, n * sizeof(uint16_t)));
    }
    // (+ the ring kernel's direction tickets behind the counters: two words per window, zeroed by the same memset)
    if ((rc = ws_alloc(m, &m->pcnt, persist_cnt_words(m, max_B, std::max(To, 1), true, true)))) return rc;
    if ((rc = ws_alloc(m, &m->perr, (size_t)4))) return rc;
    HIP_OK(m, hipMemset(m->perr, 0, 4 * sizeof(unsigned)));
    m->look_buf = nullptr;
    if (!d.bidirectional && (rc = ws_alloc(m, &m->look_buf, rows * m->Hs))) return rc;
    if ((rc = ws_alloc(m, &m->xin, rows * round_up(std::max(m->I0, m->Hs), 4)))) return rc;
    if ((rc = ws_alloc(m, &m->lens_dev, (size_t)max_B))) return rc;
    m->cap_B = max_B;
    m->cap_T = max_T;
    return DSMI_OK;
}

extern "C" void dsmi_model_destroy(dsmi_model* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    (void)hipDeviceSynchronize();
    free_ws(m);
    for (void* p : m->owned) (void)hipFree(p);
    if (m->finalized)
        for (int i = 0; i < 8; ++i) (void)hipEventDestroy(m->ev[i]);
    timer_resolve(m);
    for (auto& f : m->fwd) {
        if (f.err_host) (void)hipHostFree(f.err_host);
        if (f.done) (void)hipEventDestroy(f.done);
    }
    if (m->lens_stage) (void)hipHostFree(m->lens_stage);
    for (hipEvent_t e : m->stage_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : m->kt.free_events) (void)hipEventDestroy(e);
    stream_batch_free(m);
    delete m;
}
