// The streaming phrase watch's handles (include/dsmi.h): dsmi_spot_watch, a phrase list packed and uploaded once, and
// dsmi_spot_stream, one live utterance's carried search (the kernel: spot_stream.hip).  dsmi_spot_stream_advance_many hands
// every number and array to spot_stream_check (ctc_host.h) -- a refusal comes before any launch, before any state changes and
// before any output write -- then grows the watch's workspaces, uploads one table of descriptors, launches once and copies
// the events (and the tracks, when asked for) back.  dsmi_spot_watch_pick is the picking rule alone, on the host (spot_pick.h).
#include "decoder.h"
#include "spot_stream.h"

#include <cmath>
#include <cstring>

using namespace dsmi;

struct dsmi_spot_watch {
    dsmi_decoder* d = nullptr;
    int device = 0, C = 0, K = 0, n_groups = 0, settle = 1;
    float min_mean_logp = 0.f;
    int32_t* words = nullptr;           // device [n_groups][kSpotThreads]
    std::string err;
    // one call at a time: the descriptor table and the events of a launch (io), the tracks 2 x [n][K][F_stride] words (tr)
    std::mutex mu;
    DevBuf io, tr;
};

struct dsmi_spot_stream {
    dsmi_spot_watch* w = nullptr;
    int64_t frames = 0;                 // frames consumed since the utterance began
    unsigned char* state = nullptr;     // score [n_groups][kSpotThreads], start [n_groups][kSpotThreads], pick [K]
    std::string err;
};

static thread_local std::string g_sw_error;

#define SW_HIP(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) { g_sw_error = std::string(#expr) + ": " + hipGetErrorString(e_); return DSMI_ERR_HIP; } \
    } while (0)

extern "C" int dsmi_spot_watch_create(dsmi_decoder* d, const int32_t* phrases, const int32_t* phrase_lens, int K, int L_stride,
                                      float min_mean_logp, int settle_frames, dsmi_spot_watch** out) {
    if (!d || !out || !phrases || !phrase_lens) { g_sw_error = "bad spot watch arguments"; return DSMI_ERR_INVALID; }
    const int C = (int)d->labels.size();
    if (int rc = spot_watch_check(phrases, phrase_lens, K, L_stride, min_mean_logp, settle_frames, C, d->blank, g_sw_error)) return rc;
    std::vector<int32_t> group_of(K), first_state(K);
    const int n_groups = spot_plan(phrase_lens, K, group_of.data(), first_state.data());
    std::vector<int32_t> words((size_t)n_groups * kSpotThreads, 0);
    spot_pack(phrases, phrase_lens, K, L_stride, d->blank, group_of.data(), first_state.data(), words.data());
    SW_HIP(hipSetDevice(d->device));
    dsmi_spot_watch* w = new dsmi_spot_watch();
    w->d = d; w->device = d->device; w->C = C; w->K = K; w->n_groups = n_groups; w->settle = settle_frames; w->min_mean_logp = min_mean_logp;
    if (hipMalloc((void**)&w->words, sizeof(int32_t) * words.size()) != hipSuccess ||
        hipMemcpy(w->words, words.data(), sizeof(int32_t) * words.size(), hipMemcpyHostToDevice) != hipSuccess) {
        dsmi_spot_watch_destroy(w);
        g_sw_error = "spot watch: HIP allocation or upload failed"; return DSMI_ERR_NOMEM;
    }
    *out = w;
    return DSMI_OK;
}

extern "C" void dsmi_spot_watch_destroy(dsmi_spot_watch* w) {
    if (!w) return;
    (void)hipSetDevice(w->device);
    (void)hipDeviceSynchronize();
    if (w->words) (void)hipFree(w->words);
    w->io.release(); w->tr.release();
    delete w;
}

extern "C" const char* dsmi_spot_watch_last_error(const dsmi_spot_watch* w) { return w ? w->err.c_str() : g_sw_error.c_str(); }

extern "C" int dsmi_spot_watch_info(const dsmi_spot_watch* w, int* K, int* n_groups, int* settle_frames) {
    if (!w) return DSMI_ERR_INVALID;
    if (K) *K = w->K;
    if (n_groups) *n_groups = w->n_groups;
    if (settle_frames) *settle_frames = w->settle;
    return DSMI_OK;
}

static size_t state_bytes(const dsmi_spot_watch* w) { return (size_t)w->n_groups * kSpotThreads * 8 + sizeof(SpotPick) * (size_t)w->K; }

extern "C" int dsmi_spot_stream_create(dsmi_spot_watch* w, dsmi_spot_stream** out) {
    if (!w || !out) { g_sw_error = "bad spot stream arguments"; return DSMI_ERR_INVALID; }
    SW_HIP(hipSetDevice(w->device));
    dsmi_spot_stream* s = new dsmi_spot_stream();
    s->w = w;
    if (hipMalloc((void**)&s->state, state_bytes(w)) != hipSuccess) {
        delete s;
        g_sw_error = "spot stream: HIP allocation failed"; return DSMI_ERR_NOMEM;
    }
    *out = s;
    return DSMI_OK;
}

extern "C" void dsmi_spot_stream_destroy(dsmi_spot_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->w->device);
    (void)hipDeviceSynchronize();
    if (s->state) (void)hipFree(s->state);
    delete s;
}

extern "C" const char* dsmi_spot_stream_last_error(const dsmi_spot_stream* s) { return s ? s->err.c_str() : g_sw_error.c_str(); }

extern "C" int dsmi_spot_stream_reset(dsmi_spot_stream* s) {
    if (!s) return DSMI_ERR_INVALID;
    s->frames = 0;        // the next advance starts at t0 = 0: nothing of the state block is read
    return DSMI_OK;
}

extern "C" int dsmi_spot_stream_frames(const dsmi_spot_stream* s, int64_t* frames) {
    if (!s || !frames) return DSMI_ERR_INVALID;
    *frames = s->frames;
    return DSMI_OK;
}

extern "C" int dsmi_spot_stream_advance_many(dsmi_spot_stream* const* ss, int n, const float* const* probs_dev, const int32_t* frames,
                                             const int32_t* flush, int max_events, int32_t* hits, float* scores, int32_t* fired,
                                             int32_t* counts, float* track_scores, int32_t* track_starts, int F_stride, void* stream) {
    // ---- refusals, before any state changes
    if (!ss || !frames || !flush || !hits || !scores || !fired || !counts || n < 1 || n > DSMI_SPOT_STREAM_MANY_MAX) {
        g_sw_error = "bad spot stream arguments"; return DSMI_ERR_INVALID;
    }
    std::vector<const void*> handles(n), watch_of(n);
    std::vector<int64_t> consumed(n);
    for (int i = 0; i < n; ++i) {
        if (!ss[i]) { g_sw_error = "spot stream " + std::to_string(i) + ": null handle"; return DSMI_ERR_INVALID; }
        handles[i] = ss[i]; watch_of[i] = ss[i]->w; consumed[i] = ss[i]->frames;
    }
    dsmi_spot_watch* w = ss[0]->w;
    const bool tracks = track_scores || track_starts;
    if (int rc = spot_stream_check(handles.data(), watch_of.data(), consumed.data(), n, probs_dev, frames, w->K, max_events, tracks, F_stride,
                                   g_sw_error)) return rc;
    std::lock_guard<std::mutex> lock(w->mu);
    SW_HIP(hipSetDevice(w->device));
    hipStream_t st = (hipStream_t)stream;
    // ---- workspaces: io = the descriptors [n], then hits [n][K][M][2], scores [n][K][M], fired [n][K][M], counts [n][K]
    const int K = w->K, M = max_events;
    const size_t nK = (size_t)n * K, nKM = nK * M, out_words = 4 * nKM + nK, n_tr = tracks ? nK * F_stride : 0;
    const size_t tab_bytes = (sizeof(SpotStreamDesc) * (size_t)n + 255) & ~(size_t)255;
    const size_t io_bytes = tab_bytes + sizeof(int32_t) * out_words, tr_bytes = sizeof(int32_t) * 2 * n_tr;
    if (!w->io.holds(io_bytes) || !w->tr.holds(tr_bytes)) {
        SW_HIP(hipDeviceSynchronize());      // (a launch in flight may still read a buffer that is about to be freed)
        SW_HIP(w->io.reserve(io_bytes));
        SW_HIP(w->tr.reserve(tr_bytes));
    }
    std::vector<SpotStreamDesc> tab(n);
    const size_t rows = (size_t)w->n_groups * kSpotThreads;
    for (int i = 0; i < n; ++i) {
        SpotStreamDesc& q = tab[i];
        q.probs = frames[i] > 0 ? probs_dev[i] : nullptr;
        q.score = reinterpret_cast<float*>(ss[i]->state);
        q.start = reinterpret_cast<int32_t*>(ss[i]->state) + rows;
        q.pick = reinterpret_cast<SpotPick*>(ss[i]->state + rows * 8);
        q.T = frames[i]; q.t0 = (int32_t)ss[i]->frames; q.flush = flush[i] ? 1 : 0; q.pad = 0;
    }
    unsigned char* io = w->io.as<unsigned char>();
    SW_HIP(hipMemcpyAsync(io, tab.data(), sizeof(SpotStreamDesc) * (size_t)n, hipMemcpyHostToDevice, st));
    SpotStreamArgs a{};
    a.desc = reinterpret_cast<const SpotStreamDesc*>(io); a.words = w->words;
    a.C = w->C; a.K = K; a.n_groups = w->n_groups; a.max_events = M; a.settle = w->settle; a.F_stride = F_stride;
    a.min_mean_logp = w->min_mean_logp;
    a.hits = reinterpret_cast<int32_t*>(io + tab_bytes); a.scores = reinterpret_cast<float*>(a.hits + 2 * nKM);
    a.fired = a.hits + 3 * nKM; a.counts = a.hits + 4 * nKM;
    a.E = tracks ? w->tr.as<float>() : nullptr; a.ST = tracks ? w->tr.as<int32_t>() + n_tr : nullptr;
    SW_HIP(launch_spot_stream(a, n, st));
    // ---- from here on the handles change: the launch is in the stream
    for (int i = 0; i < n; ++i) ss[i]->frames += frames[i];
    // the events come back into an image of the call's own and reach the caller's arrays only when everything has succeeded
    std::vector<int32_t> out(out_words);
    SW_HIP(hipMemcpyAsync(out.data(), a.hits, sizeof(int32_t) * out_words, hipMemcpyDeviceToHost, st));
    if (track_scores && n_tr) SW_HIP(hipMemcpyAsync(track_scores, a.E, sizeof(float) * n_tr, hipMemcpyDeviceToHost, st));
    if (track_starts && n_tr) SW_HIP(hipMemcpyAsync(track_starts, a.ST, sizeof(int32_t) * n_tr, hipMemcpyDeviceToHost, st));
    SW_HIP(hipStreamSynchronize(st));
    std::memcpy(hits, out.data(), sizeof(int32_t) * 2 * nKM);
    std::memcpy(scores, out.data() + 2 * nKM, sizeof(float) * nKM);
    std::memcpy(fired, out.data() + 3 * nKM, sizeof(int32_t) * nKM);
    std::memcpy(counts, out.data() + 4 * nKM, sizeof(int32_t) * nK);
    if (n_tr)                                 // the kernel writes this call's frames; past them -inf / -1
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < K; ++k)
                for (int f = frames[i]; f < F_stride; ++f) {
                    const size_t at = ((size_t)i * K + k) * F_stride + f;
                    if (track_scores) track_scores[at] = -INFINITY;
                    if (track_starts) track_starts[at] = -1;
                }
    return DSMI_OK;
}

extern "C" int dsmi_spot_watch_pick(const float* E, const int32_t* ST, int frames, int t0, int flush, float min_mean_logp, int settle_frames,
                                    dsmi_spot_pick_state* state, int max_events, int32_t* hits, float* scores, int32_t* fired) {
    if (!state || frames < 0 || t0 < 0 || (int64_t)t0 + frames > (int64_t)INT32_MAX || (frames > 0 && (!E || !ST)) || max_events < 0 ||
        (max_events > 0 && (!hits || !scores || !fired)) || settle_frames < 1 || std::isnan(min_mean_logp))
        return DSMI_ERR_INVALID;
    return spot_pick_chunk(*state, E, ST, frames, t0, flush != 0, min_mean_logp, settle_frames, max_events, hits, scores, fired);
}
