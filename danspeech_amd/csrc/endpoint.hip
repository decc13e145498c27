// Utterances in LIVE audio (gfx950): the energy gate of Recognizer.listen_stream (Recognizer.py:218-324) over continuous streams
// that arrive in pushes of any size, for up to DSMI_ENDPOINT_MAX sessions per call (include/dsmi.h has the contract).
//
// A dsmi_endpointer is one stream in flight.  The stream is a sequence of buffers of `chunk` samples, buffer b = samples
// [b chunk, (b + 1) chunk); the host keeps the gate's state (host_logic.h) and three positions:
//   consumed     samples pushed so far: buffers below consumed / chunk have been gated
//   tail_start   a multiple of chunk: the tail [tail_start, consumed), decoded to float64 on the device, holds the buffers a waiting
//                session keeps and the incomplete buffer at the end of the last push -- at most (keep_n + 1) chunk - 1 samples
//
// A push is   table of sessions -> kernel 1 -> synchronise -> gate on the host -> table of copies -> kernel 2:
//   kernel 1     one wave per buffer that is complete now: sample k comes from the tail (k < consumed) or from the new chunk through
//                ld_sample; v * v as a 64-bit integer per lane, reduced across the wave, one uint64 per buffer into pinned host
//                memory.  Float samples enter the sum as llrint(x) saturated to int16.
//   kernel 2     one row of the copy table per emitted event and per retained tail, blockIdx.y the row: samples [k, k + count) of
//                the session to out_dev (events, back to back) or to the session's OTHER tail buffer -- the old tail is read by this
//                very launch, so the two buffers of a handle alternate, as the resampler's do.
#include "common.h"
#include "frontend.h"
#include "host_logic.h"

#include <cstdio>

using namespace dsmi;

struct dsmi_endpointer {
    dsmi_frontend* f = nullptr;
    dsmi_endpointer_desc desc{};
    GateParams p{};
    GateState st{};
    double* tail[2] = {nullptr, nullptr};          // device, tail_cap doubles each; tail[parity] is current
    int64_t tail_cap = 0;
    int parity = 0;
    int64_t consumed = 0, tail_start = 0, utterances = 0;
    bool ended = false;
    std::string err;
};

namespace {

// one session of a push, int64 words
enum { E_PCM, E_DTYPE, E_K0, E_NCHUNK, E_TAIL_OLD, E_TS_OLD, E_BUF0, E_CHUNK, E_NB, E_TOTAL, E_SUM0, E_WORDS };
// one copy of kernel 2: the session's row, the first sample, the count, the destination
enum { J_ROW, J_K, J_COUNT, J_DST, J_WORDS };

constexpr int GATHER_TILE = 1024;                  // samples per workgroup of kernel 2
constexpr int64_t MAX_HELD = (int64_t)1 << 24;     // (keep_n + 1) chunk: 128 MiB of float64 per tail buffer at most
constexpr int RESERVE_BUFFERS = 16;                // buffers per session the first push sizes the tables for

// Where sample k of the stream is: the carried tail [ts_old, k0), the chunk [k0, k0 + n).  The host asks for nothing else.
struct Source {
    const void* pcm; int dtype; int64_t k0, n, ts_old; const double* tail_old;
    __device__ __forceinline__ explicit Source(const int64_t* d)
        : pcm((const void*)d[E_PCM]), dtype((int)d[E_DTYPE]), k0(d[E_K0]), n(d[E_NCHUNK]), ts_old(d[E_TS_OLD]),
          tail_old((const double*)d[E_TAIL_OLD]) {}
    __device__ __forceinline__ double at(int64_t k) const {
        if (k < k0) return k >= ts_old ? tail_old[k - ts_old] : 0.0;
        k -= k0;
        return k < n ? ld_sample(pcm, dtype, k) : 0.0;
    }
};

// the sample as audioop.rms sees it: integer samples as they are, float samples rounded to nearest-even and saturated to int16
__device__ __forceinline__ int64_t gate_value(double x) {
    return (int64_t)llrint(fmin(fmax(x, -32768.0), 32767.0));
}

__global__ __launch_bounds__(256) void endpoint_sums_kernel(const int64_t* tab, unsigned long long* sums) {
    const int64_t* d = tab + (size_t)blockIdx.y * E_WORDS;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= d[E_NB]) return;
    const Source src(d);
    const int64_t chunk = d[E_CHUNK], b0 = d[E_BUF0] + w * chunk;
    const int64_t len = d[E_TOTAL] - b0 < chunk ? d[E_TOTAL] - b0 : chunk;       // the stream's final buffer may be short
    long long acc = 0;
    for (int64_t i = lane; i < len; i += 64) {
        const int64_t v = gate_value(src.at(b0 + i));
        acc += v * v;                                                           // at most 2^30 each, 2^16 of them: exact
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) sums[d[E_SUM0] + w] = (unsigned long long)acc;
}

__global__ __launch_bounds__(256) void endpoint_gather_kernel(const int64_t* tab, const int64_t* jobs) {
    const int64_t* j = jobs + (size_t)blockIdx.y * J_WORDS;
    const int64_t count = j[J_COUNT], i0 = (int64_t)blockIdx.x * GATHER_TILE;
    if (i0 >= count) return;
    const Source src(tab + (size_t)j[J_ROW] * E_WORDS);
    const int64_t k = j[J_K];
    double* dst = (double*)j[J_DST];
    for (int q = 0; q < GATHER_TILE / 256; ++q) {
        const int64_t i = i0 + q * 256 + threadIdx.x;
        if (i < count) dst[i] = src.at(k + i);
    }
}

// what create refuses, in the order create checks it; nullptr for a desc it takes
const char* check_desc(const dsmi_endpointer_desc* d, GateParams* p) {
    if (!d) return "endpointer: null desc";
    if (d->chunk < 16 || d->chunk > 65536) return "endpointer: chunk must be within 16 .. 65536";
    if (d->rate <= 0) return "endpointer: rate must be positive";
    if (d->pcm_dtype != DSMI_PCM_I16 && d->pcm_dtype != (DSMI_PCM_I16 | DSMI_PCM_STEREO) && d->pcm_dtype != DSMI_PCM_F32 && d->pcm_dtype != DSMI_PCM_F64)
        return "endpointer: the gate takes int16 (one or two channels), float32 and float64 samples: audioop.rms of 8-bit audio reads "
               "unsigned bytes as signed, and sums of squared 24/32-bit samples are not exact";
    if (!(d->energy_threshold >= 0) || !(d->non_speaking_duration >= 0) || !(d->pause_threshold >= d->non_speaking_duration) || !(d->phrase_threshold >= 0) ||
        !(d->pause_threshold < 1e9) || !(d->phrase_threshold < 1e9))
        return "endpointer: thresholds must satisfy pause_threshold >= non_speaking_duration >= 0 (Recognizer.py:237)";
    p->threshold = d->energy_threshold;
    p->pause_n = gate_buffer_count(d->pause_threshold, d->chunk, d->rate);
    p->phrase_n = gate_buffer_count(d->phrase_threshold, d->chunk, d->rate);
    p->keep_n = gate_buffer_count(d->non_speaking_duration, d->chunk, d->rate);
    return nullptr;
}

}  // namespace

void fe_endpoint_release(dsmi_frontend* f) {
    if (f->ep_tab) (void)hipFree(f->ep_tab);
    if (f->ep_sums) (void)hipHostFree(f->ep_sums);
    f->ep_tab = nullptr; f->ep_sums = nullptr; f->ep_tab_cap = f->ep_sums_cap = 0;
}

extern "C" int dsmi_endpoint_counts(const dsmi_endpointer_desc* desc, int64_t* counts3) {
    GateParams p{};
    if (!counts3 || check_desc(desc, &p)) return DSMI_ERR_INVALID;
    counts3[0] = p.pause_n; counts3[1] = p.phrase_n; counts3[2] = p.keep_n;
    return DSMI_OK;
}

extern "C" int64_t dsmi_endpoint_gate(double energy_threshold, int64_t pause_n, int64_t phrase_n, int64_t keep_n, int64_t* state4,
                                      const uint64_t* S, const int64_t* len, int64_t n_buffers, int end_of_stream, int64_t* ev_first,
                                      int64_t* ev_count, int32_t* ev_last, int64_t max_events, uint32_t* energies) {
    if (!state4 || n_buffers < 0 || (n_buffers > 0 && (!S || !len)) || max_events < 0 || (max_events > 0 && (!ev_first || !ev_count || !ev_last)) ||
        pause_n < 0 || phrase_n < 0 || keep_n < 0 || !(energy_threshold >= 0))
        return DSMI_ERR_INVALID;
    GateState st{state4[0], state4[1], state4[2], state4[3]};
    if ((st.phase != 0 && st.phase != 1) || st.kept < 0 || st.kept > keep_n || st.phrase_count < 0 || st.pause_count < 0) return DSMI_ERR_INVALID;
    for (int64_t i = 0; i < n_buffers; ++i) if (len[i] <= 0) return DSMI_ERR_INVALID;
    GateEvents ev{ev_first, ev_count, ev_last, max_events};
    endpoint_gate(GateParams{energy_threshold, pause_n, phrase_n, keep_n}, st, S, len, n_buffers, end_of_stream != 0, ev, energies);
    state4[0] = st.phase; state4[1] = st.kept; state4[2] = st.phrase_count; state4[3] = st.pause_count;
    return ev.n;
}

extern "C" int dsmi_endpointer_create(dsmi_frontend* f, const dsmi_endpointer_desc* desc, dsmi_endpointer** out) {
    auto bad = [&](int code, const char* msg) { fe_set_thread_error(msg); if (f) f->err = msg; return code; };
    if (!out) return bad(DSMI_ERR_INVALID, "endpointer: null argument");
    GateParams p{};
    if (const char* msg = check_desc(desc, &p)) return bad(DSMI_ERR_INVALID, msg);
    if (!f) return bad(DSMI_ERR_INVALID, "endpointer: null frontend");
    if (p.keep_n + 1 > MAX_HELD / desc->chunk) return bad(DSMI_ERR_CAPACITY, "endpointer: non_speaking_duration keeps more than 2^24 samples");
    if (hipSetDevice(f->device) != hipSuccess) return bad(DSMI_ERR_HIP, "hipSetDevice failed");
    dsmi_endpointer* e = new dsmi_endpointer();
    e->f = f; e->desc = *desc; e->p = p;
    e->tail_cap = (p.keep_n + 1) * desc->chunk;
    for (int k = 0; k < 2; ++k)
        if (hipMalloc((void**)&e->tail[k], sizeof(double) * e->tail_cap) != hipSuccess) {
            if (e->tail[0]) (void)hipFree(e->tail[0]);
            delete e;
            return bad(DSMI_ERR_NOMEM, "hipMalloc failed");
        }
    *out = e;
    return DSMI_OK;
}

// Frees the handle's own buffers; the frontend is not touched and may be gone already.
extern "C" void dsmi_endpointer_destroy(dsmi_endpointer* e) {
    if (!e) return;
    for (double* t : e->tail) if (t) (void)hipFree(t);      // (hipFree waits for the work that may still read it)
    delete e;
}

extern "C" const char* dsmi_endpointer_last_error(const dsmi_endpointer* e) { return e ? e->err.c_str() : dsmi_frontend_last_error(nullptr); }

extern "C" int dsmi_endpointer_reset(dsmi_endpointer* e) {
    if (!e) return DSMI_ERR_INVALID;
    e->st = GateState{};
    e->consumed = e->tail_start = e->utterances = 0;       // an empty tail: nothing on the device has to be cleared
    e->ended = false;
    return DSMI_OK;
}

extern "C" int dsmi_endpointer_position(const dsmi_endpointer* e, int64_t* n_in, int64_t* n_utterances, int64_t* n_held) {
    if (!e) return DSMI_ERR_INVALID;
    if (n_in) *n_in = e->consumed;
    if (n_utterances) *n_utterances = e->utterances;
    if (n_held) *n_held = e->consumed - e->tail_start;
    return DSMI_OK;
}

extern "C" int dsmi_endpointer_push_many(dsmi_endpointer* const* es, int n, const void* const* pcm, const int64_t* n_samples,
                                         const int* end_of_stream, double* out, int64_t out_capacity, int32_t* seg_session,
                                         int64_t* seg_len, int32_t* seg_last, int max_segments, int* n_segments, uint32_t* energies_host,
                                         void* stream) {
    char text[200];
    auto bad = [&](int code, int session, const char* msg) {
        if (session >= 0) std::snprintf(text, sizeof(text), "endpointer push: session %d: %s", session, msg);
        else std::snprintf(text, sizeof(text), "endpointer push: %s", msg);
        fe_set_thread_error(text);
        if (session >= 0 && es && es[session]) es[session]->err = text;
        return code;
    };
    // ---- everything that can refuse the call comes before the first launch and before any handle changes
    if (!es || !pcm || !n_samples || !end_of_stream || !n_segments || out_capacity < 0 || max_segments < 0 ||
        (max_segments > 0 && (!seg_session || !seg_len || !seg_last)))
        return bad(DSMI_ERR_INVALID, -1, "null argument or negative capacity");
    if (n < 1 || n > DSMI_ENDPOINT_MAX) return bad(DSMI_ERR_INVALID, -1, "the number of sessions must be 1 .. DSMI_ENDPOINT_MAX");
    for (int i = 0; i < n; ++i) {
        if (!es[i]) return bad(DSMI_ERR_INVALID, i, "null handle");
        if (es[i]->f != es[0]->f) return bad(DSMI_ERR_INVALID, i, "the handle belongs to another frontend");
        for (int k = 0; k < i; ++k) if (es[k] == es[i]) return bad(DSMI_ERR_INVALID, i, "the handle appears twice");
        if (n_samples[i] < 0) return bad(DSMI_ERR_INVALID, i, "negative sample count");
        if (n_samples[i] > 0 && !pcm[i]) return bad(DSMI_ERR_INVALID, i, "null chunk");
        if (n_samples[i] > 0 && es[i]->ended) return bad(DSMI_ERR_INVALID, i, "samples after end_of_stream: reset the session first");
        if (n_samples[i] > ((int64_t)1 << 40) || es[i]->consumed > ((int64_t)1 << 60)) return bad(DSMI_ERR_INVALID, i, "sample count out of range");
    }
    dsmi_frontend* f = es[0]->f;
    // the worst case, sized before anything runs: a session may emit all it holds and all it is given, in one event per gated
    // buffer and one more
    struct Plan { int64_t total, buf0, nb, sum0; bool eos, active; int row; };
    std::vector<Plan> plan(n);
    int64_t worst_out = 0, worst_seg = 0, n_sums = 0, max_nb = 0;
    int rows = 0;
    for (int i = 0; i < n; ++i) {
        const dsmi_endpointer* e = es[i];
        Plan& p = plan[i];
        const int64_t chunk = e->desc.chunk;
        p.total = e->consumed + n_samples[i];
        p.eos = end_of_stream[i] != 0 && !e->ended;
        p.buf0 = e->consumed / chunk * chunk;
        p.nb = p.total / chunk - e->consumed / chunk + (p.eos && p.total % chunk ? 1 : 0);
        p.active = n_samples[i] > 0 || p.eos;              // nothing new: the handle stays as it is
        p.sum0 = n_sums; p.row = -1;
        if (!p.active) continue;
        // the bounds the kernels rely on
        if (e->tail_start % chunk || e->tail_start > p.buf0 || e->consumed - e->tail_start > e->tail_cap)
            return bad(DSMI_ERR_INVALID, i, "internal: the carried tail is out of its bounds");
        p.row = rows++;
        n_sums += p.nb;
        max_nb = std::max(max_nb, p.nb);
        worst_out += e->consumed - e->tail_start + n_samples[i];
        worst_seg += p.nb + 1;
    }
    if (worst_out > out_capacity) return bad(DSMI_ERR_CAPACITY, -1, "out_dev is smaller than the samples the sessions hold and are given");
    if (worst_seg > max_segments) return bad(DSMI_ERR_CAPACITY, -1, "max_segments is below the sessions' gated buffers + 1 each");
    if (worst_out > 0 && !out) return bad(DSMI_ERR_INVALID, -1, "null out_dev");
    // (the tables are indexed by int: the worst case of 2^27 buffers in one call is no live audio)
    if (worst_seg > ((int64_t)1 << 27)) return bad(DSMI_ERR_INVALID, -1, "more than 2^27 buffers in one call: push the samples in parts");
    *n_segments = 0;
    if (rows == 0) return DSMI_OK;

    hipStream_t s = (hipStream_t)stream;
    if (hipSetDevice(f->device) != hipSuccess) return bad(DSMI_ERR_HIP, -1, "hipSetDevice failed");
    // ---- tables and the pinned sums: sized at the frontend's first push for DSMI_ENDPOINT_MAX sessions of RESERVE_BUFFERS buffers
    // each; a larger call grows them, which waits for the device
    const int64_t max_jobs = worst_seg + rows;
    const int64_t tab_need = std::max<int64_t>((int64_t)rows * E_WORDS + max_jobs * J_WORDS,
                                               (int64_t)DSMI_ENDPOINT_MAX * (E_WORDS + (RESERVE_BUFFERS + 2) * J_WORDS));
    const int64_t sums_need = std::max<int64_t>(n_sums, (int64_t)DSMI_ENDPOINT_MAX * RESERVE_BUFFERS);
    if (tab_need > f->ep_tab_cap) {
        if (hipStreamSynchronize(s) != hipSuccess) return bad(DSMI_ERR_HIP, -1, "hipStreamSynchronize failed");
        if (f->ep_tab) (void)hipFree(f->ep_tab);
        f->ep_tab = nullptr; f->ep_tab_cap = 0;
        if (hipMalloc((void**)&f->ep_tab, sizeof(int64_t) * tab_need) != hipSuccess) return bad(DSMI_ERR_NOMEM, -1, "hipMalloc failed");
        f->ep_tab_cap = tab_need;
        if (!fe_stage_reserve(f, (int)tab_need)) return bad(DSMI_ERR_NOMEM, -1, "growing the pinned staging ring failed");
    }
    if (sums_need > f->ep_sums_cap) {
        if (hipStreamSynchronize(s) != hipSuccess) return bad(DSMI_ERR_HIP, -1, "hipStreamSynchronize failed");
        if (f->ep_sums) (void)hipHostFree(f->ep_sums);
        f->ep_sums = nullptr; f->ep_sums_cap = 0;
        if (hipHostMalloc((void**)&f->ep_sums, sizeof(uint64_t) * sums_need, hipHostMallocDefault) != hipSuccess) return bad(DSMI_ERR_NOMEM, -1, "hipHostMalloc failed");
        f->ep_sums_cap = sums_need;
    }
    // ---- the table of sessions
    std::vector<int64_t> host((size_t)rows * E_WORDS, 0);
    for (int i = 0; i < n; ++i) {
        const Plan& p = plan[i];
        if (!p.active) continue;
        const dsmi_endpointer* e = es[i];
        int64_t* d = &host[(size_t)p.row * E_WORDS];
        d[E_PCM] = (int64_t)(uintptr_t)pcm[i]; d[E_DTYPE] = e->desc.pcm_dtype; d[E_K0] = e->consumed; d[E_NCHUNK] = n_samples[i];
        d[E_TAIL_OLD] = (int64_t)(uintptr_t)e->tail[e->parity]; d[E_TS_OLD] = e->tail_start;
        d[E_BUF0] = p.buf0; d[E_CHUNK] = e->desc.chunk; d[E_NB] = p.nb; d[E_TOTAL] = p.total; d[E_SUM0] = p.sum0;
    }
    if (!fe_stage_copy(f, f->ep_tab, host.data(), rows * E_WORDS, s)) return bad(DSMI_ERR_HIP, -1, "staging the sessions' descriptors failed");
    if (n_sums > 0) {
        hipLaunchKernelGGL(endpoint_sums_kernel, dim3((unsigned)((max_nb + 3) / 4), rows), dim3(256), 0, s, f->ep_tab, (unsigned long long*)f->ep_sums);
        if (hipGetLastError() != hipSuccess) return bad(DSMI_ERR_HIP, -1, "the sums kernel failed to launch");
        if (hipStreamSynchronize(s) != hipSuccess) return bad(DSMI_ERR_HIP, -1, "the sums kernel failed");
    }
    // ---- the gate, session by session (host_logic.h), on copies of the states: the handles move on once kernel 2 is in the stream
    std::vector<GateState> st(n);
    std::vector<int64_t> closed(n, 0), ts_new(n, 0), jobs;
    std::vector<int64_t> ev_first, ev_count, lens;
    std::vector<int32_t> ev_last;
    jobs.reserve((size_t)max_jobs * J_WORDS);
    int64_t off = 0, max_count = 0;
    int nseg = 0;
    for (int i = 0; i < n; ++i) {
        const Plan& p = plan[i];
        if (!p.active) continue;
        const dsmi_endpointer* e = es[i];
        const int64_t chunk = e->desc.chunk;
        st[i] = e->st;
        ev_first.assign((size_t)p.nb + 1, 0); ev_count.assign((size_t)p.nb + 1, 0); ev_last.assign((size_t)p.nb + 1, 0);
        lens.resize((size_t)p.nb);
        for (int64_t b = 0; b < p.nb; ++b) lens[(size_t)b] = std::min(chunk, p.total - (p.buf0 + b * chunk));
        GateEvents ev{ev_first.data(), ev_count.data(), ev_last.data(), p.nb + 1};
        closed[i] = endpoint_gate(e->p, st[i], f->ep_sums + p.sum0, lens.data(), p.nb, p.eos, ev, energies_host ? energies_host + p.sum0 : nullptr);
        if (ev.n > p.nb + 1) return bad(DSMI_ERR_INVALID, i, "internal: more events than the worst case");
        for (int64_t k = 0; k < ev.n; ++k) {
            // (the closing event of a stream that ends on a short buffer stands behind that buffer: at the stream's end)
            const int64_t k0 = std::min(p.buf0 + ev_first[(size_t)k] * chunk, p.total), k1 = std::min(k0 + ev_count[(size_t)k] * chunk, p.total);
            if (k0 < e->tail_start || k1 < k0 || off + (k1 - k0) > out_capacity || nseg >= max_segments)
                return bad(DSMI_ERR_INVALID, i, "internal: an event is out of its bounds");
            seg_session[nseg] = i; seg_len[nseg] = k1 - k0; seg_last[nseg] = ev_last[(size_t)k]; ++nseg;
            if (k1 > k0) {
                jobs.insert(jobs.end(), {(int64_t)p.row, k0, k1 - k0, (int64_t)(uintptr_t)(out + off)});
                max_count = std::max(max_count, k1 - k0);
            }
            off += k1 - k0;
        }
        // what the next push still needs: the buffers a waiting session keeps, and the incomplete buffer
        const int64_t next_buf = p.eos ? p.total : p.total / chunk * chunk;
        ts_new[i] = p.eos ? p.total : next_buf - st[i].kept * chunk;
        const int64_t held = p.total - ts_new[i];
        if (ts_new[i] < e->tail_start || held < 0 || held > e->tail_cap) return bad(DSMI_ERR_INVALID, i, "internal: the new tail is out of its bounds");
        if (held > 0) {
            jobs.insert(jobs.end(), {(int64_t)p.row, ts_new[i], held, (int64_t)(uintptr_t)e->tail[e->parity ^ 1]});
            max_count = std::max(max_count, held);
        }
    }
    const int n_jobs = (int)(jobs.size() / J_WORDS);
    if (n_jobs > 0) {
        int64_t* jobs_dev = f->ep_tab + (size_t)rows * E_WORDS;
        if (!fe_stage_copy(f, jobs_dev, jobs.data(), n_jobs * J_WORDS, s)) return bad(DSMI_ERR_HIP, -1, "staging the copies failed");
        // one grid row per copy; a grid has 65535 rows, which only a push of tens of thousands of buffers can exceed
        for (int j0 = 0; j0 < n_jobs; j0 += 65535)
            hipLaunchKernelGGL(endpoint_gather_kernel, dim3((unsigned)((max_count + GATHER_TILE - 1) / GATHER_TILE), std::min(n_jobs - j0, 65535)),
                               dim3(256), 0, s, f->ep_tab, jobs_dev + (size_t)j0 * J_WORDS);
        if (hipGetLastError() != hipSuccess) return bad(DSMI_ERR_HIP, -1, "the gather kernel failed to launch");
    }
    // ---- the launches are in the stream: the handles move on
    for (int i = 0; i < n; ++i) {
        if (!plan[i].active) continue;
        dsmi_endpointer* e = es[i];
        e->st = st[i];
        e->consumed = plan[i].total; e->tail_start = ts_new[i]; e->utterances += closed[i];
        if (plan[i].eos) e->ended = true;
        e->parity ^= 1;
    }
    *n_segments = nseg;
    return DSMI_OK;
}
