// Sample-rate conversion of LIVE audio (gfx950): an utterance that arrives in chunks of any size, converted chunk by chunk so that
// the concatenated outputs are bit for bit those of one dsmi_resample call over the whole utterance (resample.hip).
//
// A dsmi_resampler is one utterance in flight.  Its state is three host integers and one small device buffer:
//   total_in    input samples consumed so far
//   emitted     outputs written so far
//   the tail    every input sample from `tail_start` on, decoded to float64 on the device -- the samples the next outputs still need
//
//   polyphase   output j reads x[k_hi(j) - t], t = 0 .. kmax - 1, k_hi(j) = (j down + half) / up: it is final once sample k_hi(j)
//               is known, so after n samples  ready(n) = #{j : j down + half < n up} = ceil((n up - half) / down)  outputs are
//               (at least 0, at most dsmi_resample_count(n)).  The next output e = ready(n) has k_hi(e) >= n, so the tail
//               [max(0, k_hi(e) - (kmax - 1)), n) holds at most kmax - 1 samples.  The flush (is_last) writes the outputs up to
//               dsmi_resample_count(n) with zeros for x[k >= n], as resample_poly_kernel has them.
//   ratecv      output j reads X[c - 1], X[c], c = ceil(j i / o): linear interpolation looks no further than the sample it
//               stands on, ready(n) = dsmi_resample_count(n), and the tail is the one sample x[n - 1].
//   equal rates ready(n) = n, no tail.
//
// dsmi_resampler_push_many advances up to 256 handles by one chunk each.  Sessions are sorted by kernel (polyphase / ratecv / copy)
// and described by one table of RS_WORDS int64 words each, staged through the frontend's pinned ring: at most one launch per kernel
// present, whatever the number of sessions; blockIdx.y is the session, a workgroup makes 256 consecutive outputs of it.  The
// polyphase kernel is resample_poly_kernel with a different source of samples: the same tap table, the same fma order, and sample k
// of the utterance comes from the tail (k before this chunk), from the chunk through ld_sample, or is zero (k < 0, k >= total).
//
// The tail lives in TWO buffers used alternately: workgroup 0 of a session writes the next tail -- part old tail, part chunk when
// the chunk is shorter than the tail -- into the buffer the launch does not read, while the session's other workgroups still read
// the old one.  No second launch, no ordering between workgroups.
#include "common.h"
#include "frontend.h"
#include "resample.h"

#include <cstdio>

using namespace dsmi;

enum { RS_POLY = 0, RS_RATECV = 1, RS_COPY = 2 };

struct dsmi_resampler {
    dsmi_frontend* f = nullptr;
    int rate_in = 0, method = 0, dtype = 0, kind = RS_COPY;
    Ratio r{};
    const dsmi_resample_filter* flt = nullptr;     // polyphase: the frontend's cached table of rate_in
    int kmax = 0, kstride = 0;
    size_t lds = 0;
    double* tail[2] = {nullptr, nullptr};          // device, tail_cap doubles each; tail[parity] is current
    int tail_cap = 0, parity = 0;
    int64_t total_in = 0, emitted = 0, tail_start = 0;
    std::string err;
};

namespace {

// one session of a launch, int64 words
enum { W_PCM, W_DTYPE, W_K0, W_NCHUNK, W_J0, W_NOUT, W_OUT, W_TAIL_OLD, W_TS_OLD, W_TAIL_NEW, W_TS_NEW, W_NEWLEN, W_TAB, W_UP, W_DOWN,
       W_HALF, W_KMAX, W_KSTRIDE, RS_WORDS };

// Where sample k of the utterance is: the carried tail [ts_old, k0), the chunk [k0, k0 + n), zero elsewhere (before the
// utterance; past its end on a flush).  ts_old >= 0; nothing in [0, ts_old) is ever asked for.
struct Source {
    const void* pcm; int dtype; int64_t k0, n, ts_old; const double* tail_old;
    __device__ __forceinline__ explicit Source(const int64_t* d)
        : pcm((const void*)d[W_PCM]), dtype((int)d[W_DTYPE]), k0(d[W_K0]), n(d[W_NCHUNK]), ts_old(d[W_TS_OLD]),
          tail_old((const double*)d[W_TAIL_OLD]) {}
    __device__ __forceinline__ double at(int64_t k) const {
        if (k < k0) return k >= ts_old ? tail_old[k - ts_old] : 0.0;
        k -= k0;
        return k < n ? ld_sample(pcm, dtype, k) : 0.0;
    }
};

// workgroup 0 of a session: the tail the NEXT push reads, into the buffer this launch does not read
__device__ __forceinline__ void write_next_tail(const int64_t* d, const Source& src, int tid, int nthreads) {
    double* tail_new = (double*)d[W_TAIL_NEW];
    const int64_t ts_new = d[W_TS_NEW];
    const int len = (int)d[W_NEWLEN];
    for (int i = tid; i < len; i += nthreads) tail_new[i] = src.at(ts_new + i);
}

__global__ __launch_bounds__(RS_OT) void resample_stream_poly_kernel(const int64_t* desc, double* out) {
    extern __shared__ __attribute__((aligned(16))) double s_x[];
    const int64_t* d = desc + (size_t)blockIdx.y * RS_WORDS;
    const int tid = threadIdx.x;
    const Source src(d);
    if (blockIdx.x == 0) write_next_tail(d, src, tid, RS_OT);
    const int64_t cnt = d[W_NOUT], jb = (int64_t)blockIdx.x * RS_OT;
    if (jb >= cnt) return;
    const int64_t e0 = d[W_J0];                             // outputs of the utterance before this push
    const int up = (int)d[W_UP], down = (int)d[W_DOWN], half = (int)d[W_HALF], kmax = (int)d[W_KMAX], kstride = (int)d[W_KSTRIDE];
    const double* tab = (const double*)d[W_TAB];
    const int64_t j0 = e0 + jb, j1 = e0 + (jb + RS_OT < cnt ? jb + RS_OT : cnt) - 1;
    // output j reads x[k_hi(j) - t], t = 0 .. kmax - 1, with k_hi(j) = (j down + half) / up (non-decreasing in j)
    const int64_t k_lo = (j0 * down + half) / up - (kmax - 1), k_top = (j1 * down + half) / up;
    const int span = (int)(k_top - k_lo + 1);
    for (int i = tid; i < span; i += RS_OT) s_x[i] = src.at(k_lo + i);
    __syncthreads();
    const int64_t j = j0 + tid;
    if (j > j1) return;
    const int64_t q = j * down + half;
    const int r = (int)(q % up);
    const double* x = s_x + (q / up - k_lo);            // x[-t]: index >= 0 because k_hi(j) >= k_hi(j0)
    const double2* row = reinterpret_cast<const double2*>(tab + (size_t)r * kstride);      // kstride is even: 16-byte rows
    double acc = 0.0;
    for (int t = 0; t + 1 < kmax; t += 2) {                // resample_poly_kernel's order: t = 0 .. kmax - 1
        const double2 h = row[t >> 1];
        acc = fma(x[-t], h.x, acc);
        acc = fma(x[-t - 1], h.y, acc);
    }
    if (kmax & 1) acc = fma(x[-(kmax - 1)], tab[(size_t)r * kstride + kmax - 1], acc);
    out[d[W_OUT] + jb + tid] = acc;
}

// resample_ratecv_kernel's closed form with X[c - 1] from the carried sample; W_UP = o, W_DOWN = i, W_HALF = 32 - 8 * sample width
__global__ __launch_bounds__(256) void resample_stream_ratecv_kernel(const int64_t* desc, double* out) {
    const int64_t* d = desc + (size_t)blockIdx.y * RS_WORDS;
    const Source src(d);
    if (blockIdx.x == 0) write_next_tail(d, src, threadIdx.x, 256);
    const int64_t jl = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (jl >= d[W_NOUT]) return;
    const int64_t o_ = d[W_UP], i_ = d[W_DOWN];
    const int sh = (int)d[W_HALF];
    const int64_t j = d[W_J0] + jl;
    const int64_t ji = j * i_, c = (ji + o_ - 1) / o_, dd = c * o_ - ji;
    const double scale = (double)(1ll << sh);
    const double cur = src.at(c) * scale;
    const double prev = c > 0 ? src.at(c - 1) * scale : 0.0;
    const double v = prev * (double)dd + cur * (double)(o_ - dd);                    // integers below 2^53: exact
    const int64_t y = (int64_t)(v / (double)o_);                                    // the conversion truncates, as C's does
    out[d[W_OUT] + jl] = (double)(y >> sh);
}

// rate_in == rate_out: the decoded samples as they are (no tail: every sample is an output at once)
__global__ __launch_bounds__(256) void resample_stream_copy_kernel(const int64_t* desc, double* out) {
    const int64_t* d = desc + (size_t)blockIdx.y * RS_WORDS;
    const int64_t jl = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (jl >= d[W_NOUT]) return;
    out[d[W_OUT] + jl] = ld_sample((const void*)d[W_PCM], (int)d[W_DTYPE], jl);
}

// outputs that are final once n input samples of the utterance are known
int64_t ready_of(int kind, int64_t up, int64_t down, int64_t half, int64_t n) {
    if (n <= 0) return 0;
    if (kind == RS_COPY) return n;
    if (kind == RS_RATECV) return ((n - 1) * up) / down + 1;
    const int64_t num = n * up - half;
    return num <= 0 ? 0 : std::min((num + down - 1) / down, (n * up + down - 1) / down);
}

int64_t count_of(int kind, int64_t up, int64_t down, int64_t n) {
    if (n <= 0) return 0;
    if (kind == RS_COPY) return n;
    return kind == RS_RATECV ? ((n - 1) * up) / down + 1 : (n * up + down - 1) / down;
}

// first sample the tail must hold when `emitted` outputs are out and `total` samples are in
int64_t tail_start_of(const dsmi_resampler* r, int64_t emitted, int64_t total) {
    if (r->kind == RS_COPY) return total;
    if (r->kind == RS_RATECV) return std::max<int64_t>(total - 1, 0);
    const int64_t k_lo = (emitted * r->r.down + r->r.half) / r->r.up - (r->kmax - 1);
    return std::min(std::max<int64_t>(k_lo, 0), total);
}

const char* check_pcm_dtype(int dtype) {
    const int base = dtype & 15;
    const bool stereo_ok = base == DSMI_PCM_I16 || base == DSMI_PCM_I24 || base == DSMI_PCM_I32;
    if (dtype < 0 || base > DSMI_PCM_I32 || (dtype & ~(15 | DSMI_PCM_STEREO)) || ((dtype & DSMI_PCM_STEREO) && !stereo_ok))
        return "resampler: bad pcm_dtype (8-bit and float PCM cannot be stereo)";
    return nullptr;
}

}  // namespace

extern "C" int64_t dsmi_resample_ready(int method, int rate_in, int rate_out, int64_t n_in) {
    if (dsmi_resample_count(method, rate_in, rate_out, n_in) < 0) return DSMI_ERR_INVALID;       // bad arguments, or n_in * up overflows
    if (rate_in == rate_out) return n_in;
    Ratio r;
    const int g = std::gcd(rate_in, rate_out);
    r.up = rate_out / g; r.down = rate_in / g; r.half = 10 * (int64_t)std::max(r.up, r.down);
    return ready_of(method == DSMI_RESAMPLE_RATECV ? RS_RATECV : RS_POLY, r.up, r.down, r.half, n_in);
}

extern "C" int dsmi_resampler_create(dsmi_frontend* f, int rate_in, int method, int pcm_dtype, dsmi_resampler** out) {
    auto bad = [&](int code, const char* msg) { fe_set_thread_error(msg); if (f) f->err = msg; return code; };
    // ---- the refusals of dsmi_resample, all before the device is touched
    if (!out) return bad(DSMI_ERR_INVALID, "resampler: null argument");
    if (rate_in <= 0) return bad(DSMI_ERR_INVALID, "resampler: rate_in must be positive");
    if (method != DSMI_RESAMPLE_POLYPHASE && method != DSMI_RESAMPLE_RATECV) return bad(DSMI_ERR_INVALID, "resampler: unknown method");
    if (const char* msg = check_pcm_dtype(pcm_dtype)) return bad(DSMI_ERR_INVALID, msg);
    if (method == DSMI_RESAMPLE_RATECV && (pcm_dtype == DSMI_PCM_F32 || pcm_dtype == DSMI_PCM_F64))
        return bad(DSMI_ERR_INVALID, "resampler: ratecv is defined on integer samples, not on float PCM");
    if (!f) return bad(DSMI_ERR_INVALID, "resampler: null frontend");
    const int rate_out = f->desc.sample_rate;
    if (rate_out <= 0) return bad(DSMI_ERR_INVALID, "resampler: the frontend's sample_rate must be positive");
    Ratio r;
    if (const char* msg = poly_ratio(rate_in, rate_out, &r)) return bad(DSMI_ERR_CAPACITY, msg);     // too many taps, too steep a decimation
    const int kind = rate_in == rate_out ? RS_COPY : (method == DSMI_RESAMPLE_RATECV ? RS_RATECV : RS_POLY);
    if (kind == RS_POLY && poly_lds_bytes(r) > RS_LDS_MAX) return bad(DSMI_ERR_CAPACITY, "resampler: the input span of one workgroup does not fit LDS");
    if (hipSetDevice(f->device) != hipSuccess) return bad(DSMI_ERR_HIP, "hipSetDevice failed");
    dsmi_resampler* h = new dsmi_resampler();
    h->f = f; h->rate_in = rate_in; h->method = method; h->dtype = pcm_dtype; h->kind = kind; h->r = r;
    if (kind == RS_POLY) {
        int code = DSMI_OK; const char* msg = nullptr;
        h->flt = fe_resample_filter(f, rate_in, r, &code, &msg);
        if (!h->flt) { delete h; return bad(code, msg); }
        h->kmax = h->flt->kmax; h->kstride = poly_kstride(h->kmax); h->lds = poly_lds_bytes(r);
    }
    h->tail_cap = kind == RS_POLY ? h->kmax : 1;           // the tail holds at most kmax - 1 samples (1 for ratecv)
    if (kind != RS_COPY) {
        for (int p = 0; p < 2; ++p)
            if (hipMalloc((void**)&h->tail[p], sizeof(double) * h->tail_cap) != hipSuccess) {
                if (h->tail[0]) (void)hipFree(h->tail[0]);
                delete h;
                return bad(DSMI_ERR_NOMEM, "hipMalloc failed");
            }
    }
    *out = h;
    return DSMI_OK;
}

// Frees the handle's own buffers; the frontend (which owns the filters) is not touched and may be gone already.
extern "C" void dsmi_resampler_destroy(dsmi_resampler* r) {
    if (!r) return;
    for (double* t : r->tail) if (t) (void)hipFree(t);      // (hipFree waits for the work that may still read it)
    delete r;
}

extern "C" const char* dsmi_resampler_last_error(const dsmi_resampler* r) { return r ? r->err.c_str() : dsmi_frontend_last_error(nullptr); }

extern "C" int dsmi_resampler_reset(dsmi_resampler* r) {
    if (!r) return DSMI_ERR_INVALID;
    r->total_in = r->emitted = r->tail_start = 0;          // an empty tail: nothing on the device has to be cleared
    return DSMI_OK;
}

extern "C" int dsmi_resampler_position(const dsmi_resampler* r, int64_t* n_in, int64_t* n_out) {
    if (!r) return DSMI_ERR_INVALID;
    if (n_in) *n_in = r->total_in;
    if (n_out) *n_out = r->emitted;
    return DSMI_OK;
}

extern "C" int dsmi_resampler_push_many(dsmi_resampler* const* rs, int n, const void* const* pcm, const int64_t* n_samples, const int* is_last,
                                        double* out, int64_t out_capacity, int64_t* n_out, void* stream) {
    char text[200];
    auto bad = [&](int code, int session, const char* msg) {
        if (session >= 0) std::snprintf(text, sizeof(text), "resampler push: session %d: %s", session, msg);
        else std::snprintf(text, sizeof(text), "resampler push: %s", msg);
        fe_set_thread_error(text);
        if (session >= 0 && rs && rs[session]) rs[session]->err = text;
        return code;
    };
    // ---- everything that can refuse the call comes before the first launch and before any handle changes
    if (!rs || !pcm || !n_samples || !is_last || !n_out || out_capacity < 0) return bad(DSMI_ERR_INVALID, -1, "null argument or negative capacity");
    if (n < 1 || n > DSMI_RESAMPLE_STREAM_MAX) return bad(DSMI_ERR_INVALID, -1, "the number of sessions must be 1 .. DSMI_RESAMPLE_STREAM_MAX");
    for (int i = 0; i < n; ++i) {
        if (!rs[i]) return bad(DSMI_ERR_INVALID, i, "null handle");
        if (rs[i]->f != rs[0]->f) return bad(DSMI_ERR_INVALID, i, "the handle belongs to another frontend");
        for (int k = 0; k < i; ++k) if (rs[k] == rs[i]) return bad(DSMI_ERR_INVALID, i, "the handle appears twice");
        if (n_samples[i] < 0) return bad(DSMI_ERR_INVALID, i, "negative sample count");
        if (n_samples[i] > 0 && !pcm[i]) return bad(DSMI_ERR_INVALID, i, "null chunk");
    }
    dsmi_frontend* f = rs[0]->f;
    struct Plan { int64_t total, emitted, ts_new, nout, off; int newlen; bool launch; };
    std::vector<Plan> plan(n);
    int64_t off = 0, max_out[3] = {0, 0, 0};
    int per_kind[3] = {0, 0, 0};
    size_t lds = 0;
    for (int i = 0; i < n; ++i) {
        const dsmi_resampler* r = rs[i];
        Plan& p = plan[i];
        if (n_samples[i] > INT64_MAX - r->total_in) return bad(DSMI_ERR_INVALID, i, "sample count out of range");
        p.total = r->total_in + n_samples[i];
        if (dsmi_resample_count(r->method, r->rate_in, f->desc.sample_rate, p.total) < 0) return bad(DSMI_ERR_INVALID, i, "sample count out of range");
        p.emitted = is_last[i] ? count_of(r->kind, r->r.up, r->r.down, p.total) : ready_of(r->kind, r->r.up, r->r.down, r->r.half, p.total);
        p.nout = p.emitted - r->emitted;
        if (p.nout < 0 || p.nout > (int64_t)INT32_MAX * 128) return bad(DSMI_ERR_INVALID, i, "chunk too long");
        p.off = off;
        if (off + p.nout < off) return bad(DSMI_ERR_INVALID, i, "sample count out of range");
        off += p.nout;
        p.ts_new = is_last[i] ? p.total : tail_start_of(r, p.emitted, p.total);
        p.newlen = (int)(p.total - p.ts_new);
        // the bounds the kernels rely on: both tails fit their buffers, and the new tail starts no earlier than the old one
        if (p.newlen > r->tail_cap || r->total_in - r->tail_start > r->tail_cap || p.ts_new < r->tail_start || (r->kind == RS_POLY && p.newlen > r->kmax - 1))
            return bad(DSMI_ERR_INVALID, i, "internal: the carried tail is out of its bounds");
        p.launch = n_samples[i] > 0 || p.nout > 0;         // nothing new and nothing to flush: the handle's tail stays as it is
        if (p.launch) {
            per_kind[r->kind]++;
            max_out[r->kind] = std::max(max_out[r->kind], p.nout);
            if (r->kind == RS_POLY) lds = std::max(lds, r->lds);
        }
    }
    if (off > out_capacity) return bad(DSMI_ERR_CAPACITY, -1, "out_dev is smaller than the sum of the sessions' outputs (dsmi_resample_ready)");
    if (off > 0 && !out) return bad(DSMI_ERR_INVALID, -1, "null out_dev");
    const int n_launch = per_kind[0] + per_kind[1] + per_kind[2];
    hipStream_t s = (hipStream_t)stream;
    if (n_launch > 0) {
        if (hipSetDevice(f->device) != hipSuccess) return bad(DSMI_ERR_HIP, -1, "hipSetDevice failed");
        if (!f->rss_desc) {
            // the frontend's first push: the device table and the pinned ring at the size of the largest call, once -- growing the
            // ring waits for the whole device, which no later push may do
            if (!fe_stage_reserve(f, RS_WORDS * DSMI_RESAMPLE_STREAM_MAX)) return bad(DSMI_ERR_NOMEM, -1, "growing the pinned staging ring failed");
            if (hipMalloc((void**)&f->rss_desc, sizeof(int64_t) * RS_WORDS * DSMI_RESAMPLE_STREAM_MAX) != hipSuccess) return bad(DSMI_ERR_NOMEM, -1, "hipMalloc failed");
        }
        // ---- the descriptor table, sessions sorted by kernel: [polyphase | ratecv | copy]
        std::vector<int64_t> host((size_t)n_launch * RS_WORDS, 0);
        int at[3] = {0, per_kind[0], per_kind[0] + per_kind[1]};
        const int first[3] = {at[0], at[1], at[2]};
        for (int i = 0; i < n; ++i) {
            if (!plan[i].launch) continue;
            const dsmi_resampler* r = rs[i];
            const Plan& p = plan[i];
            int64_t* d = &host[(size_t)(at[r->kind]++) * RS_WORDS];
            d[W_PCM] = (int64_t)(uintptr_t)pcm[i]; d[W_DTYPE] = r->dtype; d[W_K0] = r->total_in; d[W_NCHUNK] = n_samples[i];
            d[W_J0] = r->emitted; d[W_NOUT] = p.nout; d[W_OUT] = p.off;
            d[W_TAIL_OLD] = (int64_t)(uintptr_t)r->tail[r->parity]; d[W_TS_OLD] = r->tail_start;
            d[W_TAIL_NEW] = (int64_t)(uintptr_t)r->tail[r->parity ^ 1]; d[W_TS_NEW] = p.ts_new; d[W_NEWLEN] = p.newlen;
            d[W_UP] = r->r.up; d[W_DOWN] = r->r.down;
            if (r->kind == RS_POLY) {
                d[W_TAB] = (int64_t)(uintptr_t)r->flt->tab; d[W_HALF] = r->r.half; d[W_KMAX] = r->kmax; d[W_KSTRIDE] = r->kstride;
            } else {
                d[W_HALF] = ratecv_shift(r->dtype);
            }
        }
        if (!fe_stage_copy(f, f->rss_desc, host.data(), n_launch * RS_WORDS, s)) return bad(DSMI_ERR_HIP, -1, "staging the sessions' descriptors failed");
        auto grid = [&](int kind) { return dim3((unsigned)std::max<int64_t>(1, (max_out[kind] + 255) / 256), per_kind[kind]); };
        static_assert(RS_OT == 256, "the grids count 256 outputs per workgroup");
        if (per_kind[RS_POLY])
            hipLaunchKernelGGL(resample_stream_poly_kernel, grid(RS_POLY), dim3(RS_OT), lds, s, f->rss_desc + (size_t)first[RS_POLY] * RS_WORDS, out);
        if (per_kind[RS_RATECV])
            hipLaunchKernelGGL(resample_stream_ratecv_kernel, grid(RS_RATECV), dim3(256), 0, s, f->rss_desc + (size_t)first[RS_RATECV] * RS_WORDS, out);
        if (per_kind[RS_COPY] && max_out[RS_COPY] > 0)
            hipLaunchKernelGGL(resample_stream_copy_kernel, grid(RS_COPY), dim3(256), 0, s, f->rss_desc + (size_t)first[RS_COPY] * RS_WORDS, out);
        if (hipGetLastError() != hipSuccess) return bad(DSMI_ERR_HIP, -1, "resample kernel failed to launch");
    }
    // ---- the launches are in the stream: the handles move on
    for (int i = 0; i < n; ++i) {
        dsmi_resampler* r = rs[i];
        const Plan& p = plan[i];
        n_out[i] = p.nout;
        if (is_last[i]) {
            r->total_in = r->emitted = r->tail_start = 0;      // the start of a new utterance
            continue;
        }
        if (!p.launch) continue;
        r->total_in = p.total; r->emitted = p.emitted; r->tail_start = p.ts_new;
        if (r->kind != RS_COPY) r->parity ^= 1;
    }
    return DSMI_OK;
}
