// Sample-rate conversion on the GPU (gfx950): audio of any rate -> the model's rate, straight from a WAV file's bytes.
//
// The reference resamples with audioop.ratecv (AudioData.get_raw_data(convert_rate=...), danspeech/audio/resources.py:568-570)
// after the 8-bit bias and SpeechFile's saturating stereo fold.  Two methods, both batched over ragged clips in ONE launch:
//
//   DSMI_RESAMPLE_RATECV     audioop.ratecv(data, width, 1, rate_in, rate_out, None), bit for bit.  ratecv is linear interpolation
//                            whose running state d has a closed form, so one thread makes one output: with i = rate_in / g,
//                            o = rate_out / g, X[k] = x[k] << (32 - 8 width), X[-1] = 0,
//                                c = ceil(j i / o),  d = c o - j i,  y[j] = trunc((X[c-1] d + X[c] (o - d)) / o) >> (32 - 8 width)
//                            Every intermediate is an integer below 2^53 and the one division is IEEE: exact in float64.
//   DSMI_RESAMPLE_POLYPHASE  (default) rational polyphase FIR with scipy.signal.resample_poly's default design: ratecv has no
//                            low-pass, so going down it folds everything above the new Nyquist back into the band.
//                                y[j] = sum_k x[k] h[j down - k up],  h = Kaiser(beta 5)-windowed sinc of 20 max(up, down) + 1 taps
//                            float64 taps (host, once per rate_in, cached on the handle), float64 accumulation, float64 output:
//                            dsmi_features takes float64, and float32 in front of the float64 STFT costs parity in quiet bins.
//
// The polyphase kernel: a workgroup makes OT consecutive outputs of one clip.  Their inputs are one contiguous span of
// (OT - 1) down / up + kmax samples: it is decoded ONCE through ld_sample (sample width, bias, stereo fold) into LDS as float64 --
// every input sample meets about 20 max(up, down) / down taps.  The tap table is laid out by phase, tab[r][t] = h[r + t up] with
// r = (j down + half) mod up: the kmax taps of one output are one contiguous row, read through the caches (a 44.1 kHz table is
// 160 rows of 56: 72 KB, resident in L2; for 8 / 32 / 48 / 96 kHz the rows are 1..3 and every lane reads the same addresses).
#include "common.h"
#include "frontend.h"
#include "resample.h"

using namespace dsmi;

namespace {

constexpr int OT = RS_OT;               // outputs per workgroup (one per thread)
constexpr size_t LDS_MAX = RS_LDS_MAX;

// meta: [4][B] = input offset, input samples, output offset, output samples of every clip
__global__ __launch_bounds__(OT) void resample_poly_kernel(const void* pcm, int dtype, const int64_t* meta, int B, const double* tab,
                                                           int up, int down, int half, int kmax, int kstride, double* out) {
    extern __shared__ __attribute__((aligned(16))) double s_x[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t off_in = meta[b], n = meta[B + b], off_out = meta[2 * B + b], cnt = meta[3 * B + b];
    const int64_t j0 = (int64_t)blockIdx.x * OT;
    if (j0 >= cnt) return;
    const int64_t j1 = (j0 + OT < cnt ? j0 + OT : cnt) - 1;
    // output j reads x[k_hi(j) - t], t = 0 .. kmax - 1, with k_hi(j) = (j down + half) / up (non-decreasing in j)
    const int64_t k_lo = (j0 * down + half) / up - (kmax - 1), k_top = (j1 * down + half) / up;
    const int span = (int)(k_top - k_lo + 1);
    for (int i = tid; i < span; i += OT) {
        const int64_t k = k_lo + i;
        s_x[i] = (k >= 0 && k < n) ? ld_sample(pcm, dtype, off_in + k) : 0.0;       // x is zero outside the clip
    }
    __syncthreads();
    const int64_t j = j0 + tid;
    if (j > j1) return;
    const int64_t q = j * down + half;
    const int r = (int)(q % up);
    const double* x = s_x + (q / up - k_lo);            // x[-t]: index >= 0 because k_hi(j) >= k_hi(j0)
    const double2* row = reinterpret_cast<const double2*>(tab + (size_t)r * kstride);      // kstride is even: 16-byte rows
    double acc = 0.0;
    for (int t = 0; t + 1 < kmax; t += 2) {
        const double2 h = row[t >> 1];
        acc = fma(x[-t], h.x, acc);
        acc = fma(x[-t - 1], h.y, acc);
    }
    if (kmax & 1) acc = fma(x[-(kmax - 1)], tab[(size_t)r * kstride + kmax - 1], acc);
    out[off_out + j] = acc;
}

// audioop.ratecv with weights (1, 0): the closed form at the top of the file.  sh = 32 - 8 * sample width.
__global__ __launch_bounds__(256) void resample_ratecv_kernel(const void* pcm, int dtype, const int64_t* meta, int B, int i_, int o_, int sh,
                                                              double* out) {
    const int b = blockIdx.y;
    const int64_t off_in = meta[b], off_out = meta[2 * B + b], cnt = meta[3 * B + b];
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= cnt) return;
    const int64_t ji = j * i_, c = (ji + o_ - 1) / o_, d = c * o_ - ji;            // c <= n - 1 for every j < cnt
    const double scale = (double)(1ll << sh);
    const double cur = ld_sample(pcm, dtype, off_in + c) * scale;
    const double prev = c > 0 ? ld_sample(pcm, dtype, off_in + c - 1) * scale : 0.0;
    const double v = prev * (double)d + cur * (double)(o_ - d);                     // integers below 2^53: exact
    const int64_t y = (int64_t)(v / (double)o_);                                    // the conversion truncates, as C's does
    out[off_out + j] = (double)(y >> sh);
}

// rate_in == rate_out: the decoded samples as they are
__global__ __launch_bounds__(256) void resample_copy_kernel(const void* pcm, int dtype, const int64_t* meta, int B, double* out) {
    const int b = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= meta[3 * B + b]) return;
    out[meta[2 * B + b] + j] = ld_sample(pcm, dtype, meta[b] + j);
}

}  // namespace

void fe_resample_release(dsmi_frontend* f) {
    for (auto& kv : f->rs_filters) if (kv.second.tab) (void)hipFree(kv.second.tab);
    f->rs_filters.clear();
    if (f->rs_meta) (void)hipFree(f->rs_meta);
    f->rs_meta = nullptr; f->rs_cap = 0;
    if (f->rss_desc) (void)hipFree(f->rss_desc);
    f->rss_desc = nullptr;
}

extern "C" int64_t dsmi_resample_count(int method, int rate_in, int rate_out, int64_t n) {
    if (rate_in <= 0 || rate_out <= 0 || n < 0 || (method != DSMI_RESAMPLE_POLYPHASE && method != DSMI_RESAMPLE_RATECV)) return DSMI_ERR_INVALID;
    if (n == 0) return 0;
    const int g = std::gcd(rate_in, rate_out);
    const int64_t o = rate_out / g, i = rate_in / g;
    if (n > (INT64_MAX - i) / o) return DSMI_ERR_INVALID;
    return method == DSMI_RESAMPLE_RATECV ? ((n - 1) * o) / i + 1 : (n * o + i - 1) / i;
}

extern "C" int dsmi_resample_taps(int rate_in, int rate_out, double* taps_out, int64_t capacity, int* up, int* down) {
    Ratio r;
    if (const char* msg = poly_ratio(rate_in, rate_out, &r)) {
        fe_set_thread_error(msg);
        return rate_in <= 0 || rate_out <= 0 ? DSMI_ERR_INVALID : DSMI_ERR_CAPACITY;
    }
    if (taps_out && capacity < r.n_taps) { fe_set_thread_error("resample: taps_out is smaller than 20 * max(up, down) + 1"); return DSMI_ERR_CAPACITY; }
    if (up) *up = r.up;
    if (down) *down = r.down;
    if (taps_out) poly_taps(r, taps_out);
    return DSMI_OK;
}

extern "C" int dsmi_resample(dsmi_frontend* f, const void* pcm, int dtype, const int64_t* n_samples, int B, int rate_in, int method,
                             double* out, int64_t out_capacity, int64_t* n_out, void* stream) {
    if (!f) return DSMI_ERR_INVALID;
    auto bad = [&](int code, const char* msg) { f->err = msg; return code; };
    const int base = dtype & 15;
    const bool stereo_ok = base == DSMI_PCM_I16 || base == DSMI_PCM_I24 || base == DSMI_PCM_I32;
    if (!pcm || !n_samples || !out || !n_out || B < 1 || B > 65535 || out_capacity < 0 || dtype < 0 || base > DSMI_PCM_I32 ||
        (dtype & ~(15 | DSMI_PCM_STEREO)) || ((dtype & DSMI_PCM_STEREO) && !stereo_ok))
        return bad(DSMI_ERR_INVALID, "bad resample arguments (8-bit and float PCM cannot be stereo)");
    if (rate_in <= 0) return bad(DSMI_ERR_INVALID, "resample: rate_in must be positive");
    if (method != DSMI_RESAMPLE_POLYPHASE && method != DSMI_RESAMPLE_RATECV) return bad(DSMI_ERR_INVALID, "resample: unknown method");
    const bool floats = dtype == DSMI_PCM_F32 || dtype == DSMI_PCM_F64;
    if (method == DSMI_RESAMPLE_RATECV && floats) return bad(DSMI_ERR_INVALID, "resample: ratecv is defined on integer samples, not on float PCM");
    const int rate_out = f->desc.sample_rate;
    Ratio r;
    // both methods refuse absurd pairs; the cap also keeps ratecv's o = up below 2^21, which its exactness needs (|X| o < 2^53)
    if (const char* msg = poly_ratio(rate_in, rate_out, &r)) return bad(DSMI_ERR_CAPACITY, msg);
    const bool same = rate_in == rate_out;
    // ---- sizes: everything that can refuse the call comes before the first write or launch
    std::vector<int64_t> host(4 * (size_t)B), counts(B);
    int64_t off_in = 0, off_out = 0, max_cnt = 0;
    for (int b = 0; b < B; ++b) {
        if (n_samples[b] < 0) return bad(DSMI_ERR_INVALID, "resample: negative sample count");
        const int64_t c = dsmi_resample_count(method, rate_in, rate_out, n_samples[b]);
        if (c < 0 || off_out + c < off_out) return bad(DSMI_ERR_INVALID, "resample: sample count out of range");
        host[b] = off_in; host[B + b] = n_samples[b]; host[2 * (size_t)B + b] = off_out; host[3 * (size_t)B + b] = c;
        counts[b] = c; off_in += n_samples[b]; off_out += c; max_cnt = std::max(max_cnt, c);
    }
    if (off_out > out_capacity) return bad(DSMI_ERR_CAPACITY, "resample: out_dev is smaller than the clips' resampled lengths (dsmi_resample_count)");
    const int kmax = poly_kmax(r), kstride = poly_kstride(kmax);
    const size_t lds = poly_lds_bytes(r);
    if (method == DSMI_RESAMPLE_POLYPHASE && !same && lds > LDS_MAX) return bad(DSMI_ERR_CAPACITY, "resample: the input span of one workgroup does not fit LDS");
    if (max_cnt > (int64_t)INT32_MAX * 128) return bad(DSMI_ERR_INVALID, "resample: clip too long");
    if (hipSetDevice(f->device) != hipSuccess) return bad(DSMI_ERR_HIP, "hipSetDevice failed");
    hipStream_t s = (hipStream_t)stream;
    // ---- the filter of this rate_in: made once, kept on the handle
    const dsmi_resample_filter* flt = nullptr;
    if (method == DSMI_RESAMPLE_POLYPHASE && !same) {
        int code = DSMI_OK; const char* msg = nullptr;
        flt = fe_resample_filter(f, rate_in, r, &code, &msg);
        if (!flt) return bad(code, msg);
    }
    if (B > f->rs_cap) {
        if (f->rs_meta) { (void)hipStreamSynchronize(s); (void)hipFree(f->rs_meta); f->rs_meta = nullptr; f->rs_cap = 0; }
        if (hipMalloc((void**)&f->rs_meta, sizeof(int64_t) * 4 * (size_t)B) != hipSuccess) return bad(DSMI_ERR_NOMEM, "hipMalloc failed");
        f->rs_cap = B;
    }
    if (max_cnt > 0) {
        if (!fe_stage_copy(f, f->rs_meta, host.data(), 4 * B, s)) return bad(DSMI_ERR_HIP, "staging the clips' offsets / lengths failed");
        const dim3 grid((unsigned)((max_cnt + 255) / 256), B);
        if (same) {
            hipLaunchKernelGGL(resample_copy_kernel, grid, dim3(256), 0, s, pcm, dtype, f->rs_meta, B, out);
        } else if (method == DSMI_RESAMPLE_RATECV) {
            hipLaunchKernelGGL(resample_ratecv_kernel, grid, dim3(256), 0, s, pcm, dtype, f->rs_meta, B, r.down, r.up, ratecv_shift(dtype), out);
        } else {
            static_assert(OT == 256, "grid above counts 256 outputs per workgroup");
            hipLaunchKernelGGL(resample_poly_kernel, grid, dim3(OT), lds, s, pcm, dtype, f->rs_meta, B, flt->tab, flt->up, flt->down,
                               flt->half, flt->kmax, kstride, out);
        }
        if (hipGetLastError() != hipSuccess) return bad(DSMI_ERR_HIP, "resample kernel failed to launch");
    }
    std::copy(counts.begin(), counts.end(), n_out);
    return DSMI_OK;
}
