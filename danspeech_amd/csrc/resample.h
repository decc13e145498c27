// What resample.hip (dsmi_resample: whole clips) and resample_stream.hip (dsmi_resampler_*: an utterance in chunks) share, all
// of it host code: the rate pair's up / down and its refusals, scipy.signal.resample_poly's tap design, the layout of the
// per-phase tap table on the device, and the frontend's cache of those tables (one per rate_in).
#pragma once
#include "common.h"
#include "frontend.h"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace dsmi {

constexpr int RS_OT = 256;                 // outputs per workgroup (one per thread) of both polyphase kernels
constexpr size_t RS_LDS_MAX = 64 * 1024;   // the staged input span must fit: guaranteed by DSMI_RESAMPLE_MAX_DECIMATION (checked)

// I0(x), 0 <= x: the power series (every term positive: no cancellation)
inline double bessel_i0(double x) {
    const double t = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= t / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

struct Ratio { int up, down; int64_t half, n_taps; };

// up / down of rate_in -> rate_out and the filter's size; the message of a refusal, or nullptr
inline const char* poly_ratio(int rate_in, int rate_out, Ratio* r) {
    if (rate_in <= 0 || rate_out <= 0) return "resample: rates must be positive";
    const int g = std::gcd(rate_in, rate_out);
    r->up = rate_out / g; r->down = rate_in / g;
    r->half = 10 * (int64_t)std::max(r->up, r->down);
    r->n_taps = 2 * r->half + 1;
    if (r->n_taps > DSMI_RESAMPLE_MAX_TAPS) return "resample: the filter of this rate pair has more than DSMI_RESAMPLE_MAX_TAPS taps";
    if ((int64_t)rate_in > (int64_t)DSMI_RESAMPLE_MAX_DECIMATION * rate_out) return "resample: rate_in above DSMI_RESAMPLE_MAX_DECIMATION x rate_out";
    return nullptr;
}

// scipy.signal.resample_poly's default filter: firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)) * up
inline void poly_taps(const Ratio& r, double* h) {
    // fc * sinc(fc * m) with fc = 1 / max(up, down) rounded first, as firwin does: the taps on the sinc's zeros are nothing but the
    // rounding of that argument, and only the same argument gives the same taps there
    const double pi = 3.14159265358979323846, fc = 1.0 / (double)std::max(r.up, r.down), i0b = bessel_i0(5.0);
    long double sum = 0.0L;
    for (int64_t m = -r.half; m <= r.half; ++m) {
        const double y = pi * (fc * (double)m);
        const double sinc = m == 0 ? 1.0 : std::sin(y) / y;
        const double a = (double)m / (double)r.half;
        const double w = bessel_i0(5.0 * std::sqrt(std::max(0.0, 1.0 - a * a))) / i0b;
        const double v = fc * sinc * w;
        h[m + r.half] = v;
        sum += (long double)v;
    }
    const double scale = (double)((long double)r.up / sum);
    for (int64_t k = 0; k < r.n_taps; ++k) h[k] *= scale;
}

// ratecv works at the file's sample width: samples are shifted up to 32 bits, interpolated, and shifted back
inline int ratecv_shift(int dtype) {
    switch (dtype & 15) {
        case DSMI_PCM_U8: return 24;
        case DSMI_PCM_I16: return 16;
        case DSMI_PCM_I24: return 8;
        default: return 0;
    }
}

// The table's layout: tab[r][t] = h[r + t up], r = (j down + half) mod up, t = 0 .. kmax - 1, rows of kstride doubles (even: a
// row starts on 16 bytes).  Output j reads x[k_hi(j) - t] against tab[r][t], k_hi(j) = (j down + half) / up.
inline int poly_kmax(const Ratio& r) { return (int)((r.n_taps + r.up - 1) / r.up); }
inline int poly_kstride(int kmax) { return (kmax + 1) & ~1; }
// dynamic LDS of a workgroup of RS_OT outputs: its input span as float64
inline size_t poly_lds_bytes(const Ratio& r) {
    return sizeof(double) * ((size_t)(((int64_t)(RS_OT - 1) * r.down + r.up - 1) / r.up) + poly_kmax(r) + 1);
}

// The filter of rate_in on the frontend: made once (host taps, one upload), kept on the handle.  nullptr and *code / *msg on failure.
// The device is current.
inline const dsmi_resample_filter* fe_resample_filter(dsmi_frontend* f, int rate_in, const Ratio& r, int* code, const char** msg) {
    auto it = f->rs_filters.find(rate_in);
    if (it == f->rs_filters.end()) {
        const int kmax = poly_kmax(r), kstride = poly_kstride(kmax);
        std::vector<double> h(r.n_taps), tab((size_t)r.up * kstride, 0.0);
        poly_taps(r, h.data());
        for (int ph = 0; ph < r.up; ++ph)
            for (int t = 0; t < kmax; ++t) {
                const int64_t idx = ph + (int64_t)t * r.up;
                if (idx < r.n_taps) tab[(size_t)ph * kstride + t] = h[idx];
            }
        dsmi_resample_filter nf;
        nf.up = r.up; nf.down = r.down; nf.half = (int)r.half; nf.kmax = kmax;
        if (hipMalloc((void**)&nf.tab, sizeof(double) * tab.size()) != hipSuccess) { *code = DSMI_ERR_NOMEM; *msg = "hipMalloc failed"; return nullptr; }
        if (hipMemcpy(nf.tab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(nf.tab);
            *code = DSMI_ERR_HIP; *msg = "uploading the resampling filter failed";
            return nullptr;
        }
        it = f->rs_filters.emplace(rate_in, nf).first;
    }
    return &it->second;       // (std::map: the address stays put while other filters are added)
}

}  // namespace dsmi
