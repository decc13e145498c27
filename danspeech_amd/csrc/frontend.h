// What features.hip and resample.hip share: the handle behind dsmi_frontend*, its pinned staging ring, and the one decode of a
// PCM sample (sample width, 8-bit bias, saturating stereo fold) every front-end kernel reads its input through.
#pragma once
#include "common.h"

#include <map>

// One cached polyphase filter of a frontend: rate_in -> sampling_rate (resample.hip).
struct dsmi_resample_filter {
    int up = 0, down = 0, half = 0, kmax = 0;    // kmax = ceil((2 half + 1) / up): taps of one output
    double* tab = nullptr;                       // device [up][kmax]: tab[r][t] = h[r + t up] (0 past the filter's end)
};

// The handle behind dsmi_frontend* : one SpectrogramAudioParser on one GPU.
struct dsmi_frontend {
    dsmi_frontend_desc desc{};
    int device = 0;
    int n_fft = 0, hop = 0, n_freq = 0;
    std::string err;
    double* tw = nullptr;    // [n_fft][2] cos, sin
    double* win = nullptr;   // [n_fft]
    int64_t* offs = nullptr; // device: per-clip sample offset, n_samples [2][cap], then float64 partial statistics [cap][NSL][2]
    int cap = 0;
    // pinned staging of the per-batch offsets / lengths (an async copy must not read pageable memory that is gone or
    // overwritten when the copy engine gets to it): a ring of slots, each reused only after its copy has completed
    static constexpr int kStage = 4;
    int64_t* stage = nullptr; int stage_cap = 0, stage_next = 0;
    hipEvent_t stage_ev[kStage] = {nullptr, nullptr, nullptr, nullptr}; bool stage_used[kStage] = {false, false, false, false};
    // dsmi_resample: the filters made so far (one per rate_in) and the clips' [4][rs_cap] offsets / counts on the device
    std::map<int, dsmi_resample_filter> rs_filters;
    int64_t* rs_meta = nullptr; int rs_cap = 0;
    // dsmi_resampler_push_many: the sessions' descriptor table on the device, sized for DSMI_RESAMPLE_STREAM_MAX sessions (resample_stream.hip)
    int64_t* rss_desc = nullptr;
    // dsmi_endpointer_push_many: the device table (sessions, then kernel 2's copies) and the pinned per-buffer sums (endpoint.hip)
    int64_t* ep_tab = nullptr; int64_t ep_tab_cap = 0;
    uint64_t* ep_sums = nullptr; int64_t ep_sums_cap = 0;
};

// host[0..n) -> dev[0..n) on stream s through the frontend's pinned ring (features.hip)
bool fe_stage_copy(dsmi_frontend* f, int64_t* dev, const int64_t* host, int n, hipStream_t s);
// makes the ring's slots at least n words each now (growing it waits for the whole device): a caller that knows its largest table
// grows the ring once, on first use, and never on a later call (features.hip)
bool fe_stage_reserve(dsmi_frontend* f, int n);
// the message dsmi_frontend_last_error(NULL) returns on this thread: failures of calls that have no handle (features.hip)
void fe_set_thread_error(const char* msg);
// frees what dsmi_resample and dsmi_resampler_push_many keep on the handle (resample.hip; the device is current and idle)
void fe_resample_release(dsmi_frontend* f);
// frees what dsmi_endpointer_push_many keeps on the handle (endpoint.hip; the device is current and idle)
void fe_endpoint_release(dsmi_frontend* f);

namespace dsmi {

// One integer sample of a WAV frame stream (resources.py:551-554 for the 8-bit bias).
__device__ __forceinline__ int64_t ld_int(const void* p, int base, int64_t i) {
    switch (base) {
        case DSMI_PCM_I16: return ((const int16_t*)p)[i];
        case DSMI_PCM_U8: return (int64_t)((const uint8_t*)p)[i] - 128;
        case DSMI_PCM_I32: return ((const int32_t*)p)[i];
        default: {
            const uint8_t* q = (const uint8_t*)p + 3 * i;
            const int32_t v = (int32_t)q[0] | ((int32_t)q[1] << 8) | ((int32_t)q[2] << 16);
            return v >= (1 << 23) ? v - (1 << 24) : v;
        }
    }
}

// Sample i of a clip at its integer scale as float64 (load_audio, resources.py:630-640); two channels fold
// into the saturating sum of audioop.tomono(buf, width, 1, 1) (resources.py:302-303).
__device__ __forceinline__ double ld_sample(const void* p, int dtype, int64_t i) {
    if (dtype == DSMI_PCM_F64) return ((const double*)p)[i];
    if (dtype == DSMI_PCM_F32) return (double)((const float*)p)[i];
    const int base = dtype & 15;
    if (!(dtype & DSMI_PCM_STEREO)) return (double)ld_int(p, base, i);
    const int64_t lim = base == DSMI_PCM_I16 ? (1ll << 15) : (base == DSMI_PCM_I24 ? (1ll << 23) : (1ll << 31));
    const int64_t v = ld_int(p, base, 2 * i) + ld_int(p, base, 2 * i + 1);
    return (double)(v < -lim ? -lim : (v > lim - 1 ? lim - 1 : v));
}

}  // namespace dsmi
