// The online picking rule of the streaming phrase watch (include/dsmi.h: dsmi_spot_stream_advance_many), ONE statement of it:
// spot_stream_kernel (spot_stream.hip) runs it in the registers of the thread that owns a phrase's last state, dsmi_spot_watch_pick
// runs it on the host over caller-supplied tracks, and tools/asan/host_fuzz.cpp (spotwatch) holds it to the rule written out plainly.
// No HIP, no allocation, no library call: a plain C++ compiler takes it.
#pragma once
#include <cstdint>

#include "../../include/dsmi.h"

#if defined(__HIPCC__)
#define DSMI_PICK_HD __host__ __device__ __forceinline__
#else
#define DSMI_PICK_HD inline
#endif

namespace dsmi {

using SpotPick = dsmi_spot_pick_state;      // {pending, ps, pe, last_end, pv}; a new utterance: {0, 0, 0, -1, 0.f}

DSMI_PICK_HD SpotPick spot_pick_fresh() { return SpotPick{0, 0, 0, -1, 0.f}; }

// Frame f (counted from the utterance's first frame) with E[f] = e and ST[f] = st.  At most one candidate fires per frame:
// emit(start, last, score, fired) with the window's frames [start, last], inclusive.
//   1. a pending candidate that has waited settle frames fires;
//   2. f is a candidate iff e > -inf, e >= min_mean_logp * (float)(f - st + 1) (dsmi_spot's float32 multiply) and st > last_end;
//   3. a candidate becomes pending, or replaces a pending one whose window it meets when it scores strictly more, or -- beyond
//      the pending window -- makes the pending one fire and becomes pending itself.
template <typename Emit>
DSMI_PICK_HD void spot_pick_frame(SpotPick& p, int f, float e, int st, float min_mean_logp, int settle, Emit&& emit) {
    if (p.pending && f - p.pe >= settle) {
        emit(p.ps, p.pe, p.pv, f);
        p.last_end = p.pe;
        p.pending = 0;
    }
    const bool cand = e > -__builtin_inff() && e >= min_mean_logp * (float)(f - st + 1) && st > p.last_end;
    if (!cand) return;
    if (p.pending) {
        if (st <= p.pe) {
            if (!(e > p.pv)) return;         // the windows meet: strictly better or the earlier one stays
        } else {
            emit(p.ps, p.pe, p.pv, f);
            p.last_end = p.pe;
        }
    }
    p.pending = 1; p.ps = st; p.pe = f; p.pv = e;
}

// The utterance ends after `frames` frames in all: what is pending fires with fired = frames.
template <typename Emit>
DSMI_PICK_HD void spot_pick_flush(SpotPick& p, int frames, Emit&& emit) {
    if (!p.pending) return;
    emit(p.ps, p.pe, p.pv, frames);
    p.last_end = p.pe;
    p.pending = 0;
}

// A chunk of tracks: E / ST [frames] of the frames t0 .. t0 + frames - 1, then the flush.  The first min(count, max_events)
// events go to hits [max_events][2] = [start, end), scores and fired; returns the count.
inline int spot_pick_chunk(SpotPick& p, const float* E, const int32_t* ST, int frames, int t0, bool flush, float min_mean_logp, int settle,
                           int max_events, int32_t* hits, float* scores, int32_t* fired) {
    int count = 0;
    auto emit = [&](int s, int e, float v, int at) {
        if (count < max_events) { hits[2 * count] = s; hits[2 * count + 1] = e + 1; scores[count] = v; fired[count] = at; }
        ++count;
    };
    for (int f = 0; f < frames; ++f) spot_pick_frame(p, t0 + f, E[f], ST[f], min_mean_logp, settle, emit);
    if (flush) spot_pick_flush(p, t0 + frames, emit);
    return count;
}

}  // namespace dsmi
