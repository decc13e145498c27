// Streaming phrase watch (spot_stream.hip): spot.hip's trellis carried from one chunk of a live session's probabilities to the
// next, for N sessions per launch, with the online picking rule (spot_pick.h) run beside it.  Launched by
// dsmi_spot_stream_advance_many (spot_watch.hip), which checks every argument first (spot_stream_check: ctc_host.h).
#pragma once
#include "common.h"
#include "ctc_host.h"
#include "spot_pick.h"

namespace dsmi {

// one stream of a launch.  Its state block: score [n_groups][kSpotThreads] floats, start [n_groups][kSpotThreads] ints, then
// pick [K]; read at the kernel's entry (not at all when t0 = 0: a new utterance holds -inf / -1 and a fresh picker) and
// written at its exit.
struct SpotStreamDesc {
    const float* probs;                 // [T][C] this call's frames (null when T = 0)
    float* score;
    int32_t* start;
    SpotPick* pick;
    int32_t T, t0, flush, pad;
};

struct SpotStreamArgs {
    const SpotStreamDesc* desc;         // [n]
    const int32_t* words;               // [n_groups][kSpotThreads] (spot_pack)
    int C, K, n_groups, max_events, settle, F_stride;
    float min_mean_logp;
    int32_t* hits;                      // [n][K][max_events][2]
    float* scores;                      // [n][K][max_events]
    int32_t* fired;                     // [n][K][max_events]
    int32_t* counts;                    // [n][K]
    float* E;                           // [n][K][F_stride] this call's frames, or null: no tracks
    int32_t* ST;
};

// one launch: n_groups x n workgroups
hipError_t launch_spot_stream(const SpotStreamArgs& a, int n, hipStream_t s);

}  // namespace dsmi
