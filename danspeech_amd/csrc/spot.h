// CTC phrase search (spot.hip): for every (clip, phrase) the best path that emits exactly the phrase and ends at each frame,
// with the frame it began at, then the best disjoint occurrences.  Launched by dsmi_spot (ctc_tools.hip), which checks every
// argument first and packs the phrases into workgroups (spot_plan, spot_pack and the word flags: ctc_host.h).
#pragma once
#include "common.h"
#include "ctc_host.h"

namespace dsmi {

struct SpotArgs {
    const float* probs;                 // [B][T_out][C] softmax probabilities
    int T_out, C, K, n_groups;
    const int32_t* sizes;               // [B] frames of each clip (<= T_out)
    const int32_t* words;               // [n_groups][kSpotThreads]
    float* E;                           // [B][K][T_out] end scores
    int32_t* ST;                        // [B][K][T_out] start frames
    int max_hits;
    float min_mean_logp;
    int32_t* hits;                      // [B][K][max_hits][2]
    float* scores;                      // [B][K][max_hits]
    int32_t* counts;                    // [B][K]
};

// two launches: the trellis (n_groups x B workgroups), then the picking (K x B workgroups)
hipError_t launch_spot(const SpotArgs& a, int B, hipStream_t s);

}  // namespace dsmi
