// CTC phrase search (spot.hip): for every (clip, phrase) the best path that emits exactly the phrase and ends at each frame,
// with the frame it began at, then the best disjoint occurrences.  Launched by dsmi_spot (decoder.hip), which checks every
// argument first and packs the phrases into workgroups with spot_plan.
#pragma once
#include "common.h"

namespace dsmi {

constexpr int kSpotThreads = 256;       // one state per thread: a group of phrases holds at most this many states
constexpr int kSpotChunk = 16;          // frames of probabilities per prefetch (as align.hip)

// per-state word of a group, [n_groups][kSpotThreads]: label in the low byte, then
constexpr int kSpotSkip = 1 << 8;       // even state >= 2 whose token differs from the token before: s-2 competes
constexpr int kSpotFirst = 1 << 9;      // state 0 of a phrase: always restarts, never looks at s-1 / s-2 (the neighbouring phrase)
constexpr int kSpotLast = 1 << 10;      // state S-1 of a phrase: writes the tracks of phrase (word >> kSpotPhraseShift)
constexpr int kSpotLive = 1 << 11;      // a state at all (the tail of a group is dead)
constexpr int kSpotPhraseShift = 16;

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

// The packing (host only): phrases in order, S = 2 * len - 1 states each, a phrase that does not fit the group's kSpotThreads
// states opens the next group.  group_of[k], first_state[k] = where phrase k's state 0 sits.  Returns the number of groups.
inline int spot_plan(const int32_t* lens, int K, int32_t* group_of, int32_t* first_state) {
    int g = 0, used = 0;
    for (int k = 0; k < K; ++k) {
        const int S = 2 * lens[k] - 1;
        if (used + S > kSpotThreads) { ++g; used = 0; }
        group_of[k] = g;
        first_state[k] = used;
        used += S;
    }
    return g + 1;
}

// two launches: the trellis (n_groups x B workgroups), then the picking (K x B workgroups)
hipError_t launch_spot(const SpotArgs& a, int B, hipStream_t s);

}  // namespace dsmi
