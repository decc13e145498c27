// CTC transcript scoring (score.hip): the log likelihood of a label sequence summed over every CTC alignment, in float64, one
// workgroup per candidate.  Launched by dsmi_score (decoder.hip), which checks every argument and the feasibility of every
// candidate first and orders the workgroups with score_plan.
#pragma once
#include <algorithm>
#include <cstdint>

namespace dsmi {

// The launch order (host only): candidates with the most frames first (the longest chains start first), then by clip (the
// candidates of one clip run side by side and share the clip's probabilities in L2), then the most tokens first, then by index.
// Every entry of the three arrays is >= 0.  order[i] = the candidate workgroup i scores.  Returns N.
inline int score_plan(const int32_t* cand_clip, const int32_t* cand_frames, const int32_t* target_lens, int N, int32_t* order) {
    for (int n = 0; n < N; ++n) order[n] = n;
    std::sort(order, order + N, [&](int32_t x, int32_t y) {
        if (cand_frames[x] != cand_frames[y]) return cand_frames[x] > cand_frames[y];
        if (cand_clip[x] != cand_clip[y]) return cand_clip[x] < cand_clip[y];
        if (target_lens[x] != target_lens[y]) return target_lens[x] > target_lens[y];
        return x < y;
    });
    return N;
}

}  // namespace dsmi

// (the plan above needs no HIP: tools/asan/host_fuzz.cpp includes this header in a CPU build; the launch below does)
#ifdef __HIPCC__
#include "common.h"

namespace dsmi {

constexpr int kScoreThreads = 256;
constexpr int kScoreChunk = 16;         // frames of probabilities per prefetch (as align.hip)

struct ScoreArgs {
    const float* probs;                 // [B][T_out][C] softmax probabilities
    int T_out, C, blank;
    const int32_t* sizes;               // [B] frames of each clip (<= T_out)
    const int32_t* order;               // [N] workgroup i scores candidate order[i]
    const int32_t* cand_clip;           // [N] the clip of each candidate
    const int32_t* tlen;                // [N] tokens of each candidate; -1 = infeasible, skipped
    const int32_t* targets;             // [N][L_stride] label ids, never the blank
    int L_stride;
    int S_max;                          // 2 * max(tlen) + 1 over the scored candidates: the LDS carve's alpha stride
    double* logp;                       // [N]
};

size_t score_lds_bytes(int S_max);
hipError_t launch_score(const ScoreArgs& a, int N, hipStream_t s);

}  // namespace dsmi
#endif
