// CTC transcript scoring (score.hip): the log likelihood of a label sequence summed over every CTC alignment, in float64, one
// workgroup per candidate.  Launched by dsmi_score (ctc_tools.hip), which checks every argument and the feasibility of every
// candidate first and orders the workgroups with score_plan (ctc_host.h).
#pragma once
#include "common.h"

namespace dsmi {

constexpr int kScoreThreads = 256;

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
