// CTC token confidence (alt.hip): for every token of a candidate transcript, the log likelihood of the transcript with that
// token replaced by each other label, or deleted -- a forward-backward pass over the candidate's trellis in float64.  Launched by
// dsmi_alternatives (ctc_tools.hip), which checks every argument and the feasibility of every candidate first, orders the
// workgroups with score_plan and places each candidate's stored trellises with alt_place (ctc_host.h).
#pragma once
#include "common.h"

namespace dsmi {

constexpr int kAltThreads = 256;

struct AltArgs {
    const float* probs;                 // [B][T_out][C] softmax probabilities
    int T_out, C, blank;
    const int32_t* sizes;               // [B] frames of each clip (<= T_out)
    const int32_t* order;               // [N] the workgroups of rank i work on candidate order[i]
    const int32_t* cand_clip;           // [N] the clip of each candidate
    const int32_t* tlen;                // [N] tokens of each candidate; -1 = infeasible, skipped
    const int32_t* targets;             // [N][L_stride] label ids, never the blank
    const int32_t* base;                // [N] where the candidate's trellises begin, in elements (alt_place)
    int L_stride;
    int S_max;                          // 2 * max(tlen) + 1 over the feasible candidates: the LDS carve's row stride
    int n_blocks;                       // slot workgroups per candidate: ceil(max(tlen) * C / kAltThreads)
    // the stored trellises of a candidate with T frames, L tokens, S = 2L + 1 states, each from its base:
    double* fwd;                        // [T][L][2]: alpha_t(2k), logsumexp(alpha_t(2k), alpha_t(2k-1))          at base
    double* bwd;                        // [T][S]: beta_t(s)                                                       at base
    double* bwd_pair;                   // [T][L]: logsumexp(beta_t(2k+2), beta_t(2k+3)), rows 1 .. T-1            at base / 2
    double* logp;                       // [N]
    double* alt;                        // [N][L_stride][C]; rows k < tlen of feasible candidates are written
};

size_t alt_lds_bytes(int S_max);
hipError_t launch_alt(const AltArgs& a, int N, hipStream_t s);

}  // namespace dsmi
