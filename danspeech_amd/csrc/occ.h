// CTC occupancy (occ.hip): for a candidate transcript, the posterior that frame t is emitted by token k (tok) or carries label c
// (occ), given the transcript -- alpha + beta over the candidate's trellis in float64.  Launched by dsmi_occupancy
// (ctc_tools.hip), which checks every argument and the feasibility of every candidate first (occ_check), orders the workgroups
// with score_plan and places each candidate's two stored trellises with alt_place (ctc_host.h).
#pragma once
#include "common.h"

namespace dsmi {

constexpr int kOccThreads = 256;

struct OccArgs {
    const float* probs;                 // [B][T_out][C] softmax probabilities
    int T_out, C, blank, N;
    const int32_t* sizes;               // [B] frames of each clip (<= T_out)
    const int32_t* order;               // [N] the workgroup of rank i works on candidate order[i]
    const int32_t* cand_clip;           // [N] the clip of each candidate
    const int32_t* tlen;                // [N] tokens of each candidate; -1 = infeasible, skipped
    const int32_t* targets;             // [N][L_stride] label ids, never the blank
    const int32_t* base;                // [N] where the candidate's trellises begin, in elements (alt_place)
    int L_stride;
    int S_max;                          // 2 * max(tlen) + 1 over the feasible candidates: the LDS carve's row stride
    // the stored trellises of a candidate with T frames and S = 2L + 1 states, [T][S] each from its base:
    double* fwd;                        // alpha_t(s)
    double* bwd;                        // beta_t(s) - lp(t, label(s))
    bool both;                          // occ or tok is asked for: false = the forward pass alone, for logp
    double* logp;                       // [N]
    double* occ;                        // [N][T_out][C], or null: written in full
    double* tok;                        // [N][T_out][L_stride], or null: written in full
};

size_t occ_lds_bytes(int S_max);
hipError_t launch_occ(const OccArgs& a, hipStream_t s);

}  // namespace dsmi
