// The host half of dsmi_align_long (ctc_tools.hip; the kernels: align_long.hip): the geometry of a call and the check of what a
// caller hands in.  No HIP: a plain C++ compiler takes it, and tools/asan/host_fuzz.cpp (alignlong) runs it under ASan + UBSan on
// exactly sized arrays.  What the numbers alone refuse is refused before any array is read.
#pragma once
#include "ctc_host.h"

namespace dsmi {

// One forward launch advances every state by kAlongF frames; one workgroup of it owns kAlongW states and recomputes the 2 * kAlongF
// states to their left (a state moves right by at most two per frame), so its LDS rows hold kAlongW + 2 * kAlongF = 512 states:
// two per thread.  DESIGN.md ("Long-form alignment") has the budget and the geometries that were timed beside this one.
constexpr int kAlongW = 384;            // states a forward workgroup stores
constexpr int kAlongF = 64;             // frames per forward launch and per backtrace window
static_assert((kAlongW + 2 * kAlongF) % 256 == 0, "whole rounds of the workgroup's threads");

struct AlongPlan {
    int64_t W, F, state_tiles, frame_tiles, rows, bytes;
};

// T >= 1, L >= 0.  Checkpoint row j holds alpha of frame min(j * F, T - 1): row 0 is frame 0, frame tile j leads from row j to
// row j + 1, the last row is frame T - 1.
inline AlongPlan align_long_geometry(int64_t T, int64_t L, int W = kAlongW, int F = kAlongF) {
    AlongPlan p;
    const int64_t S = 2 * L + 1;
    p.W = W;
    p.F = F;
    p.state_tiles = (S + W - 1) / W;
    p.frame_tiles = (T - 1 + F - 1) / F;
    p.rows = p.frame_tiles + 1;
    p.bytes = p.rows * S * (int64_t)sizeof(float);
    return p;
}

// the numbers of a call: DSMI_OK with *plan filled, or the refusal with nothing written
inline int align_long_numbers(int T, int L, int lead_free, int tail_free, AlongPlan* plan, std::string& err) {
    if (T <= 0 || L < 0) return ctc_refuse(err, DSMI_ERR_INVALID, "align_long: T must be positive and L not negative");
    if ((lead_free != 0 && lead_free != 1) || (tail_free != 0 && tail_free != 1))
        return ctc_refuse(err, DSMI_ERR_INVALID, "align_long: lead_free and tail_free are 0 or 1");
    if (L > DSMI_ALIGN_LONG_MAX_TOKENS)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "align_long: L " + std::to_string(L) + " exceeds DSMI_ALIGN_LONG_MAX_TOKENS (" + std::to_string(DSMI_ALIGN_LONG_MAX_TOKENS) + ")");
    if (T > DSMI_ALIGN_LONG_MAX_FRAMES)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "align_long: T " + std::to_string(T) + " exceeds DSMI_ALIGN_LONG_MAX_FRAMES (" + std::to_string(DSMI_ALIGN_LONG_MAX_FRAMES) + ")");
    const AlongPlan p = align_long_geometry(T, L);
    if (p.bytes > (int64_t)DSMI_ALIGN_LONG_MAX_WORKSPACE)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "align_long: the checkpoint rows, " + std::to_string(p.rows) + " of " + std::to_string(2 * (int64_t)L + 1) +
                          " floats, exceed DSMI_ALIGN_LONG_MAX_WORKSPACE (" + std::to_string(p.bytes) + " bytes)");
    *plan = p;
    return DSMI_OK;
}

// dsmi_align_long_plan: info [6]
inline int align_long_plan(int T, int L, int64_t* info) {
    AlongPlan p;
    std::string err;
    if (int rc = align_long_numbers(T, L, 0, 0, &p, err)) return rc;
    info[0] = p.W; info[1] = p.F; info[2] = p.state_tiles; info[3] = p.frame_tiles; info[4] = p.rows; info[5] = p.bytes;
    return DSMI_OK;
}

constexpr CtcRows kAlongRows{"align_long", "transcript", "target length", "target id", "DSMI_ALIGN_LONG_MAX_TOKENS", 0, DSMI_ALIGN_LONG_MAX_TOKENS};

// A whole call behind its null-pointer checks: targets [L].  *feasible = whether the transcript fits the frames (dsmi_align's rule).
inline int align_long_check(int T, int L, int lead_free, int tail_free, const int32_t* targets, int C, int blank, AlongPlan* plan,
                            bool* feasible, std::string& err) {
    if (int rc = align_long_numbers(T, L, lead_free, tail_free, plan, err)) return rc;
    int repeats = 0;
    if (int rc = ctc_check_row(kAlongRows, 0, targets, L, L, C, blank, &repeats, err)) return rc;
    *feasible = ctc_feasible_len(L, repeats, T) >= 0;
    return DSMI_OK;
}

}  // namespace dsmi
