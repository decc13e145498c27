// Long-form CTC forced alignment (align_long.hip): dsmi_align's Viterbi path for one recording whose trellis fits neither one
// workgroup's LDS nor a stored backpointer table.  Launched by dsmi_align_long (ctc_tools.hip), which checks every argument and
// the feasibility first; the geometry is align_long_host.h's.
#pragma once
#include "common.h"
#include "align_long_host.h"

namespace dsmi {

constexpr int kAlongThreads = 256;

struct AlongArgs {
    const float* probs;                 // [T][C] softmax probabilities
    int T, C, blank, L, S;              // S = 2L + 1
    int lead_free, tail_free;
    const int32_t* targets;             // [L] label ids, never the blank
    float* rows;                        // [frame tiles + 1][S] checkpoints: row j = alpha of frame min(j * kAlongF, T - 1)
    int W, F, frame_tiles, state_tiles; // align_long_host.h's plan
    int32_t* spans;                     // [L][2] frames [start, end) of each token, zeroed before the launch
    float* token_probs;                 // [L]
    float* path_logp;                   // [1]
};

// row 0, the forward launches in frame order, the backtrace, the token means: all on `s`, no signalling inside a launch
hipError_t launch_align_long(const AlongArgs& a, hipStream_t s);

}  // namespace dsmi
