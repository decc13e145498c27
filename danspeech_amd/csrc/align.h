// CTC forced alignment (align.hip): the Viterbi path of a fixed label sequence through the CTC trellis, one workgroup per
// clip.  Launched by dsmi_align (ctc_tools.hip), which checks every argument and the feasibility of every clip first.
#pragma once
#include "common.h"

namespace dsmi {

constexpr int kAlignThreads = 256;
constexpr int kAlignTile = 64;          // frames per backtrace tile: 64 steps lower the state by at most 126
constexpr int kAlignTileCols = 33;      // dwords per tile row: 132 bytes hold states s - 126 .. s from a 4-byte aligned start

struct AlignArgs {
    const float* probs;                 // [B][T_out][C] softmax probabilities
    int T_out, C, blank;
    const int32_t* sizes;               // [B] frames of each clip (<= T_out)
    const int32_t* tlen;                // [B] tokens of each clip; -1 = infeasible, skipped
    const int32_t* targets;             // [B][L_stride] label ids, never the blank
    int L_stride;
    int S_max;                          // 2 * max(tlen) + 1 over the aligned clips: the LDS carve's alpha stride
    unsigned char* bp;                  // [B][T_out][S_stride] backpointers (0, 1, 2), + kAlignBpSlack bytes
    int S_stride;                       // multiple of 4
    int32_t* spans;                     // [B][L_stride][2] frames [start, end) of each token
    float* token_probs;                 // [B][L_stride]
    float* path_logp;                   // [B]
};

constexpr size_t kAlignBpSlack = 256;   // a tile row reads up to 132 bytes from its start column: past the last row, too

size_t align_lds_bytes(int S_max);
hipError_t launch_align(const AlignArgs& a, int B, hipStream_t s);

}  // namespace dsmi
