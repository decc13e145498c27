// Batched edit distance (edit.hip): for each pair of token sequences the packed cost d << 16 | s of the minimum-distance alignment
// with the fewest substitutions, one wave per pair or two / four short pairs per wave.  Launched by dsmi_edit_distance
// (ctc_tools.hip), which checks every argument, answers the pairs with an empty side itself and packs the rest with edit_pack
// (edit_host.h).
#pragma once
#include "common.h"
#include "edit_host.h"

namespace dsmi {

struct EditArgs {
    const int32_t* lens;                // [M] tokens of each pool row
    const int32_t* pool;                // [M][L_stride] tokens, any int32
    int L_stride;
    const int32_t* pair_a;              // [n_launch] pool row of each pair's a, in launch order; both rows hold at least one token
    const int32_t* pair_b;              // [n_launch] ... of its b
    const int32_t* waves;               // [n_waves] first launch index | segment code << kEditSegShift | pairs << kEditCountShift
    int n_waves;
    int col_words;                      // LDS words per wave (the boundary column between two stripes), 0 = no pair has a second stripe
    uint32_t* packed;                   // [n_launch] D[La][Lb], in launch order
};

hipError_t launch_edit(const EditArgs& a, hipStream_t s);

}  // namespace dsmi
