// Batched edit distance on the GPU (gfx950): for each pair (a, b) of token sequences the packed cost of the minimum-distance
// alignment with the fewest substitutions (the contract: include/dsmi.h).  Costs are uint32 d << 16 | s, a match adds 0, a
// substitution 0x10001, a deletion or an insertion 0x10000:
//     D[i][0] = i << 16, D[0][j] = j << 16, D[i][j] = min3(D[i-1][j] + DEL, D[i][j-1] + INS, D[i-1][j-1] + (a_i == b_j ? 0 : SUB))
// and the minimum of packed integers is the lexicographic minimum of (distance, substitutions).
//
// One wave per pair, or two / four pairs per wave in segments of 32 / 16 lanes (edit_pack, edit_host.h), in a skewed wavefront.
// Lane l of a segment owns column j = 64 * stripe + l + 1 of b, keeps b_j in a register, and computes cell (i = k - l, j) at
// step k.  Everything a step needs is in registers:
//     up    D[i-1][j]    the lane's own value of the step before;
//     left  D[i][j-1]    the left neighbour's value of the step before: the values move up one lane per step;
//     diag  D[i-1][j-1]  the left value received one step earlier;
//     a_i                moves up one lane per step beside the values (lane l - 1 compared a_i one step earlier).
// Lane 0 of a segment takes none of this from the lane below it, which belongs to another pair: its left and diagonal are the
// boundary column (i << 16 in stripe 0; in later stripes what lane 63 of the stripe before wrote to LDS, read one step ahead),
// and its a_i comes from a chunk of 16 tokens that the 16 lanes of its row loaded from global memory one chunk (16 steps)
// ahead and that moves DOWN one lane per step, so that the row's lane 0 always holds the token of the current step.
// The three moves are DPP lane shifts (full-rate VALU: wave_shr:1 twice, row_shl:1 once), so the step is 32-bit integer VALU
// work only; the form with ds_bpermute in their place is kept for the comparison (tools/exp/edit_time.py, experiments build).
// Waves of a workgroup are independent: no workgroup barrier anywhere.  The LDS holds only the boundary columns, sized by the
// longest a of the launch's pairs that have a second stripe.
#include "edit.h"

namespace dsmi {

// lane l receives v of lane l - 1 (lane 0 receives anything)
template <bool kDpp> __device__ __forceinline__ uint32_t edit_up1(uint32_t v, int up_addr) {
    if constexpr (kDpp) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, true);
    else return (uint32_t)__builtin_amdgcn_ds_bpermute(up_addr, (int)v);
}
// lane l receives v of lane l + 1 within its row of 16 lanes (a row's lane 15 receives anything)
template <bool kDpp> __device__ __forceinline__ uint32_t edit_down1(uint32_t v, int down_addr) {
    if constexpr (kDpp) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101 /* row_shl:1 */, 0xf, 0xf, true);
    else return (uint32_t)__builtin_amdgcn_ds_bpermute(down_addr, (int)v);
}

struct EditLane {                       // what a lane keeps from stripe to stripe
    const int32_t *a0, *b0;             // its pair's rows of the pool
    int La, Lb, ls;                     // its pair's lengths; its lane within the segment
    bool lane0, lane63;                 // the segment's first lane; the wave's last lane
    int up_addr, down_addr;             // (ds_bpermute form) where the lane below / the row's next lane sits
};

// One stripe of 64 columns (st; the only one of a 16- or 32-lane segment): returns the lane's D[La][j].  kFirst: stripe 0, the
// boundary column is i << 16; otherwise it is read from col.  kMore: another stripe follows, lane 63 writes its column to col.
template <bool kDpp, bool kFirst, bool kMore>
__device__ __forceinline__ uint32_t edit_stripe(const EditLane& e, int st, int K, int La_max, uint32_t* col) {
    const int j = 64 * st + e.ls + 1, row_lane = e.ls & 15;
    const uint32_t bj = (uint32_t)(j <= e.Lb ? e.b0[j - 1] : 0);
    uint32_t val = (uint32_t)j << 16;                        // D[0][j]
    uint32_t diag = (uint32_t)(j - 1) << 16;                 // D[0][j-1]
    uint32_t av = 0;
    uint32_t colv = kFirst ? 0u : col[1];                    // D[1][64 * st], for step 1
    int32_t nxt = row_lane < e.La ? e.a0[row_lane] : 0;
    for (int k0 = 0; k0 < K; k0 += 16) {
        uint32_t chunk = (uint32_t)nxt;                      // a_{k0 + 1 + row_lane}
        const int ix = k0 + 16 + row_lane;
        nxt = ix < e.La ? e.a0[ix] : 0;
        // always 16 steps, unrolled, so that the wait for the chunk fetched above falls behind them: in a step past K no cell
        // of the pair is left to compute (every lane that owns a column is beyond row La)
#pragma unroll
        for (int k = k0 + 1; k <= k0 + 16; ++k) {
            uint32_t left = edit_up1<kDpp>(val, e.up_addr);
            const uint32_t ain = edit_up1<kDpp>(av, e.up_addr);
            const uint32_t bnd = kFirst ? (uint32_t)k << 16 : colv;      // D[k][64 * st]
            if (!kFirst) colv = col[min(k + 1, La_max)];                  // (one step ahead)
            left = e.lane0 ? bnd : left;
            av = e.lane0 ? chunk : ain;
            const int i = k - e.ls;
            const uint32_t sub = diag + (av == bj ? 0u : kEditSub);
            const uint32_t c = min(min(val + kEditIndel, left + kEditIndel), sub);
            diag = left;
            const bool on = (unsigned)(i - 1) < (unsigned)e.La;
            val = on ? c : val;
            chunk = edit_down1<kDpp>(chunk, e.down_addr);
            if (kMore && e.lane63 && on) col[i] = val;
        }
    }
    return val;
}

template <bool kDpp> __global__ void __launch_bounds__(64 * kEditWavesPerBlock) edit_kernel(EditArgs a) {
    extern __shared__ uint32_t edit_cols[];      // [kEditWavesPerBlock][col_words]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int w = blockIdx.x * kEditWavesPerBlock + wv;
    if (w >= a.n_waves) return;                  // (wave-uniform; no barrier follows)
    const uint32_t word = (uint32_t)__builtin_amdgcn_readfirstlane(a.waves[w]);      // (the same for the wave: scalar loops below)
    const int first = (int)(word & 0xffffffu), code = (int)(word >> kEditSegShift) & 3, cnt = (int)(word >> kEditCountShift) & 7;
    const int seg = 16 << code, q = lane >> (4 + code);
    const bool live = q < cnt;
    EditLane e;
    e.ls = lane & (seg - 1); e.lane0 = e.ls == 0; e.lane63 = lane == 63;
    e.up_addr = ((lane + 63) & 63) << 2; e.down_addr = ((lane & 48) | ((lane + 1) & 15)) << 2;
    e.La = 0; e.Lb = 0; e.a0 = a.pool; e.b0 = a.pool;
    if (live) {
        const int ra = a.pair_a[first + q], rb = a.pair_b[first + q];
        e.La = a.lens[ra]; e.Lb = a.lens[rb];
        e.a0 = a.pool + (size_t)ra * a.L_stride; e.b0 = a.pool + (size_t)rb * a.L_stride;
    }
    // wave-uniform: the longest a of the wave's pairs; the stripes (a wave of one 64-lane segment only)
    const int La_max = max(max(__builtin_amdgcn_readlane(e.La, 0), __builtin_amdgcn_readlane(e.La, 16)),
                           max(__builtin_amdgcn_readlane(e.La, 32), __builtin_amdgcn_readlane(e.La, 48)));
    const int Lb_u = __builtin_amdgcn_readlane(e.Lb, 0);
    const int stripes = code == 2 ? (Lb_u + 63) >> 6 : 1;
    uint32_t* col = edit_cols + (size_t)wv * a.col_words;

    // a stripe's last step: its last lane with a column at row La_max
    uint32_t val;
    if (stripes == 1) {
        val = edit_stripe<kDpp, true, false>(e, 0, La_max + (code == 2 ? Lb_u : seg) - 1, La_max, col);
    } else {
        edit_stripe<kDpp, true, true>(e, 0, La_max + 63, La_max, col);
        for (int st = 1; st + 1 < stripes; ++st) edit_stripe<kDpp, false, true>(e, st, La_max + 63, La_max, col);
        val = edit_stripe<kDpp, false, false>(e, stripes - 1, La_max + Lb_u - 64 * (stripes - 1) - 1, La_max, col);
    }
    if (live && e.ls == ((e.Lb - 1) & 63)) a.packed[first + q] = val;
}

template <bool kDpp> static hipError_t launch_edit_form(const EditArgs& a, hipStream_t s) {
    const size_t lds = sizeof(uint32_t) * kEditWavesPerBlock * (size_t)a.col_words;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(edit_kernel<kDpp>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int blocks = (a.n_waves + kEditWavesPerBlock - 1) / kEditWavesPerBlock;
    hipLaunchKernelGGL(edit_kernel<kDpp>, dim3(blocks), dim3(64 * kEditWavesPerBlock), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_edit(const EditArgs& a, hipStream_t s) {
#ifdef DSMI_EXPERIMENTS
    // DSMI_DEBUG_EDIT_MOVE=bpermute: the three lane moves of a step through ds_bpermute (measured, not adopted: DESIGN.md)
    const char* form = exp_env("DSMI_DEBUG_EDIT_MOVE");
    if (form && std::string(form) == "bpermute") return launch_edit_form<false>(a, s);
#endif
    return launch_edit_form<true>(a, s);
}

}  // namespace dsmi
