// The order in which the dense kernels' workgroups take output tiles (gemm.hip): a pure function of the tile grid, the label of the
// drawing workgroup (blockIdx.x & 7: the workgroups that share an XCD) and the tickets it draws from eight counters.  Without a HIP
// include, like rnn_plan.h and gate_plan.h: the kernels execute it with device atomics, tools/dense_tiles_replay.cpp replays it on
// the CPU (tests/test_dense_tiles_host.py).
//
// Every label owns a contiguous share of the linear tile order -- ceil(total / 8) tiles, the last labels what is left of the total,
// possibly nothing: a partition for every total, also one that is no multiple of 8 -- and walks it front to back, which is the
// static order of the kernels (a W panel of `pn` units, inside it m-tile by m-tile, inside an m-tile the units of the panel: the
// panel stays in the XCD's L2).  A workgroup whose own share is used up draws from the label that has most left, until all eight
// are used up.  Nobody waits for anybody: a draw is one atomic add, a failed draw marks that label dead for this workgroup.
#pragma once

#if defined(__HIP__) || defined(__CUDACC__)
#define DSMI_TILES_HD __host__ __device__
#else
#define DSMI_TILES_HD
#endif

namespace dsmi {

constexpr int kDenseLabels = 8;
constexpr int kDenseCntStride = 64;                                    // words from one label's counter to the next: a 256-byte line each
constexpr int kDenseCntWords = (kDenseLabels + 1) * kDenseCntStride;   // ... and the line of the "done" word behind them

// mtiles x nunits output tiles; a unit is what one workgroup takes of N at a time (an n-tile, or a pair of them: the 128 x 256 form)
struct DenseGrid { int mtiles, nunits, pn; };      // pn: units of a W panel (>= 1)
struct DenseTile { int mt, nu; };

DSMI_TILES_HD inline int dense_total(const DenseGrid& g) { return g.mtiles * g.nunits; }
// (`unit`: tiles that stay together on one label -- a share is whole units; the conv kernels' f-neighbours, conv_rows.h.  `total` is a
// multiple of it.)
DSMI_TILES_HD inline int dense_share(int total, int unit = 1) { return (total / unit + kDenseLabels - 1) / kDenseLabels * unit; }
DSMI_TILES_HD inline int dense_base(int total, int label, int unit = 1) { return label * dense_share(total, unit); }
// tiles of `label`'s own share
DSMI_TILES_HD inline int dense_count(int total, int label, int unit = 1) {
    const int share = dense_share(total, unit), left = total - label * share;
    return left < 0 ? 0 : (left < share ? left : share);
}

// linear index (< total) -> tile: panel, then m-tile, then the unit inside the panel (the last panel may be narrower)
DSMI_TILES_HD inline DenseTile dense_tile_at(const DenseGrid& g, int idx) {
    const int per_panel = g.pn * g.mtiles;
    const int panel = idx / per_panel, rem = idx - panel * per_panel;
    const int left = g.nunits - panel * g.pn, pw = g.pn < left ? g.pn : left;
    DenseTile t;
    t.mt = rem / pw;
    t.nu = panel * g.pn + (rem - t.mt * pw);
    return t;
}
// the tile of `label`'s ticket (< dense_count(total, label))
DSMI_TILES_HD inline DenseTile tile_of(const DenseGrid& g, int label, int ticket) { return dense_tile_at(g, dense_base(dense_total(g), label) + ticket); }

// A ticket that `label`'s counter gave: the linear index of its tile, or -1 with the label marked dead (its share is used up).
DSMI_TILES_HD inline int dense_redeem(int total, int label, unsigned ticket, unsigned& dead, int unit = 1) {
    if (ticket < (unsigned)dense_count(total, label, unit)) return dense_base(total, label, unit) + (int)ticket;
    dead |= 1u << label;
    return -1;
}

// Draw from the other labels: the one with most left first (peek(l): the counter's value now, add(l): fetch-and-add 1).  -1: all used up.
// At most eight failed adds per workgroup and kernel, so a counter never exceeds its share by more than the workgroups of the launch.
template <class Add, class Peek>
DSMI_TILES_HD inline int dense_steal(int total, unsigned& dead, Add add, Peek peek, int unit = 1) {
    for (;;) {
        int best = -1, best_left = 0;
        for (int l = 0; l < kDenseLabels; ++l) {
            if ((dead >> l) & 1u) continue;
            const int cnt = dense_count(total, l, unit);
            const unsigned seen = peek(l);
            const int left = seen < (unsigned)cnt ? cnt - (int)seen : 0;
            if (left == 0) dead |= 1u << l;
            else if (left > best_left) { best = l; best_left = left; }
        }
        if (best < 0) return -1;
        const int idx = dense_redeem(total, best, add(best), dead, unit);
        if (idx >= 0) return idx;
    }
}

// One draw of a workgroup of `label`: its own share first, then the others'.  `dead` is the workgroup's own word, 0 at its start.
template <class Add, class Peek>
DSMI_TILES_HD inline int dense_draw(int total, int label, unsigned& dead, Add add, Peek peek, int unit = 1) {
    if (!((dead >> label) & 1u)) {
        const int idx = dense_redeem(total, label, add(label), dead, unit);
        if (idx >= 0) return idx;
    }
    return dense_steal(total, dead, add, peek, unit);
}

}  // namespace dsmi
