// The conv kernels' frequency axis as pure functions (conv_split.hip, conv1_split.hip): which kernel rows of an output row read real
// input rows and which only the zero padding, and the order in which the workgroups take the output tiles.  Without a HIP include,
// like dense_tiles.h: the kernels execute it, tools/dense_tiles_replay.cpp replays it on the CPU (tests/test_conv_tiles_host.py).
#pragma once

#include "dense_tiles.h"

namespace dsmi {

// ---- kernel rows.  Output row f at kernel row kf reads input row sf * f - pf + kf; rows outside [0, fi) are padding, their products
// exact zeros.  The kernel rows that read a real row are one range: lo = max(0, pf - sf f), hi = min(kf - 1, fi - 1 + pf - sf f).
struct ConvRows { int lo, hi; };      // empty when lo > hi
DSMI_TILES_HD inline bool conv_rows_empty(const ConvRows& r) { return r.lo > r.hi; }
DSMI_TILES_HD inline ConvRows conv_rows_of(int f, int fi, int kf, int pf, int sf) {
    const int a = pf - sf * f, b = fi - 1 + a;
    ConvRows r;
    r.lo = a > 0 ? a : 0;
    r.hi = b < kf - 1 ? b : kf - 1;
    return r;
}
// A workgroup of `nf` output rows from f0: the range that holds the ranges of its live rows (f < fo); empty when it has none.  The
// kernels walk it with their barriers; a wave multiplies inside its own range only.
DSMI_TILES_HD inline ConvRows conv_rows_wg(int f0, int nf, int fo, int fi, int kf, int pf, int sf) {
    ConvRows u{kf, -1};
    for (int w = 0; w < nf && f0 + w < fo; ++w) {
        const ConvRows r = conv_rows_of(f0 + w, fi, kf, pf, sf);
        if (conv_rows_empty(r)) continue;
        if (r.lo < u.lo) u.lo = r.lo;
        if (r.hi > u.hi) u.hi = r.hi;
    }
    return u;
}

// ---- tiles.  A conv's output tiles are (z, t-tile, f-tile), z = clip x 32-channel tile; a GROUP is the f-tiles of one (z, t-tile):
// neighbours in f read overlapping input rows, so a group stays on one label (= XCD: its L2), back to back.  The linear order is
// t-tile, then z, then f-tile, and a label's share is whole groups (dense_tiles.h with unit = nf): with eight t-tiles label l walks
// t-tile l clip by clip, which is where the hardware puts the workgroups of the (t-tiles, f-tiles, z) grid the kernels launch in
// the static order.
struct ConvGrid { int nt, nf, nz; };
struct ConvTile { int tt, ft, z; };
DSMI_TILES_HD inline int conv_total(const ConvGrid& g) { return g.nt * g.nf * g.nz; }
DSMI_TILES_HD inline ConvTile conv_tile_at(const ConvGrid& g, int idx) {
    const int group = idx / g.nf;
    ConvTile t;
    t.ft = idx - group * g.nf;
    t.tt = group / g.nz;
    t.z = group - t.tt * g.nz;
    return t;
}
// the tile of `label`'s ticket (< dense_count(total, label, g.nf))
DSMI_TILES_HD inline ConvTile conv_tile_of(const ConvGrid& g, int label, int ticket) {
    return conv_tile_at(g, dense_base(conv_total(g), label, g.nf) + ticket);
}

}  // namespace dsmi
