// The order in which the dense kernels' workgroups take output tiles (gemm.hip, conv_split.hip, conv1_split.hip): a pure function of
// the tile grid, the label of the drawing workgroup (blockIdx.x & 7: the workgroups that share an XCD) and the tickets it draws from
// eight counters -- and the workgroup's whole side of the hand-out, TileTaker: first draw, early request, redeem or steal, leave and
// reset.  Without a HIP include, like rnn_plan.h and gate_plan.h: the kernels run TileTaker over device atomics (TileCounters, the
// one place that touches the counters), tools/dense_tiles_replay.cpp runs the same steps over plain words on the CPU
// (tests/test_dense_tiles_host.py, tests/test_conv_tiles_host.py).
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

// ---- the workgroup's side.  `C` is the launch's counters: add(l) fetch-and-add 1 on label l's counter, peek(l) its value now,
// done() fetch-and-add 1 on the "done" word, zero(l) store 0 to word l (l == kDenseLabels: the "done" word), workgroups() how many
// the launch has (asked behind done(): on the device it is a load, which so stays where the kernels had it).  One lane of the
// workgroup runs the steps: first() at its start, then per tile ask() in front of the tile's stores and next() behind them -- the
// request's way to memory and back lies under the stores --, and tiles_leave() once it has drawn -1.
struct TileTaker {
    int total, label, unit;     // `unit`: see dense_share
    unsigned& dead;             // the labels this workgroup has found used up: the workgroup's own word, 0 at its start
    bool asked;                 // ask() has drawn from the own counter ...
    unsigned ticket;            // ... this, until next() redeems it

    // (the kernels make one per tile over the same `dead`, so that request and ticket do not live in registers from one tile to the next)
    DSMI_TILES_HD TileTaker(int total_, int label_, int unit_, unsigned& dead_) : total(total_), label(label_), unit(unit_), dead(dead_), asked(false), ticket(0) {}

    // Draw from the other labels: the one with most left first.  -1: all used up.  At most eight failed adds per workgroup and
    // kernel, so a counter never exceeds its share by more than the workgroups of the launch.
    template <class C>
    DSMI_TILES_HD int steal(C& c) {
        for (;;) {
            int best = -1, best_left = 0;
            for (int l = 0; l < kDenseLabels; ++l) {
                if ((dead >> l) & 1u) continue;
                const int cnt = dense_count(total, l, unit);
                const unsigned seen = c.peek(l);
                const int left = seen < (unsigned)cnt ? cnt - (int)seen : 0;
                if (left == 0) dead |= 1u << l;
                else if (left > best_left) { best = l; best_left = left; }
            }
            if (best < 0) return -1;
            const int idx = dense_redeem(total, best, c.add(best), dead, unit);
            if (idx >= 0) return idx;
        }
    }
    // the early request: a ticket of the own label, unless its share is known to be used up
    template <class C>
    DSMI_TILES_HD void ask(C& c) {
        if (!((dead >> label) & 1u)) { asked = true; ticket = c.add(label); }
    }
    // the next tile's linear index (-1: none left): what ask() was given, else from the others
    template <class C>
    DSMI_TILES_HD int next(C& c) {
        unsigned d = dead;      // (on a copy: the device compiler then marks the label with a select, not behind a branch)
        int idx = asked ? dense_redeem(total, label, ticket, d, unit) : -1;
        dead = d;
        asked = false;
        if (idx < 0) idx = steal(c);
        return idx;
    }
    // the draw at a workgroup's start: its own share first, then the others'
    template <class C>
    DSMI_TILES_HD int first(C& c) {
        if (!((dead >> label) & 1u)) {
            const int idx = dense_redeem(total, label, c.add(label), dead, unit);
            if (idx >= 0) return idx;
        }
        return steal(c);
    }
};

// A workgroup that has drawn -1 leaves; the last of the launch to do so -- everybody else has drawn for the last time -- zeroes the
// counters for the next launch on the stream.
template <class C>
DSMI_TILES_HD inline void tiles_leave(C& c) {
    if (c.done() == c.workgroups() - 1) {
#pragma unroll
        for (int l = 0; l <= kDenseLabels; ++l) c.zero(l);
    }
}

#if defined(__HIP__)
// The counters of a launch on the device: kDenseCntWords words, zero between launches.  Relaxed and agent-wide: a ticket is the value
// one fetch-and-add returned, nothing is published through the counters.
struct TileCounters {
    unsigned* cnt;
    __device__ unsigned add(int l) const { return __hip_atomic_fetch_add(cnt + l * kDenseCntStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ unsigned peek(int l) const { return __hip_atomic_load(cnt + l * kDenseCntStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ unsigned done() const { return add(kDenseLabels); }
    __device__ unsigned workgroups() const { return gridDim.x; }
    __device__ void zero(int l) const { __hip_atomic_store(cnt + l * kDenseCntStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
#endif

// ---- the host's side
// A by-demand launch: two workgroups per CU (the occupancy of all three kernels), each of which takes tile after tile, and behind a
// kernel's own LDS the words through which lane 0's draw reaches the workgroup.
constexpr int kTileTicketLds = 16;
inline int tiles_workgroups(int total, int n_cus) { return total < 2 * n_cus ? total : 2 * n_cus; }

// Who takes tiles by demand, from the texts of DSMI_DENSE_TILES and DSMI_CONV_TILES (null: not set) and whether the dense token is on.
// A text that is empty counts as not set; "0" is the static order, every XCD an equal share; any other text is by demand.
//   the GEMM (gemm_f16x3_wide_kernel): DSMI_DENSE_TILES; not set: by demand where the dense token is off, the static order where it
//     is on -- the gain is measured only with the token off (profiles/dense_tiles.txt); with it on a GEMM already has the chip's free
//     CUs to itself and the effect of 512 resident workgroups on the ring windows beside it is not measured.
//   the convs (conv_split.hip, conv1_split.hip): DSMI_CONV_TILES decides for them alone; without it a DSMI_DENSE_TILES that is set
//     decides for them as for the GEMM; neither set: the static order, whether the dense token is on or off -- by demand the convs
//     are held bit-identical and within the float64 bound, but they did not meet the bar for a default (profiles/conv_tiles.txt).
struct TileSwitches { bool gemm, convs; };
inline TileSwitches tile_switches(const char* dense_text, const char* conv_text, bool dense_token_on) {
    auto is_set = [](const char* e) { return e && *e; };
    auto by_demand = [](const char* e) { return !(e[0] == '0' && e[1] == 0); };
    TileSwitches s;
    s.gemm = is_set(dense_text) ? by_demand(dense_text) : !dense_token_on;
    s.convs = is_set(conv_text) ? by_demand(conv_text) : (is_set(dense_text) && by_demand(dense_text));
    return s;
}

}  // namespace dsmi
