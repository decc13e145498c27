// Replays the dense kernels' tile hand-out (danspeech_amd/csrc/dense_tiles.h) on the CPU: the counters are plain words, a
// "workgroup" runs the kernels' own TileTaker and tiles_leave over them, and a schedule says which workgroup takes its next step.
// tests/test_dense_tiles_host.py builds this file with -fsanitize=address,undefined and runs it.
//
//   dense_tiles_replay check            every grid x every draw order, launch after launch over the same counters: each tile exactly
//                                       once, nothing past the end, every workgroup counts itself out once, the last one leaves
//                                       all nine words zero; prints "ok ..."
//   dense_tiles_replay switch D C T ... tile_switches for the texts of DSMI_DENSE_TILES and DSMI_CONV_TILES ("-": not set) and the
//                                       dense token (0 | 1), triple after triple: one "gemm convs" per line
//   dense_tiles_replay map M N PN       the tiles of every label's own share, one "label ticket mt nu" per line (no stealing)
// and the conv kernels' side of it (danspeech_amd/csrc/conv_rows.h; tests/test_conv_tiles_host.py):
//   dense_tiles_replay conv-rows        the real kernel rows of every output row and workgroup, fi = 1 .. 200, both geometries; "ok ..."
//   dense_tiles_replay conv-check [R]   conv grids of 1-9 t-tiles x 1-14 f-tiles x 1-12 clip tiles, the same draw orders; "ok ..."
//   dense_tiles_replay conv-map T F Z   the tiles of every label's own share, one "label ticket tt ft z" per line (no stealing)
#include "../danspeech_amd/csrc/conv_rows.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dsmi;

static int g_fail = 0;
#define REQUIRE(cond, ...)                                            \
    do {                                                              \
        if (!(cond)) {                                                \
            std::fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                        \
            std::fprintf(stderr, "\n");                               \
            if (++g_fail > 20) std::exit(1);                          \
        }                                                             \
    } while (0)

struct Rng {      // xorshift64*: the same sequence everywhere
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

// One launch of a by-demand kernel over `cnt`, the counter words as they lie on the device.  A workgroup is a TileTaker (dense_tiles.h:
// the very steps the kernels run) and a state: first -> (ask -> next)* -> leave.  A schedule says which workgroup takes its next
// whole step; and with `nest` set, the counters may let other workgroups take whole steps in front of any single add, peek or done
// of the stepping one (one level deep, seeded) -- which puts other draws between a steal's peeks and its add, inside a first draw,
// and between the counts of two leaving workgroups.
struct Launch;
struct SimCounters {      // the counters policy of TileTaker / tiles_leave
    Launch& s;
    int w;                // the workgroup that is stepping
    unsigned add(int l);
    unsigned peek(int l);
    unsigned done();
    void zero(int l);
    unsigned workgroups() const;
};

struct Launch {
    enum State { kFirst, kHasTile, kAsked, kLeaving, kGone };
    int total, nwg, unit;               // unit: tiles that stay on one label (conv_rows.h: the f-tiles of a group)
    std::vector<unsigned>& cnt;         // kDenseCntWords words, zero before and behind the launch
    std::vector<unsigned> dead;         // per workgroup: TileTaker::dead
    std::vector<TileTaker> taker;       // per workgroup
    std::vector<int> state, done_calls;
    std::vector<int> hits;              // per linear tile index
    std::vector<int> live;              // workgroups that are not gone yet, in no particular order
    long draws = 0, stolen = 0;
    Rng* nest = nullptr;                // finer interleaving: see above
    bool nested = false;

    Launch(std::vector<unsigned>& cnt_, int total_, int nwg_, int unit_ = 1)
        : total(total_), nwg(nwg_), unit(unit_), cnt(cnt_), dead(nwg_, 0u), state(nwg_, kFirst), done_calls(nwg_, 0), hits(total_, 0), live(nwg_) {
        taker.reserve(nwg);
        for (int w = 0; w < nwg; ++w) { taker.emplace_back(total, w & (kDenseLabels - 1), unit, dead[w]); live[w] = w; }
        for (int l = 0; l <= kDenseLabels; ++l) REQUIRE(word(l) == 0u, "total %d: word %d is %u before the launch", total, l, word(l));
    }
    bool gone(int w) const { return state[w] == kGone; }
    void got(int w, int idx) {
        ++draws;
        if (idx < 0) { state[w] = kLeaving; return; }
        state[w] = kHasTile;
        REQUIRE(idx < total, "index %d of %d handed out", idx, total);
        if (idx >= total) return;
        hits[idx] += 1;
        const int label = w & (kDenseLabels - 1);
        if (idx < dense_base(total, label, unit) || idx >= dense_base(total, label, unit) + dense_count(total, label, unit)) ++stolen;
    }
    // one whole step of workgroup w
    void step(int w) {
        SimCounters c{*this, w};
        switch (state[w]) {
            case kFirst: got(w, taker[w].first(c)); break;
            case kHasTile: taker[w].ask(c); state[w] = kAsked; break;
            case kAsked: got(w, taker[w].next(c)); break;
            case kLeaving:
                tiles_leave(c);
                state[w] = kGone;
                live.erase(std::find(live.begin(), live.end(), w));
                break;
            default: REQUIRE(false, "workgroup %d steps after it has left", w);
        }
    }
    // in front of one access of workgroup w: maybe a few whole steps of others
    void others(int w) {
        if (!nest || nested || nest->below(4) != 0) return;
        nested = true;
        for (int n = 1 + nest->below(3); n > 0 && live.size() > 1; --n) {
            const int v = live[nest->below((int)live.size())];
            if (v != w) step(v);
        }
        nested = false;
    }
    unsigned& word(int l) {
        REQUIRE(l >= 0 && l <= kDenseLabels, "word %d", l);
        return cnt[(size_t)(l < 0 || l > kDenseLabels ? 0 : l) * kDenseCntStride];
    }
    void finish(const char* what) {
        REQUIRE(live.empty(), "%s: total %d, %zu workgroups have not left", what, total, live.size());
        for (int i = 0; i < total; ++i) REQUIRE(hits[i] == 1, "%s: total %d, tile %d handed out %d times", what, total, i, hits[i]);
        for (int w = 0; w < nwg; ++w) REQUIRE(done_calls[w] == 1, "%s: total %d, workgroup %d counted itself out %d times", what, total, w, done_calls[w]);
        for (int l = 0; l <= kDenseLabels; ++l) REQUIRE(word(l) == 0u, "%s: total %d, word %d is %u behind the launch", what, total, l, word(l));
    }
};

unsigned SimCounters::add(int l) {
    REQUIRE(l >= 0 && l < kDenseLabels, "label %d", l);
    s.others(w);
    const unsigned t = s.word(l)++;
    REQUIRE(t < (unsigned)(dense_count(s.total, l, s.unit) + s.nwg), "total %d: counter %d ran to %u", s.total, l, t + 1);
    return t;
}
unsigned SimCounters::peek(int l) {
    REQUIRE(l >= 0 && l < kDenseLabels, "label %d", l);
    s.others(w);
    return s.word(l);
}
unsigned SimCounters::done() {
    s.others(w);
    s.done_calls[w] += 1;
    return s.word(kDenseLabels)++;
}
void SimCounters::zero(int l) {
    REQUIRE(s.live.size() == 1 && s.live[0] == w, "total %d: workgroup %d resets the counters with %zu workgroups still there", s.total, w, s.live.size());
    s.word(l) = 0u;
}
unsigned SimCounters::workgroups() const { return (unsigned)s.nwg; }

// Every draw order is one launch over the SAME counter words: each must find them zero and leave them zero, so the launches of a
// grid relaunch each other, with a different schedule or seed each time.
static long replay_orders(int total, int n_cus, int n_random, int unit = 1) {
    const int nwg = tiles_workgroups(total, n_cus);
    std::vector<unsigned> cnt(kDenseCntWords, 0u);
    long draws = 0;
    {   // labels take strict turns; inside a label its workgroups take turns
        Launch s(cnt, total, nwg, unit);
        std::vector<int> next_of(kDenseLabels, 0);
        for (bool any = true; any;) {
            any = false;
            for (int l = 0; l < kDenseLabels; ++l) {
                const int n_l = (nwg - l + kDenseLabels - 1) / kDenseLabels;      // workgroups with this label
                for (int tries = 0; tries < n_l; ++tries) {
                    const int w = l + kDenseLabels * (next_of[l]++ % n_l);
                    if (s.gone(w)) continue;
                    s.step(w);
                    any = true;
                    break;
                }
            }
        }
        s.finish("turns");
        draws += s.draws;
    }
    for (int l = 0; l < kDenseLabels && l < nwg; ++l) {      // one label draws everything: every other share is stolen; then the others come and go
        Launch s(cnt, total, nwg, unit);
        for (bool any = true; any;) {
            any = false;
            for (int w = l; w < nwg; w += kDenseLabels)
                if (s.state[w] != Launch::kLeaving && !s.gone(w)) { s.step(w); any = true; }
        }
        REQUIRE(s.stolen == total - dense_count(total, l, unit), "one label: %ld stolen of %d", s.stolen, total);
        for (int w = 0; w < nwg; ++w)
            while (!s.gone(w)) s.step(w);
        s.finish("one label");
        REQUIRE(s.stolen == total - dense_count(total, l, unit), "one label: %ld stolen of %d behind the others", s.stolen, total);
        draws += s.draws;
    }
    for (int it = 0; it < n_random; ++it) {      // seeded random interleavings, some of them with a few workgroups far slower than the rest
        Launch s(cnt, total, nwg, unit);
        Rng rng(1000003ull * (uint64_t)total + (uint64_t)it), nest_rng(7919ull * (uint64_t)total + 31ull * (uint64_t)it + 1);
        if (it % 2 == 1) s.nest = &nest_rng;      // every other one also interleaves inside the steps
        const int slow = it % 3 == 0 ? rng.below(nwg) + 1 : 0;      // the first `slow` workgroups step 16 times less often
        while (!s.live.empty()) {
            const int w = s.live[rng.below((int)s.live.size())];
            if (w < slow && rng.below(16) != 0) continue;
            s.step(w);
        }
        s.finish("random");
        draws += s.draws;
    }
    for (size_t i = 0; i < cnt.size(); ++i) REQUIRE(cnt[i] == 0u, "total %d: word %zu is %u behind the last launch", total, i, cnt[i]);      // also between the nine
    return draws;
}

// every linear index maps to a tile of the grid, no two to the same one; a label's tickets are its share of the linear order
static void check_map(const DenseGrid& g) {
    const int total = dense_total(g);
    std::vector<char> seen((size_t)total, 0);
    int sum = 0;
    for (int l = 0; l < kDenseLabels; ++l) {
        const int n = dense_count(total, l);
        REQUIRE(n >= 0 && n <= dense_share(total), "share of label %d: %d", l, n);
        REQUIRE(n == 0 || dense_base(total, l) == sum, "label %d starts at %d, not %d", l, dense_base(total, l), sum);
        for (int t = 0; t < n; ++t) {
            const DenseTile tl = tile_of(g, l, t);
            REQUIRE(tl.mt >= 0 && tl.mt < g.mtiles && tl.nu >= 0 && tl.nu < g.nunits, "%d x %d pn %d: label %d ticket %d -> (%d, %d)", g.mtiles, g.nunits, g.pn, l, t, tl.mt, tl.nu);
            if (tl.mt < 0 || tl.mt >= g.mtiles || tl.nu < 0 || tl.nu >= g.nunits) continue;
            char& c = seen[(size_t)tl.mt * g.nunits + tl.nu];
            REQUIRE(!c, "%d x %d pn %d: tile (%d, %d) twice", g.mtiles, g.nunits, g.pn, tl.mt, tl.nu);
            c = 1;
        }
        sum += n;
    }
    REQUIRE(sum == total, "%d x %d: the shares add up to %d", g.mtiles, g.nunits, sum);
}

// ---- the conv kernels (conv_rows.h)
// kf lies in a row's range exactly when the input row it reads is a real one; a workgroup's range is the union of its live rows'
// ranges; a row's first real kernel row is even where the kernel's two-slot weight ring assumes it (sf and pf even: conv_split.hip)
static long check_conv_rows(int KF, int PF, int SF, int nf_wg, bool lo_even) {
    long n = 0;
    for (int fi = 1; fi <= 200; ++fi) {
        const int fo = (fi + 2 * PF - KF) / SF + 1;
        REQUIRE(fo >= 1, "fi %d: fo %d", fi, fo);
        for (int f = 0; f < fo; ++f) {
            const ConvRows r = conv_rows_of(f, fi, KF, PF, SF);
            for (int kf = 0; kf < KF; ++kf, ++n) {
                const int row = SF * f - PF + kf;
                REQUIRE((kf >= r.lo && kf <= r.hi) == (row >= 0 && row < fi), "KF %d fi %d f %d kf %d: range %d..%d, input row %d", KF, fi, f, kf, r.lo, r.hi, row);
            }
            REQUIRE(!conv_rows_empty(r), "KF %d fi %d f %d: no real row", KF, fi, f);
            if (lo_even) REQUIRE(r.lo % 2 == 0, "KF %d fi %d f %d: first real kernel row %d is odd", KF, fi, f, r.lo);
        }
        for (int f0 = 0; f0 < fo; f0 += nf_wg) {
            const ConvRows u = conv_rows_wg(f0, nf_wg, fo, fi, KF, PF, SF);
            if (lo_even) REQUIRE(u.lo % 2 == 0, "KF %d fi %d f0 %d: the workgroup's first kernel row %d is odd", KF, fi, f0, u.lo);
            for (int kf = 0; kf < KF; ++kf, ++n) {
                bool any = false;
                for (int w = 0; w < nf_wg && f0 + w < fo; ++w) {
                    const ConvRows r = conv_rows_of(f0 + w, fi, KF, PF, SF);
                    any = any || (kf >= r.lo && kf <= r.hi);
                }
                REQUIRE((kf >= u.lo && kf <= u.hi) == any, "KF %d fi %d f0 %d kf %d: workgroup range %d..%d", KF, fi, f0, kf, u.lo, u.hi);
            }
        }
        // rows past fo and an empty workgroup: nothing
        REQUIRE(conv_rows_empty(conv_rows_wg(fo, nf_wg, fo, fi, KF, PF, SF)), "KF %d fi %d: a workgroup past fo has rows", KF, fi);
    }
    return n;
}

// every linear index maps to a tile of the grid, no two to the same one; the shares are whole groups, add up, and inside a share the
// f-tiles of one (z, t-tile) are consecutive tickets; with eight t-tiles a label's tickets are the workgroups the hardware gives its XCD
// from the (t-tiles, f-tiles, z) grid of the static order (linear id x + 8 (y + nf z): XCD = x, in the order z, y)
static void check_conv_map(const ConvGrid& g) {
    const int total = conv_total(g);
    std::vector<char> seen((size_t)total, 0);
    int sum = 0;
    for (int l = 0; l < kDenseLabels; ++l) {
        const int n = dense_count(total, l, g.nf);
        REQUIRE(n >= 0 && n % g.nf == 0 && n <= dense_share(total, g.nf), "share of label %d: %d", l, n);
        REQUIRE(n == 0 || dense_base(total, l, g.nf) == sum, "label %d starts at %d, not %d", l, dense_base(total, l, g.nf), sum);
        for (int t = 0; t < n; ++t) {
            const ConvTile tl = conv_tile_of(g, l, t);
            const bool inside = tl.tt >= 0 && tl.tt < g.nt && tl.ft >= 0 && tl.ft < g.nf && tl.z >= 0 && tl.z < g.nz;
            REQUIRE(inside, "%d x %d x %d: label %d ticket %d -> (%d, %d, %d)", g.nt, g.nf, g.nz, l, t, tl.tt, tl.ft, tl.z);
            if (!inside) continue;
            char& c = seen[((size_t)tl.z * g.nt + tl.tt) * g.nf + tl.ft];
            REQUIRE(!c, "%d x %d x %d: tile (%d, %d, %d) twice", g.nt, g.nf, g.nz, tl.tt, tl.ft, tl.z);
            c = 1;
            const ConvTile first = conv_tile_of(g, l, t - t % g.nf);
            REQUIRE(tl.ft == t % g.nf && tl.tt == first.tt && tl.z == first.z, "%d x %d x %d: label %d ticket %d is no f-neighbour of ticket %d", g.nt, g.nf, g.nz, l, t, t - t % g.nf);
            if (g.nt == kDenseLabels) REQUIRE(tl.tt == l && tl.z == t / g.nf, "%d x %d x %d: label %d ticket %d -> (%d, %d, %d), the grid's XCD order gives (%d, %d, %d)", g.nt, g.nf, g.nz, l, t, tl.tt, tl.ft, tl.z, l, t % g.nf, t / g.nf);
        }
        sum += n;
    }
    REQUIRE(sum == total, "%d x %d x %d: the shares add up to %d", g.nt, g.nf, g.nz, sum);
}

int main(int argc, char** argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "conv-rows")) {
        long n = check_conv_rows(41, 20, 2, 8, false);      // conv1_split.hip: 8 rows per workgroup, no parity assumed
        n += check_conv_rows(21, 10, 2, 4, true);           // conv_split.hip: 4 rows per workgroup
        if (g_fail) return 1;
        std::printf("ok %ld kernel rows\n", n);
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "conv-map")) {
        const ConvGrid g{std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])};
        if (g.nt < 1 || g.nf < 1 || g.nz < 1) return 2;
        const int total = conv_total(g);
        for (int l = 0; l < kDenseLabels; ++l)
            for (int t = 0; t < dense_count(total, l, g.nf); ++t) {
                const ConvTile tl = conv_tile_of(g, l, t);
                std::printf("%d %d %d %d %d\n", l, t, tl.tt, tl.ft, tl.z);
            }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "conv-check")) {
        const int n_random = argc >= 3 ? std::atoi(argv[2]) : 20;
        long draws = 0;
        int maps = 0;
        for (int nt = 1; nt <= 9; ++nt)
            for (int nf = 1; nf <= 14; ++nf)
                for (int nz = 1; nz <= 12; ++nz) {
                    const ConvGrid g{nt, nf, nz};
                    check_conv_map(g);
                    ++maps;
                    // 256 CUs (most of these grids: one workgroup per tile), and a small device on which the workgroups loop
                    draws += replay_orders(conv_total(g), 256, n_random, nf);
                    draws += replay_orders(conv_total(g), 4, n_random, nf);
                }
        if (g_fail) return 1;
        std::printf("ok %d maps %ld draws\n", maps, draws);
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "map")) {
        const DenseGrid g{std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])};
        if (g.mtiles < 1 || g.nunits < 1 || g.pn < 1) return 2;
        const int total = dense_total(g);
        for (int l = 0; l < kDenseLabels; ++l)
            for (int t = 0; t < dense_count(total, l); ++t) {
                const DenseTile tl = tile_of(g, l, t);
                std::printf("%d %d %d %d\n", l, t, tl.mt, tl.nu);
            }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "check")) {
        const int n_random = argc >= 3 ? std::atoi(argv[2]) : 1000;
        // m-tiles x n-units (pairs of n-tiles in the 128 x 256 form); the last two: a single unit
        static const int grids[][2] = {{1, 1}, {1, 7}, {3, 3}, {2, 19}, {251, 19}, {256, 19}, {5, 1}, {251, 1}};
        long draws = 0;
        int maps = 0;
        for (const auto& mn : grids) {
            // every panel width: the launcher's three, and whatever DSMI_DEBUG_GEMM_PN makes of it (wider than the grid acts as the grid's width)
            for (int pn = 1; pn <= std::max(mn[1], 3) + 1; ++pn) { check_map(DenseGrid{mn[0], mn[1], pn}); ++maps; }
            // (the draw order does not depend on the panel width: it hands out linear indices); 256 CUs, and a small device on which
            // the workgroups loop at every size
            draws += replay_orders(mn[0] * mn[1], 256, n_random);
            draws += replay_orders(mn[0] * mn[1], 4, n_random / 10);
        }
        if (g_fail) return 1;
        std::printf("ok %d maps %ld draws\n", maps, draws);
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "switch")) {      // triples DENSE CONV TOKEN; a text of "-" stands for a variable that is not set
        if ((argc - 2) % 3 != 0) return 2;
        for (int i = 2; i + 2 < argc; i += 3) {
            const char* d = std::strcmp(argv[i], "-") ? argv[i] : nullptr;
            const char* c = std::strcmp(argv[i + 1], "-") ? argv[i + 1] : nullptr;
            const TileSwitches s = tile_switches(d, c, std::atoi(argv[i + 2]) != 0);
            std::printf("%d %d\n", s.gemm ? 1 : 0, s.convs ? 1 : 0);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: %s check [random-orders] | map M N PN | conv-rows | conv-check [random-orders] | conv-map T F Z | switch DENSE CONV TOKEN ...\n", argv[0]);
    return 2;
}
