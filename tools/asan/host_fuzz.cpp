// CPU harness for the host-only code of libdsmi.so, built with -fsanitize=address,undefined (`make -C danspeech_amd/csrc asan`).
// The .klm and ARPA readers parse untrusted files; the GPU pool has no device sanitizer, so this is where they are held to
// "a damaged file is refused or read, never a stray access".  tests/test_asan_host.py feeds it a few hundred mutated files.
//   host_fuzz lm FILE...      load each file (ARPA text or KenLM binary); when it loads, look n-grams up and score sequences
//   host_fuzz plan SEED N     random shard plans and phrase gates checked against their definitions
//   host_fuzz rnnplan FILE    the recurrent-layer plan (rnn_plan.h) of every input row of FILE, one line of text per row, each plan
//                             checked against the invariants below; rows: kind D H B inflight ring_windows lane KERNEL MODE DENSE n_cus
//   host_fuzz rnnplan grid    the invariants over the grid of 29 315 520 inputs that the plan was compared on with the code it replaced
//   host_fuzz rnnforms        which template instantiation of the persistent kernels runs which shape (rnn_plan.h: rnn_*_form): the grid
//                             of tests/rnn_form_table.json, one point per line
//   host_fuzz gate SEED N     the device gate's admission (gate_plan.h): a table of launches with the masks written out by hand, then N
//                             random sequences of planned launches of models of different widths, checked against the invariants below
//   host_fuzz scoreplan SEED N  the launch order of CTC transcript scoring (ctc_host.h: score_plan) on N random candidate lists with many
//                             ties: a permutation, every neighbouring pair in the documented order, nothing written past order[N)
//   host_fuzz ctccheck SEED N   the argument checks and the phrase packing of dsmi_align / dsmi_spot / dsmi_score / dsmi_alternatives (ctc_host.h) on N random
//                             calls held in exactly sized heap arrays, against the definitions written out below; what is refused
//                             on the numbers alone is called with null arrays
//   host_fuzz occcheck SEED N   the argument check of dsmi_occupancy (ctc_host.h: occ_check) and where each candidate's stored trellis lies, on N random
//                             calls held in exactly sized heap arrays, each good or with one fault, against the rules written out
//                             below; the stored trellis against its cap; what is refused on the numbers alone is called with null arrays
//   host_fuzz grammarcheck SEED N  the host half of dsmi_grammar (grammar_host.h: grammar_check, grammar_plan) on N random calls whose pool of
//                             graphs lies in exactly sized heap arrays, each good or with one fault, against the rules written out
//                             below; one node or arc over each limit; what is refused on the numbers alone is called with null arrays
//   host_fuzz grammarpostcheck SEED N  the host half of dsmi_grammar_posterior (grammar_post_host.h: grammar_post_check, grammar_post_plan,
//                             grammar_post_pack) on N random calls whose pool lies in exactly sized heap arrays, each good or with one
//                             fault: the successor transpose, the start lists and the label buckets against a plain restatement, the
//                             plan's numbers, the refusals and the cap on the stored trellises
//   host_fuzz grammarstreamcheck SEED N  the host half of streaming grammar decoding (grammar_stream_host.h: grammar_stream_plan,
//                             grammar_heavy_list, grammar_stream_check) on N random advance calls held in exactly sized heap arrays, each
//                             good or with one fault, against the rules written out below; the plan's numbers and refusals
//   host_fuzz alignlong SEED N  the host half of dsmi_align_long (align_long_host.h: align_long_check, align_long_plan) on N random calls whose
//                             transcript is an exactly sized heap array, each good or with one fault, against the rules written out
//                             below; the checkpoint rows on either side of their cap; what is refused on the numbers alone is called
//                             with a null array
//   host_fuzz editcheck SEED N  the host half of dsmi_edit_distance (edit_host.h: edit_check, edit_plan, edit_pack, edit_unpack) on N random
//                             calls held in exactly sized heap arrays, against the rules written out below; what is refused on the
//                             numbers alone is called with null arrays
//   host_fuzz lmscore SEED N    the host half of dsmi_lm_score (lm_score_host.h: lm_score_check, lm_score_plan, lm_score_pack, lm_score_unpack)
//                             on N random calls held in exactly sized heap arrays, against the rules written out below; what is
//                             refused on the numbers alone is called with null arrays
//   host_fuzz spotwatch SEED N  the host half of the streaming phrase watch (ctc_host.h: spot_watch_check, spot_stream_check; spot_pick.h: the
//                             online picking rule) on N random calls held in exactly sized heap arrays: the checks against the rules written
//                             out below, the rule over random tracks cut into random chunks against the rule written out plainly, nothing
//                             written past max_events
//   host_fuzz streampass FILE   the streaming pass plan (stream_host.h: stream_pass_plan, stream_pass_commit) of every line of FILE, each one
//                             session's schedule from a fresh handle: "context T_out_cap have_probs | T first last | T first last | ...";
//                             per pass the code, every StreamPass field and the flags after it; a refusal must have written nothing
#define __host__
#define __device__
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "lm.h"
#include "lm.cpp.inc"
#include "lm_klm.cpp.inc"
#include "host_logic.h"
#include "rnn_plan.h"
#include "gate_plan.h"
#include "ctc_host.h"
#include "align_long_host.h"
#include "grammar_host.h"
#include "grammar_post_host.h"
#include "grammar_stream_host.h"
#include "edit_host.h"
#include "lm_score_host.h"
#include "spot_pick.h"
#include "stream_host.h"

using namespace dsmi;

static int run_lm(int argc, char** argv) {
    std::vector<std::string> labels;
    const char* lab = "_abcdefghijklmnopqrstuvwxyz\xc3\xa6\xc3\xb8\xc3\xa5\xc3\xa9\xc3\xbc ";
    for (const char* p = lab; *p;) { const unsigned char c = (unsigned char)*p; const int n = c < 0x80 ? 1 : (c >> 5) == 6 ? 2 : 3; labels.emplace_back(p, n); p += n; }
    int loaded = 0, refused = 0;
    for (int i = 2; i < argc; ++i) {
        HostLM lm;
        const std::string msg = lm.load(argv[i], labels);
        if (!msg.empty()) { ++refused; continue; }
        ++loaded;
        if (lm.order < 1 || lm.order > kMaxOrder || lm.vocab.empty()) { std::fprintf(stderr, "%s: loaded with an implausible shape\n", argv[i]); return 3; }
        std::mt19937 rng(12345);
        const LmView v = lm.view();
        double sink = 0;
        for (int rep = 0; rep < 300; ++rep) {
            int32_t ids[kMaxOrder];
            const int n = 1 + (int)(rng() % (unsigned)lm.order);
            for (int k = 0; k < n; ++k) ids[k] = (int32_t)(rng() % lm.vocab.size());
            float lp = 0, bo = 0;
            sink += lm_lookup(v, ids, n, &lp, &bo) ? lp + bo : 0.0;
            sink += lm_cond_log10(v, ids, n - 1, ids[n - 1], lm.unk);
        }
        std::vector<int32_t> words;
        for (int k = 0; k < 7; ++k) words.push_back((int32_t)(rng() % lm.vocab.size()));
        sink += lm.sent_ln(words);
        // the dictionary trie the beam search walks
        for (size_t s = 0; s < lm.trie_word.size(); ++s) if (lm.trie_word[s] >= (int32_t)lm.vocab.size()) { std::fprintf(stderr, "dictionary word id out of range\n"); return 3; }
        for (int32_t nx : lm.trie_next) if (nx >= (int32_t)lm.trie_word.size()) { std::fprintf(stderr, "dictionary arc out of range\n"); return 3; }
        if (std::isnan(sink)) { std::fprintf(stderr, "%s: NaN score\n", argv[i]); return 3; }
    }
    std::printf("loaded %d refused %d\n", loaded, refused);
    return 0;
}

static int run_plan(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    for (int rep = 0; rep < reps; ++rep) {
        const int n = (int)(rng() % 70), world = 1 + (int)(rng() % 9);
        std::vector<int64_t> len((size_t)n);
        for (auto& l : len) l = (int64_t)(rng() % 5) * 1000 + (rng() % 3);
        std::vector<int32_t> rank_of((size_t)n, -1), slot_of((size_t)n, -1);
        plan_shards(len.data(), n, world, rank_of.data(), slot_of.data());
        // every rank's clips in slot order are non-increasing in length, ranks differ by at most one clip, every clip placed once
        std::vector<std::vector<int64_t>> per((size_t)world);
        for (int r = 0; r < world; ++r) per[(size_t)r].assign((size_t)((n - r + world - 1) / world > 0 ? (n - r + world - 1) / world : 0), -1);
        for (int i = 0; i < n; ++i) {
            if (rank_of[(size_t)i] < 0 || rank_of[(size_t)i] >= world) return 4;
            auto& row = per[(size_t)rank_of[(size_t)i]];
            if (slot_of[(size_t)i] < 0 || (size_t)slot_of[(size_t)i] >= row.size() || row[(size_t)slot_of[(size_t)i]] != -1) return 4;
            row[(size_t)slot_of[(size_t)i]] = len[(size_t)i];
        }
        for (auto& row : per) for (size_t k = 1; k < row.size(); ++k) if (row[k] > row[k - 1]) return 4;
        // the phrase gate: random energies, every phrase inside the signal, in order, never more stored than asked for
        const int64_t nhops = (int64_t)(rng() % 400);
        const int step = 128 << (rng() % 7);
        std::vector<double> e((size_t)nhops);
        for (auto& x : e) x = (rng() % 3) ? 0.0 : 1000.0;
        const int cap = (int)(rng() % 6);
        std::vector<int64_t> s0((size_t)cap + 1, -7), s1((size_t)cap + 1, -7);
        const int found = segment_phrases(e.data(), nhops, step, 600.0, (int)(rng() % 9), (int)(rng() % 4), s0.data(), s1.data(), cap);
        if (found < 0 || s0[(size_t)cap] != -7 || s1[(size_t)cap] != -7) return 5;
        for (int k = 0; k < std::min(found, cap); ++k)
            if (s0[(size_t)k] < 0 || s1[(size_t)k] <= s0[(size_t)k] || s1[(size_t)k] > nhops * step || (k && s0[(size_t)k] < s1[(size_t)k - 1] - 2 * (int64_t)step)) return 5;
        // the live gate: random energies in random runs, fewer event slots than events now and then; nothing past the slots is
        // written, every event lies inside the buffers seen so far (kept ones before the run included) and in stream order
        {
            const GateParams gp{1000.0, (int64_t)(rng() % 5), (int64_t)(rng() % 4), (int64_t)(rng() % 4)};
            GateState st;
            int64_t seen = 0, end_prev = 0;
            for (int run = 0; run < 4; ++run) {
                const int64_t nb = (int64_t)(rng() % 40);
                std::vector<uint64_t> S((size_t)nb);
                std::vector<int64_t> len((size_t)nb, 1024);
                for (auto& v : S) v = (rng() % 3) ? 0u : (uint64_t)2000 * 2000 * 1024;
                const int64_t gcap = (int64_t)(rng() % 8);
                std::vector<int64_t> f0((size_t)gcap + 1, -7), c0((size_t)gcap + 1, -7);
                std::vector<int32_t> l0((size_t)gcap + 1, -7);
                std::vector<uint32_t> en((size_t)nb + 1, 7u);
                GateEvents ev{f0.data(), c0.data(), l0.data(), gcap};
                const int64_t kept_before = st.kept;
                const int64_t closed = endpoint_gate(gp, st, S.data(), len.data(), nb, run == 3, ev, en.data());
                if (closed < 0 || ev.n < 0 || ev.n > nb + 1 || f0[(size_t)gcap] != -7 || c0[(size_t)gcap] != -7 || l0[(size_t)gcap] != -7 || en[(size_t)nb] != 7u) return 6;
                if (st.kept < 0 || st.kept > gp.keep_n || (st.phase != 0 && st.phase != 1)) return 6;
                for (int64_t k = 0; k < std::min(ev.n, gcap); ++k) {
                    const int64_t a = seen + f0[(size_t)k], b = a + c0[(size_t)k];
                    if (f0[(size_t)k] < -kept_before || c0[(size_t)k] < 0 || b > seen + nb || a < end_prev) return 6;
                    end_prev = b;
                }
                if (ev.n > gcap) end_prev = 0;      // events past the slots are counted, not stored: their ranges are unknown here
                seen += nb;
            }
        }
    }
    std::printf("plans and gates ok\n");
    return 0;
}


// ---- rnnplan: one row of input as the environment and the caller's hints would give it -----------------------------------------
// kernel: DSMI_RNN_KERNEL (- unset, duo, ring, ring4, ring8); mode: DSMI_RNN_MODE (- unset, steps, persist8); dense: DSMI_DENSE_MODE
// (split, f32).  The fence around the four-wave form's small shapes is lifted as in a process STARTED with DSMI_RNN_KERNEL=ring4.
static RnnPlanInput rnn_plan_input(int kind, int D, int H, int B, int inflight, int ring_windows, int lane, const std::string& kernel,
                                   const std::string& mode, const std::string& dense, int n_cus) {
    RnnPlanInput in;
    in.geom = make_rnn_geom(kind, H, D);
    in.geom16 = make_rnn_geom_u(kind, H, D, 16);
    in.have16 = H % 16 == 0;
    in.split16 = dense != "f32";
    in.B = B; in.n_cus = n_cus; in.inflight = inflight; in.ring_windows = ring_windows; in.lane = lane;
    in.rnn_mode = mode == "steps" ? 0 : 1;
    in.persist_gen = mode == "persist8" ? 1 : 2;
    in.rnn_kernel = kernel == "duo" ? 1 : (kernel == "ring" ? 2 : 0);
    in.ring8 = kernel == "ring8";
    in.ring4 = in.ring4_small_shapes = kernel == "ring4";
    return in;
}

// "x16|" or "x8|", then per launch "kernel at n nwin gate slot0 nslots cus ticket part;" (rnn_launch_text, rnn_plan.h)
static std::string rnn_plan_text(const RnnPlan& plan) {
    std::string out = plan.x16 ? "x16|" : "x8|";
    for (int i = 0; i < plan.launches.size(); ++i) {
        char buf[160];
        rnn_launch_text(plan.launches[i], buf, sizeof buf);
        out += buf;
    }
    return out;
}

// Does the launcher of launch `l` have a template instantiation for it (rnn_plan.h: rnn_*_form)?  The ring forms: for a window of
// l.n tiles, which is where the planned n meets the schedule the instantiation allows.
static bool rnn_launch_has_form(const RnnPlanInput& in, const RnnLaunch& l) {
    const int kind = in.geom16.kind, nkb = ceil_div(in.geom16.H, 32), ntiles = ceil_div(in.B, kTileClips);
    switch (l.kernel) {
        case RNN_PERSIST8: return rnn_persist_form(ceil_div(in.geom.nq, 2), ceil_div(in.B, 32), false, false).n != 0;
        case RNN_PERSIST16: return l.n >= 1 && rnn_persist16_form(kind, nkb, ceil_div(ntiles, l.n), false).n != 0;
        case RNN_PERSIST16_HALF: return l.n >= 1 && rnn_persist16_half_form(kind, nkb, ceil_div(ntiles, l.n), false) != 0;
        case RNN_DUO: return rnn_persist_duo_form(kind, nkb, false).n != 0;
        case RNN_RING8: return rnn_persist_ring_form(kind, nkb, l.n, false) != 0;
        case RNN_RING4: return rnn_persist_ring4_form(kind, nkb, l.n, false) != 0;
        default: return true;      // per step: every shape
    }
}

// Every real tile, tile pair or direction in exactly one launch; the gate slots within what the device holds; windows side by side
// within the device's CUs; tiles per window within the form's cap; the launches' shares sum to 1; every launch has an instantiation
// (rule 10).  0, or the number of the broken rule.
static int rnn_plan_check(const RnnPlanInput& in, const RnnPlan& plan) {
    if (plan.launches.size() < 1) return 1;
    const int ntiles = ceil_div(in.B, kTileClips), k0 = plan.launches[0].kernel;
    const int items = k0 == RNN_RING8 || k0 == RNN_RING4 ? ntiles : (k0 == RNN_DUO ? (ntiles + 1) / 2 : (k0 == RNN_PERSIST8 ? in.geom.D : 1));
    std::vector<int> seen((size_t)items, 0);
    double parts = 0;
    if (plan.x16 != rnn_kernel_is16(k0)) return 2;
    for (int i = 0; i < plan.launches.size(); ++i) {
        const RnnLaunch& l = plan.launches[i];
        const bool ring = l.kernel == RNN_RING8 || l.kernel == RNN_RING4;
        if (ring != (k0 == RNN_RING8 || k0 == RNN_RING4) || (!ring && l.kernel != k0)) return 3;      // one family per layer
        parts += l.part;
        if (!rnn_launch_has_form(in, l)) return 10;
        if (ring) {
            if (l.n < 1 || l.n > (l.kernel == RNN_RING8 ? kRingMaxTiles : kRing4MaxTiles) || l.nwin < 1) return 4;
            if (l.kernel == RNN_RING8 ? l.n > rnn_persist_ring_tiles(in.geom16, in.B, l.cus)
                                      : l.n > rnn_persist_ring4_tiles(in.geom16, in.B, l.cus, in.ring4_small_shapes, in.ring4_most)) return 4;
            for (int w = 0; w < l.nwin; ++w)
                for (int t = l.at + w * l.n; t < std::min(l.at + (w + 1) * l.n, ntiles); ++t) seen[(size_t)t] += 1;
            const int held = std::min(kRingSlots, l.cus > 0 ? in.n_cus / l.cus : 0);
            if (l.gate != GATE_RING || l.nslots != l.nwin || l.slot0 < 0 || l.slot0 + l.nslots > held) return 5;
            if (l.cus != rnn_persist_ring_cus(in.geom16) || l.nwin * l.cus > in.n_cus) return 6;
            if (l.ticket < 0 || l.ticket + 2 * l.nwin > 2 * ntiles + 2) return 7;      // the ticket words run_rnn_plan zeroes behind the counters (model.h: persist_cnt_words)
        } else if (l.kernel != RNN_STEPS) {
            if (l.gate != GATE_LANES || l.slot0 < 0 || l.slot0 + l.nslots > kMaxLanes || l.nslots < 1) return 5;
            if (l.kernel == RNN_DUO || l.kernel == RNN_PERSIST8) {
                if (l.n < 1) return 4;
                for (int i = l.at; i < l.at + l.n; ++i) { if (i < 0 || i >= items) return 8; seen[(size_t)i] += 1; }
                if (l.kernel == RNN_DUO && l.n * in.geom16.nwg * in.geom16.D > in.n_cus) return 6;
                if (l.kernel == RNN_PERSIST8 && l.n * in.geom.nwg > in.n_cus) return 6;
            } else {
                if (l.n < 1 || l.n * in.geom16.nwg * in.geom16.D > in.n_cus) return 6;
                if (ceil_div(ntiles, l.n) > (l.kernel == RNN_PERSIST16_HALF ? 2 : kPersist16MaxTiles)) return 4;
                seen[0] += 1;
            }
        } else {
            if (l.gate != GATE_NONE) return 5;
            seen[0] += 1;
        }
    }
    for (int c : seen) if (c != 1) return 8;
    if (std::fabs(parts - 1.0) > 1e-12) return 9;
    return 0;
}

static int run_rnnplan(int argc, char** argv) {
    if (argc < 3) return 2;
    static const char* const kernels[] = {"-", "duo", "ring", "ring4", "ring8"};
    static const char* const modes[] = {"-", "steps", "persist8"};
    static const char* const denses[] = {"split", "f32"};
    if (!std::strcmp(argv[2], "grid")) {
        long points = 0;
        static const int Bs[] = {1, 16, 17, 20, 32, 33, 48, 56, 64, 70, 96, 128, 256};
        std::vector<int> Hs;
        for (int H = 16; H <= 1344; H += 16) Hs.push_back(H);      // every width the 16-unit kernels may take, and three they do not
        for (int H : {100, 904, 1288}) Hs.push_back(H);
        for (int kind = 0; kind < 3; ++kind) for (int D = 1; D <= 2; ++D) for (int H : Hs) for (int B : Bs)
        for (int inflight : {1, 2, 4}) for (int rw : {0, 1, 2, 4}) for (int lane = 0; lane < 4; ++lane)
        for (const char* k : kernels) for (const char* mo : modes) for (const char* de : denses) for (int n_cus : {256, 128, 64}) {
            const RnnPlanInput in = rnn_plan_input(kind, D, H, B, inflight, rw, lane, k, mo, de, n_cus);
            const int bad = rnn_plan_check(in, plan_rnn_layer(in));
            if (bad) { std::fprintf(stderr, "rule %d broken at %d %d %d %d %d %d %d %s %s %s %d\n", bad, kind, D, H, B, inflight, rw, lane, k, mo, de, n_cus); return 6; }
            ++points;
        }
        std::printf("%ld plans ok\n", points);
        return 0;
    }
    std::FILE* f = std::fopen(argv[2], "r");
    if (!f) return 2;
    int kind, D, H, B, inflight, rw, lane, n_cus;
    char k[16], mo[16], de[16];
    int rc = 0;
    while (std::fscanf(f, "%d %d %d %d %d %d %d %15s %15s %15s %d", &kind, &D, &H, &B, &inflight, &rw, &lane, k, mo, de, &n_cus) == 11) {
        if (kind < 0 || kind > 2 || D < 1 || D > 2 || H < 1 || H > 4096 || B < 1 || B > 4096 || n_cus < 1) { rc = 2; break; }
        const RnnPlanInput in = rnn_plan_input(kind, D, H, B, inflight, rw, lane, k, mo, de, n_cus);
        const RnnPlan plan = plan_rnn_layer(in);
        const int bad = rnn_plan_check(in, plan);
        if (bad) { std::fprintf(stderr, "rule %d broken\n", bad); rc = 6; break; }
        std::printf("%s\n", rnn_plan_text(plan).c_str());
    }
    std::fclose(f);
    return rc;
}

// ---- rnnforms: the table of the persistent kernels' instantiations (rnn_plan.h: rnn_*_form), one grid point per line --------------
// "form kind H tiles stamps carried|answer"; the answer: the kernel's template arguments behind KIND with the defaults written out,
// "-" where no instantiation runs the shape (tests/rnn_form_table.json: the same grid from the launchers' if-ladders these replaced)
static int run_rnnforms() {
    static const char* const kinds[] = {"gru", "lstm", "rnn"};
    std::vector<int> Hs;
    for (int H = 16; H <= 1344; H += 16) Hs.push_back(H);
    for (int H : {100, 904, 1288}) Hs.push_back(H);
    for (int kind = 0; kind < 3; ++kind) for (int H : Hs) for (int tiles = 1; tiles <= 8; ++tiles) for (int st = 0; st < 2; ++st) {
        const int nkb = ceil_div(H, 32);
        // (the first argument is the form's n: 0 -> "-")
        auto row = [&](const char* form, int ca, const char* kernel, std::initializer_list<int> args) {
            std::string answer = *args.begin() ? kernel : "-";
            const char* sep = "";
            for (int v : args) if (*args.begin()) { answer += sep + std::to_string(v); sep = ","; }
            std::printf("%s %s %d %d %d %d|%s\n", form, kinds[kind], H, tiles, st, ca, answer.c_str());
        };
        for (int ca = 0; ca < 2; ++ca) {
            const RnnForm f = rnn_persist_form(ceil_div(make_rnn_geom(kind, H, 1).nq, 2), tiles, ca != 0, st != 0);
            row("persist8", ca, "", {f.n, f.alt, st, ca});
        }
        const RnnForm f16 = rnn_persist16_form(kind, nkb, tiles, st != 0);
        if (f16.alt) row("p16w8", 0, "pipe:", {f16.n, 0});
        else row("p16w8", 0, "", {f16.n, kPersist16Waves, st});
        row("p16w4", 0, "", {rnn_persist16_half_form(kind, nkb, tiles, st != 0), 4, st});
        const RnnForm fd = rnn_persist_duo_form(kind, nkb, st != 0);
        row("duo", 0, "", {fd.n, st, fd.alt});
        row("ring8", 0, "", {rnn_persist_ring_form(kind, nkb, tiles, st != 0), st, 0});
        row("ring4", 0, "", {rnn_persist_ring4_form(kind, nkb, tiles, st != 0), tiles > 4 ? 8 : 4, st, 0});
    }
    return 0;
}

// ---- gate: what a launch waits for and records at the per-device gate ----------------------------------------------------------
// The expected masks are written out by hand from the four functions gate_plan.h replaced (gate_wait, ring_gate_wait, gate_record,
// ring_gate_record): bit i = lane slot i / ring slot i.
struct GateCase {
    const char* name;
    int ring_cus[kRingSlots];
    int gate, slot0, nslots, cus, n_cus;
    bool turn;
    unsigned w_lanes, w_ring; bool w_full, w_acquire;
    unsigned r_lanes, r_ring; bool r_full, r_release;
    int after[kRingSlots];
};
static const GateCase kGateCases[] = {
    // lane launches: their own lanes, every ring slot and the whole-device event, with or without the turn word
    {"lane width 1, turn", {0, 0, 0, 0, 0}, GATE_LANES, 2, 1, 0, 256, true, 0x4, 0x1f, true, false, 0x4, 0, false, false, {0, 0, 0, 0, 0}},
    {"lane width 1, no turn", {0, 0, 0, 0, 0}, GATE_LANES, 2, 1, 0, 256, false, 0x4, 0x1f, true, false, 0x4, 0, false, false, {0, 0, 0, 0, 0}},
    {"lane width 2, turn", {50, 0, 0, 0, 0}, GATE_LANES, 2, 2, 0, 256, true, 0xc, 0x1f, true, false, 0xc, 0, false, false, {50, 0, 0, 0, 0}},
    {"lane width 2, no turn", {50, 0, 0, 0, 0}, GATE_LANES, 0, 2, 0, 256, false, 0x3, 0x1f, true, false, 0x3, 0, false, false, {50, 0, 0, 0, 0}},
    // the whole device: every event but the whole-device one and the lock -- or, without the word, the events alone
    {"lane width 4, turn", {0, 50, 0, 0, 0}, GATE_LANES, 0, 4, 0, 256, true, 0xf, 0x1f, false, true, 0, 0, true, true, {0, 50, 0, 0, 0}},
    {"lane width 4, no turn", {0, 50, 0, 0, 0}, GATE_LANES, 0, 4, 0, 256, false, 0xf, 0x1f, true, false, 0xf, 0, false, false, {0, 50, 0, 0, 0}},
    // ring windows
    {"ring on empty slots", {0, 0, 0, 0, 0}, GATE_RING, 1, 1, 50, 256, true, 0xf, 0x02, true, false, 0, 0x02, false, false, {0, 50, 0, 0, 0}},
    {"four of 56 CUs and one of 50 on 256", {56, 56, 56, 56, 0}, GATE_RING, 4, 1, 50, 256, true, 0xf, 0x11, true, false, 0, 0x10, false, false, {56, 56, 56, 56, 50}},
    {"the same on 304 CUs", {56, 56, 56, 56, 0}, GATE_RING, 4, 1, 50, 304, true, 0xf, 0x10, true, false, 0, 0x10, false, false, {56, 56, 56, 56, 50}},
    {"own slot busy", {50, 50, 0, 0, 0}, GATE_RING, 1, 1, 50, 256, false, 0xf, 0x02, true, false, 0, 0x02, false, false, {50, 50, 0, 0, 0}},
    {"own slot busy, the others too wide", {56, 56, 56, 56, 56}, GATE_RING, 2, 1, 50, 256, true, 0xf, 0x05, true, false, 0, 0x04, false, false, {56, 56, 50, 56, 56}},
    {"own slot first: the next one in index order", {0, 56, 56, 56, 56}, GATE_RING, 0, 1, 50, 256, true, 0xf, 0x03, true, false, 0, 0x01, false, false, {50, 56, 56, 56, 56}},
    {"two windows that fit", {50, 50, 50, 50, 50}, GATE_RING, 2, 2, 50, 256, true, 0xf, 0x0c, true, false, 0, 0x0c, false, false, {50, 50, 50, 50, 50}},
    {"two windows, one other to wait for", {70, 70, 56, 56, 0}, GATE_RING, 2, 2, 64, 256, true, 0xf, 0x0d, true, false, 0, 0x0c, false, false, {70, 70, 64, 64, 0}},
    {"exactly the device: no more waits", {100, 100, 0, 0, 56}, GATE_RING, 2, 1, 100, 256, true, 0xf, 0x05, true, false, 0, 0x04, false, false, {100, 100, 100, 0, 56}},
    {"one CU beyond: two others", {100, 100, 0, 0, 57}, GATE_RING, 2, 1, 100, 256, true, 0xf, 0x07, true, false, 0, 0x04, false, false, {100, 100, 100, 0, 57}},
};

static int gate_literal_cases() {
    for (const GateCase& c : kGateCases) {
        DeviceGateState st;
        for (int i = 0; i < kRingSlots; ++i) st.ring_cus[i] = c.ring_cus[i];
        RnnLaunch l;
        l.gate = c.gate; l.slot0 = c.slot0; l.nslots = c.nslots; l.cus = c.cus;
        const DeviceGateWait w = gate_plan_wait(st, l, c.n_cus, c.turn);
        const DeviceGateRecord r = gate_plan_record(st, l, c.turn);
        bool ok = w.lanes == c.w_lanes && w.ring == c.w_ring && w.full == c.w_full && w.acquire == c.w_acquire &&
                  r.lanes == c.r_lanes && r.ring == c.r_ring && r.full == c.r_full && r.release == c.r_release;
        for (int i = 0; i < kRingSlots; ++i) ok = ok && r.after.ring_cus[i] == c.after[i];
        if (!ok) {
            std::fprintf(stderr, "gate case '%s': wait %x %x %d %d, record %x %x %d %d\n", c.name, w.lanes, w.ring, w.full, w.acquire, r.lanes, r.ring, r.full, r.release);
            return 7;
        }
    }
    return 0;
}

// Random sequences: two or three models of different widths on one device, layers planned by plan_rnn_layer in random order.  The
// simulation takes every recorded ring window for running until a later launch has waited for its slot.  0, or the broken rule:
//   1  the CUs of the windows not waited for plus the new launch's exceed the device
//   2  a lane launch waits for every ring slot (and its own lanes); a ring launch for every lane, its own slots and the whole-device event
//   3  a whole-device launch waits for every lane and ring slot, and takes the turn exactly when the word exists (else the event)
//   4  what is recorded is exactly the launch's own slots (a whole-device launch under the lock: the lock given back, the whole-device event)
static long g_extra_waits = 0;      // ring launches that had to wait for a slot not their own
static int gate_sequence(std::mt19937& rng, int n_cus, bool turn) {
    static const int Hs[] = {256, 512, 640, 800, 832, 896, 1024};
    const int nmodels = 2 + (int)(rng() % 2);
    int kind[3], H[3], D[3];
    for (int k = 0; k < nmodels; ++k) { kind[k] = (int)(rng() % 3); H[k] = Hs[rng() % 7]; D[k] = 1 + (int)(rng() % 2); }
    DeviceGateState st;
    int running[kRingSlots] = {0, 0, 0, 0, 0};
    const unsigned all_lanes = (1u << kMaxLanes) - 1, all_ring = (1u << kRingSlots) - 1;
    for (int step = 0; step < 60; ++step) {
        const int k = (int)(rng() % (unsigned)nmodels);
        static const int Bs[] = {1, 16, 32, 33, 64, 96, 128};
        static const char* const kernels[] = {"-", "-", "-", "duo", "ring"};
        const RnnPlanInput in = rnn_plan_input(kind[k], D[k], H[k], Bs[rng() % 7], 1 + (int)(rng() % 4), (int)(rng() % 3), (int)(rng() % 8),
                                               kernels[rng() % 5], (rng() % 8) ? "-" : "persist8", "split", n_cus);
        const RnnPlan plan = plan_rnn_layer(in);
        for (int i = 0; i < plan.launches.size(); ++i) {
            const RnnLaunch& l = plan.launches[i];
            if (l.gate == GATE_NONE || l.join) continue;
            const unsigned own = ((1u << l.nslots) - 1) << l.slot0;
            const DeviceGateWait w = gate_plan_wait(st, l, n_cus, turn);
            const DeviceGateRecord r = gate_plan_record(st, l, turn);
            for (int s = 0; s < kRingSlots; ++s) if (w.ring >> s & 1) running[s] = 0;
            int busy = l.gate == GATE_RING ? l.nslots * l.cus : 0;
            for (int s = 0; s < kRingSlots; ++s) busy += running[s];
            if (busy > n_cus) return 1;
            if (l.gate == GATE_RING && (w.ring & ~own)) ++g_extra_waits;
            const bool whole = l.gate == GATE_LANES && l.nslots >= kMaxLanes;
            if (l.gate == GATE_RING) {
                if (w.lanes != all_lanes || !w.full || w.acquire || (w.ring & own) != own) return 2;
                if (r.ring != own || r.lanes || r.full || r.release) return 4;
            } else if (!whole) {
                if (w.ring != all_ring || w.lanes != own || !w.full || w.acquire) return 2;
                if (r.lanes != own || r.ring || r.full || r.release) return 4;
            } else {
                if (w.ring != all_ring || w.lanes != all_lanes || w.acquire != turn || w.full != !turn) return 3;
                if (r.ring || r.lanes != (turn ? 0u : all_lanes) || r.full != turn || r.release != turn) return 4;
            }
            for (int s = 0; s < kRingSlots; ++s) {
                const bool mine = l.gate == GATE_RING && (own >> s & 1);
                if (r.after.ring_cus[s] != (mine ? l.cus : st.ring_cus[s])) return 4;
                if (mine) running[s] = l.cus;
            }
            st = r.after;
        }
    }
    return 0;
}

static int run_gate(int argc, char** argv) {
    if (const int bad = gate_literal_cases()) return bad;
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    for (int rep = 0; rep < reps; ++rep)
        for (int n_cus : {256, 128, 64})
            if (const int bad = gate_sequence(rng, n_cus, rep % 2 == 0)) { std::fprintf(stderr, "gate rule %d broken on %d CUs (sequence %d)\n", bad, n_cus, rep); return 8; }
    std::printf("%d gate cases and %d sequences ok, %ld launches waited for other windows\n", (int)(sizeof kGateCases / sizeof kGateCases[0]), 3 * reps, g_extra_waits);
    return 0;
}

// ---- scoreplan: frames descending, then clip ascending, then tokens descending, then index ascending --------------------------
static int run_scoreplan(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    for (int rep = 0; rep < reps; ++rep) {
        const int N = 1 + (int)(rng() % 300), B = 1 + (int)(rng() % 9), span = 1 + (int)(rng() % 6);
        std::vector<int32_t> frames_of((size_t)B), clip((size_t)N), frames((size_t)N), lens((size_t)N), order((size_t)N + 1, -7);
        for (auto& f : frames_of) f = (int32_t)(rng() % (unsigned)span);       // few distinct values: clips tie on frames
        for (int n = 0; n < N; ++n) {
            clip[(size_t)n] = (int32_t)(rng() % (unsigned)B);
            frames[(size_t)n] = frames_of[(size_t)clip[(size_t)n]];
            lens[(size_t)n] = (int32_t)(rng() % (unsigned)span);
        }
        if (score_plan(clip.data(), frames.data(), lens.data(), N, order.data()) != N || order[(size_t)N] != -7) return 9;
        std::vector<int> seen((size_t)N, 0);
        for (int i = 0; i < N; ++i) {
            const int32_t x = order[(size_t)i];
            if (x < 0 || x >= N || seen[(size_t)x]++) return 9;
            if (i == 0) continue;
            const int32_t w = order[(size_t)i - 1];
            const long long kw[4] = {-(long long)frames[(size_t)w], clip[(size_t)w], -(long long)lens[(size_t)w], w};
            const long long kx[4] = {-(long long)frames[(size_t)x], clip[(size_t)x], -(long long)lens[(size_t)x], x};
            if (!std::lexicographical_compare(kw, kw + 4, kx, kx + 4)) return 9;
        }
    }
    std::printf("%d score plans ok\n", reps);
    return 0;
}

// ---- ctccheck: every array is a heap block of exactly the size the call declares, so a read past it is a sanitizer report ----
static std::vector<int32_t> exact(size_t n, int32_t v = 0) { std::vector<int32_t> a(n, v); a.shrink_to_fit(); return a; }
static const int32_t* ptr_or_null(const std::vector<int32_t>& a) { return a.empty() ? nullptr : a.data(); }

// The shortest frame labelling that emits the row: every token once, a blank between two equal tokens.
static int min_frames(const int32_t* row, int L, int blank) {
    std::vector<int32_t> path;
    for (int k = 0; k < L; ++k) {
        if (k && row[k] == row[k - 1]) path.push_back(blank);
        path.push_back(row[k]);
    }
    return (int)path.size();
}

// A row of L ids of an alphabet of C labels; with `spoil` one of them is the blank, C or negative.  Returns the first bad id's index or -1.
static int random_row(std::mt19937& rng, int32_t* row, int L, int C, int blank, bool spoil) {
    for (int k = 0; k < L; ++k) {
        do row[k] = (int32_t)(rng() % (unsigned)C); while (row[k] == blank);
        if (k && C > 2 && rng() % 3 == 0) row[k] = row[k - 1];      // runs of equal tokens
    }
    if (!spoil || L == 0) return -1;
    const int at = (int)(rng() % (unsigned)L);
    const int32_t bad[3] = {(int32_t)blank, (int32_t)C, -1 - (int32_t)(rng() % 5)};
    row[at] = bad[rng() % 3];
    return at;
}

#define CTC_FAIL(what) do { std::fprintf(stderr, "ctccheck: %s (repetition %d, line %d)\n", what, rep, __LINE__); return 10; } while (0)

static int run_ctccheck(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long rows_checked = 0, words_checked = 0;
    for (int rep = 0; rep < reps; ++rep) {
        const int C = 2 + (int)(rng() % 127), blank = (int)(rng() % (unsigned)C);
        const int B = 1 + (int)(rng() % 6), To = 1 + (int)(rng() % 40);
        std::string err;
        // ---- the clip sizes: inside 0 .. T_out, or one of them outside; no sizes = T_out frames each
        {
            std::vector<int32_t> sizes = exact((size_t)B), sz = exact((size_t)B, -7);
            for (auto& v : sizes) v = (int32_t)(rng() % (unsigned)(To + 1));
            const bool spoil = rng() % 3 == 0;
            if (spoil) sizes[rng() % (unsigned)B] = rng() % 2 ? To + 1 + (int32_t)(rng() % 3) : -1 - (int32_t)(rng() % 3);
            const int rc = ctc_check_sizes(kSpotRows, sizes.data(), B, To, sz.data(), err);
            if (rc != (spoil ? DSMI_ERR_INVALID : DSMI_OK)) CTC_FAIL("sizes: wrong code");
            if (spoil && err.find(": size outside 0 .. T_out") == std::string::npos) CTC_FAIL("sizes: wrong message");
            if (!spoil && sz != sizes) CTC_FAIL("sizes: not copied");
            if (ctc_check_sizes(kSpotRows, nullptr, B, To, sz.data(), err) != DSMI_OK || sz != exact((size_t)B, To)) CTC_FAIL("sizes: null is not T_out");
        }
        // ---- one token row of each tool: the length, the ids, the repeat count, the feasibility rule
        for (const CtcRows* kind : {&kAlignRows, &kSpotRows, &kScoreRows}) {
            const int L_stride = (int)(rng() % 20), L = (int)(rng() % 24) - 2;
            int repeats = -7;
            if (L < kind->min_len || L > L_stride) {      // refused on the length: the row is not read (there is none)
                if (ctc_check_row(*kind, rep, nullptr, L, L_stride, C, blank, &repeats, err) != DSMI_ERR_INVALID || repeats != -7) CTC_FAIL("row: a bad length passed");
                if (err.find(std::string(kind->length) + " outside " + std::to_string(kind->min_len) + " .. L_stride") == std::string::npos) CTC_FAIL("row: wrong message");
                continue;
            }
            std::vector<int32_t> row = exact((size_t)L);
            const int bad_at = random_row(rng, row.data(), L, C, blank, rng() % 3 == 0);
            int first_bad = -1;
            for (int k = L - 1; k >= 0; --k) if (row[(size_t)k] < 0 || row[(size_t)k] >= C || row[(size_t)k] == blank) first_bad = k;
            if ((bad_at < 0) != (first_bad < 0)) CTC_FAIL("row: the test's own spoiling");
            const int rc = ctc_check_row(*kind, rep, ptr_or_null(row), L, L_stride, C, blank, &repeats, err);
            if (rc != (first_bad < 0 ? DSMI_OK : DSMI_ERR_INVALID)) CTC_FAIL("row: wrong code");
            ++rows_checked;
            if (first_bad >= 0) {
                if (err.find(std::string(kind->id) + " " + std::to_string(row[(size_t)first_bad]) + " is the blank or not a label") == std::string::npos) CTC_FAIL("row: wrong id named");
                continue;
            }
            int equal_pairs = 0;
            for (int k = 1; k < L; ++k) equal_pairs += row[(size_t)k] == row[(size_t)k - 1];
            const int need = min_frames(ptr_or_null(row), L, blank);
            if (repeats != equal_pairs || L + repeats != need) CTC_FAIL("row: repeat count");
            for (int frames : {need - 1, need, need + 1, 0, To})
                if (frames >= 0 && ctc_feasible_len(L, repeats, frames) != (need <= frames ? L : -1)) CTC_FAIL("feasibility rule");
        }
        // ---- whole calls with nothing wrong: what the checks hand the launch
        {
            const int L_stride = (int)(rng() % 12), N = 1 + (int)(rng() % 9);
            std::vector<int32_t> sizes = exact((size_t)B), clip = exact((size_t)N), lens = exact((size_t)N), tg = exact((size_t)N * L_stride);
            for (auto& v : sizes) v = (int32_t)(rng() % (unsigned)(To + 1));
            for (int n = 0; n < N; ++n) {
                clip[(size_t)n] = (int32_t)(rng() % (unsigned)B);
                lens[(size_t)n] = (int32_t)(rng() % (unsigned)(L_stride + 1));
                random_row(rng, tg.data() + (size_t)n * L_stride, lens[(size_t)n], C, blank, false);
            }
            std::vector<int32_t> sz, tl, frames;
            int L_max = -7;
            if (score_check(sizes.data(), B, To, clip.data(), ptr_or_null(tg), lens.data(), N, L_stride, C, blank, sz, tl, frames, &L_max, err) != DSMI_OK) CTC_FAIL("score: a good call refused");
            int want_max = 0;
            for (int n = 0; n < N; ++n) {
                const int T = sizes[(size_t)clip[(size_t)n]], L = lens[(size_t)n];
                const int want = min_frames(tg.data() + (size_t)n * L_stride, L, blank) <= T ? L : -1;
                if (frames[(size_t)n] != T || tl[(size_t)n] != want) CTC_FAIL("score: frames or feasibility");
                want_max = std::max(want_max, want);
            }
            if (sz != sizes || L_max != want_max || (int)tl.size() != N) CTC_FAIL("score: sizes or the longest candidate");
            // the same call through the token-confidence check: the same verdicts, and trellises placed back to back
            {
                std::vector<int32_t> sz2, tl2, frames2, base;
                int L_max2 = -7;
                uint64_t trellis = 7;
                if (alt_check(sizes.data(), B, To, clip.data(), ptr_or_null(tg), lens.data(), N, L_stride, C, blank, sz2, tl2, frames2, base, &L_max2, &trellis, err) != DSMI_OK) CTC_FAIL("alternatives: a good call refused");
                if (sz2 != sz || tl2 != tl || frames2 != frames || L_max2 != L_max || (int)base.size() != N) CTC_FAIL("alternatives: not score's verdicts");
                uint64_t at = 0;
                for (int n = 0; n < N; ++n) {
                    if ((uint64_t)base[(size_t)n] != at) CTC_FAIL("alternatives: a trellis out of place");
                    if (tl[(size_t)n] >= 0) at += (uint64_t)frames[(size_t)n] * (2 * (uint64_t)tl[(size_t)n] + 1);
                }
                if (trellis != at) CTC_FAIL("alternatives: the trellis total");
            }
            // the same rows as one transcript per clip (the first B of them, N >= B or not)
            const int Ba = std::min(B, N);
            if (align_check(sizes.data(), Ba, To, ptr_or_null(tg), lens.data(), L_stride, C, blank, sz, tl, &L_max, err) != DSMI_OK) CTC_FAIL("align: a good call refused");
            want_max = 0;
            for (int b = 0; b < Ba; ++b) {
                const int L = lens[(size_t)b], want = min_frames(tg.data() + (size_t)b * L_stride, L, blank) <= sizes[(size_t)b] ? L : -1;
                if (tl[(size_t)b] != want) CTC_FAIL("align: feasibility");
                want_max = std::max(want_max, want);
            }
            if (L_max != want_max || (int)sz.size() != Ba) CTC_FAIL("align: the longest transcript");
            // one fault: a clip index outside the batch
            clip[rng() % (unsigned)N] = rng() % 2 ? B : -1;
            if (score_check(sizes.data(), B, To, clip.data(), ptr_or_null(tg), lens.data(), N, L_stride, C, blank, sz, tl, frames, &L_max, err) != DSMI_ERR_INVALID ||
                err.find("clip outside 0 .. B-1") == std::string::npos) CTC_FAIL("score: a clip outside the batch passed");
        }
        // ---- refused on the numbers alone: no array exists
        {
            std::vector<int32_t> sz, tl, frames;
            int L_max = 0;
            const int32_t* none = nullptr;
            const int big = 1 + (int)(rng() % 1000);
            if (align_check(none, 0, To, none, none, 3, C, blank, sz, tl, &L_max, err) != DSMI_ERR_INVALID) CTC_FAIL("align: B = 0");
            if (align_check(none, B, -big, none, none, 3, C, blank, sz, tl, &L_max, err) != DSMI_ERR_INVALID) CTC_FAIL("align: T_out < 0");
            if (align_check(none, B, To, none, none, -big, C, blank, sz, tl, &L_max, err) != DSMI_ERR_INVALID) CTC_FAIL("align: L_stride < 0");
            if (align_check(none, B, To, none, none, DSMI_ALIGN_MAX_TOKENS + big, C, blank, sz, tl, &L_max, err) != DSMI_ERR_CAPACITY) CTC_FAIL("align: L_stride over the limit");
            if (score_check(none, B, To, none, none, none, 0, 3, C, blank, sz, tl, frames, &L_max, err) != DSMI_ERR_INVALID) CTC_FAIL("score: N = 0");
            if (score_check(none, B, To, none, none, none, big, -1, C, blank, sz, tl, frames, &L_max, err) != DSMI_ERR_INVALID) CTC_FAIL("score: L_stride < 0");
            if (score_check(none, B, To, none, none, none, big, DSMI_SCORE_MAX_TOKENS + big, C, blank, sz, tl, frames, &L_max, err) != DSMI_ERR_CAPACITY) CTC_FAIL("score: L_stride over the limit");
            if (score_check(none, B, To, none, none, none, (1 << 24) / 2048 + big, 2048, C, blank, sz, tl, frames, &L_max, err) != DSMI_ERR_CAPACITY ||
                err.find("2^24") == std::string::npos) CTC_FAIL("score: N * L_stride over 2^24");
            {
                std::vector<int32_t> base;
                uint64_t trellis = 0;
                if (alt_check(none, B, To, none, none, none, 0, 3, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_INVALID) CTC_FAIL("alternatives: N = 0");
                if (alt_check(none, B, To, none, none, none, big, -1, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_INVALID) CTC_FAIL("alternatives: L_stride < 0");
                if (alt_check(none, B, To, none, none, none, big, DSMI_ALT_MAX_TOKENS + big, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_CAPACITY ||
                    err.find("DSMI_ALT_MAX_TOKENS") == std::string::npos) CTC_FAIL("alternatives: L_stride over the limit");
                if (alt_check(none, B, To, none, none, none, (1 << 24) / (1024 * C) + big, 1024, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_CAPACITY ||
                    err.find("2^24") == std::string::npos) CTC_FAIL("alternatives: N * L_stride * n_labels over 2^24");
            }
            const float floor_ = -1.f;
            if (spot_check(none, B, To, none, none, 0, 3, 4, floor_, C, blank, sz, err) != DSMI_ERR_INVALID) CTC_FAIL("spot: K = 0");
            if (spot_check(none, B, To, none, none, 2, 3, rng() % 2 ? 0 : DSMI_SPOT_MAX_HITS + big, floor_, C, blank, sz, err) != DSMI_ERR_INVALID) CTC_FAIL("spot: max_hits");
            if (spot_check(none, B, To, none, none, 2, 3, 4, std::nanf(""), C, blank, sz, err) != DSMI_ERR_INVALID) CTC_FAIL("spot: NaN floor");
            if (spot_check(none, B, To, none, none, 2, DSMI_SPOT_MAX_TOKENS + big, 4, floor_, C, blank, sz, err) != DSMI_ERR_CAPACITY) CTC_FAIL("spot: L_stride over the limit");
            if (spot_check(none, B, To, none, none, DSMI_SPOT_MAX_PHRASES + big, 3, 4, floor_, C, blank, sz, err) != DSMI_ERR_CAPACITY) CTC_FAIL("spot: K over the limit");
            if (spot_check(none, 1 << 14, 4 + big, none, none, 1 << 12, 3, 4, floor_, C, blank, sz, err) != DSMI_ERR_CAPACITY) CTC_FAIL("spot: the track cap");
            if (spot_check(none, 1, 1 << 26, none, none, 2 + big, 3, 4, floor_, C, blank, sz, err) != DSMI_ERR_CAPACITY) CTC_FAIL("spot: the track cap by T_out");
        }
        // ---- phrase search: the check, the plan and every packed word
        {
            const int K = 1 + (int)(rng() % 40), L_stride = 1 + (int)(rng() % (rng() % 4 ? 12 : DSMI_SPOT_MAX_TOKENS));
            std::vector<int32_t> sizes = exact((size_t)B, To), lens = exact((size_t)K), ph = exact((size_t)K * L_stride), sz;
            for (int k = 0; k < K; ++k) {
                lens[(size_t)k] = 1 + (int32_t)(rng() % (unsigned)L_stride);
                random_row(rng, ph.data() + (size_t)k * L_stride, lens[(size_t)k], C, blank, false);
            }
            if (spot_check(sizes.data(), B, To, ph.data(), lens.data(), K, L_stride, 1 + (int)(rng() % DSMI_SPOT_MAX_HITS), -INFINITY, C, blank, sz, err) != DSMI_OK) CTC_FAIL("spot: a good call refused");
            std::vector<int32_t> group_of = exact((size_t)K, -7), first = exact((size_t)K, -7);
            const int n_groups = spot_plan(lens.data(), K, group_of.data(), first.data());
            std::vector<int> used((size_t)n_groups, 0);
            for (int k = 0; k < K; ++k) {      // in order, back to back, a group never beyond kSpotThreads states, a new group only when needed
                const int g = group_of[(size_t)k], S = 2 * lens[(size_t)k] - 1;
                if (g < 0 || g >= n_groups || (k && g != group_of[(size_t)k - 1] && (g != group_of[(size_t)k - 1] + 1 || used[(size_t)g - 1] + S <= kSpotThreads))) CTC_FAIL("plan: groups out of order");
                if (first[(size_t)k] != used[(size_t)g]) CTC_FAIL("plan: a gap or an overlap");
                used[(size_t)g] += S;
                if (used[(size_t)g] > kSpotThreads) CTC_FAIL("plan: a group beyond 256 states");
            }
            if (group_of[(size_t)K - 1] != n_groups - 1) CTC_FAIL("plan: the number of groups");
            std::vector<int32_t> words = exact((size_t)n_groups * kSpotThreads), want = exact((size_t)n_groups * kSpotThreads);
            spot_pack(ph.data(), lens.data(), K, L_stride, blank, group_of.data(), first.data(), words.data());
            for (int k = 0; k < K; ++k) {
                std::vector<int32_t> ext;      // token, blank, token, ..., token
                for (int j = 0; j < lens[(size_t)k]; ++j) { if (j) ext.push_back(blank); ext.push_back(ph[(size_t)k * L_stride + j]); }
                for (size_t s = 0; s < ext.size(); ++s) {
                    const int32_t w = words[(size_t)group_of[(size_t)k] * kSpotThreads + first[(size_t)k] + s];
                    const bool skip = s % 2 == 0 && s >= 2 && ext[s] != ext[s - 2], last = s + 1 == ext.size();
                    if ((w & 255) != ext[s] || !(w & kSpotLive) || !!(w & kSpotSkip) != skip || !!(w & kSpotFirst) != (s == 0) || !!(w & kSpotLast) != last ||
                        (w >> kSpotPhraseShift) != (last ? k : 0) || (w & 0xf000)) CTC_FAIL("pack: a word's label, flags or phrase index");
                    want[(size_t)group_of[(size_t)k] * kSpotThreads + first[(size_t)k] + s] = w;
                    ++words_checked;
                }
            }
            if (words != want) CTC_FAIL("pack: a word where no state sits");
        }
    }
    std::printf("%d ctc calls ok, %ld rows and %ld packed words checked\n", reps, rows_checked, words_checked);
    return 0;
}

// ---- occcheck: dsmi_occupancy's check (ctc_host.h: occ_check) and the placing of its stored trellis, each array a heap block of
// exactly the size the call declares
#define OCC_FAIL(what) do { std::fprintf(stderr, "occcheck: %s (repetition %d, line %d)\n", what, rep, __LINE__); return 11; } while (0)

static int run_occcheck(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long good = 0, refused = 0, infeasible = 0;
    for (int rep = 0; rep < reps; ++rep) {
        const int C = 2 + (int)(rng() % 127), blank = (int)(rng() % (unsigned)C);
        const int B = 1 + (int)(rng() % 6), To = 1 + (int)(rng() % 40);
        const int L_stride = (int)(rng() % 12), N = 1 + (int)(rng() % 9);
        std::string err;
        std::vector<int32_t> sz, tl, frames, base;
        int L_max = -7;
        uint64_t trellis = 7;
        // ---- a whole call; with `fault` one thing is wrong with it, and the rule that refuses it is written out here
        std::vector<int32_t> sizes = exact((size_t)B), clip = exact((size_t)N), lens = exact((size_t)N), tg = exact((size_t)N * L_stride);
        for (auto& v : sizes) v = (int32_t)(rng() % (unsigned)(To + 1));
        for (int n = 0; n < N; ++n) {
            clip[(size_t)n] = (int32_t)(rng() % (unsigned)B);
            lens[(size_t)n] = (int32_t)(rng() % (unsigned)(L_stride + 1));
            random_row(rng, tg.data() + (size_t)n * L_stride, lens[(size_t)n], C, blank, false);
        }
        const bool no_sizes = rng() % 5 == 0;
        const int fault = rng() % 2 ? 0 : 1 + (int)(rng() % 4);
        const char* text = "";
        if (fault == 1) { sizes[rng() % (unsigned)B] = rng() % 2 ? To + 1 : -1; text = "size outside 0 .. T_out"; }
        if (fault == 2) { clip[rng() % (unsigned)N] = rng() % 2 ? B : -1; text = "clip outside 0 .. B-1"; }
        if (fault == 3) { lens[rng() % (unsigned)N] = rng() % 2 ? L_stride + 1 : -1; text = "target length outside 0 .. L_stride"; }
        if (fault == 4) {
            int n = -1;
            for (int m = 0; m < N; ++m) if (lens[(size_t)m] > 0) n = m;
            if (n < 0) { text = nullptr; }      // (no token to spoil: a good call after all)
            else { tg[(size_t)n * L_stride + rng() % (unsigned)lens[(size_t)n]] = rng() % 2 ? blank : C; text = "is the blank or not a label"; }
        }
        const bool bad = fault != 0 && text != nullptr && !(fault == 1 && no_sizes);
        const int rc = occ_check(no_sizes ? nullptr : sizes.data(), B, To, clip.data(), ptr_or_null(tg), lens.data(), N, L_stride, C, blank,
                                 sz, tl, frames, base, &L_max, &trellis, err);
        if (bad) {
            if (rc != DSMI_ERR_INVALID) OCC_FAIL("a bad call passed");
            if (err.rfind("occupancy: ", 0) != 0 || err.find(text) == std::string::npos) OCC_FAIL("wrong message");
            ++refused;
        } else {
            if (rc != DSMI_OK) OCC_FAIL("a good call refused");
            if ((int)sz.size() != B || (int)tl.size() != N || (int)frames.size() != N || (int)base.size() != N) OCC_FAIL("the lengths of what the check hands on");
            uint64_t at = 0;
            int want_max = 0;
            for (int n = 0; n < N; ++n) {
                const int T = no_sizes ? To : sizes[(size_t)clip[(size_t)n]], L = lens[(size_t)n];
                const int want = min_frames(tg.data() + (size_t)n * L_stride, L, blank) <= T ? L : -1;
                if (frames[(size_t)n] != T || tl[(size_t)n] != want) OCC_FAIL("frames or feasibility");
                if ((uint64_t)base[(size_t)n] != at) OCC_FAIL("a trellis out of place");
                if (want >= 0) at += (uint64_t)T * (2 * (uint64_t)L + 1);       // [T][S], back to back
                else ++infeasible;
                want_max = std::max(want_max, want);
            }
            if (trellis != at || L_max != want_max) OCC_FAIL("the trellis total or the longest candidate");
            ++good;
        }
        // ---- the stored trellis over the cap: candidates of 1024 tokens on 4096 frames, 2^25 elements hold three of them and not four
        {
            const int n_long = 3 + (int)(rng() % 3), Ll = DSMI_OCC_MAX_TOKENS, Tl = 4096;
            std::vector<int32_t> one = exact(1, Tl), zero = exact((size_t)n_long, 0), full = exact((size_t)n_long, Ll), rows = exact((size_t)n_long * Ll);
            for (size_t i = 0; i < rows.size(); ++i) rows[i] = (int32_t)((blank + 1 + (int)(i & 1)) % C == blank ? (blank + 2) % C : (blank + 1 + (int)(i & 1)) % C);
            const int rc2 = occ_check(one.data(), 1, Tl, zero.data(), rows.data(), full.data(), n_long, Ll, C, blank, sz, tl, frames, base, &L_max, &trellis, err);
            const uint64_t want = (uint64_t)n_long * Tl * (2 * (uint64_t)Ll + 1);
            if (C > 2) {      // (two labels: one token label alone, no row of alternating tokens)
                if (want > ((uint64_t)1 << 25) ? (rc2 != DSMI_ERR_CAPACITY || err.find("2^25") == std::string::npos) : rc2 != DSMI_OK) OCC_FAIL("the trellis cap");
            }
        }
        // ---- refused on the numbers alone: no array exists
        {
            const int32_t* none = nullptr;
            const int big = 1 + (int)(rng() % 1000);
            if (occ_check(none, 0, To, none, none, none, N, 3, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_INVALID) OCC_FAIL("B = 0");
            if (occ_check(none, B, -big, none, none, none, N, 3, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_INVALID) OCC_FAIL("T_out < 0");
            if (occ_check(none, B, To, none, none, none, 0, 3, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_INVALID) OCC_FAIL("N = 0");
            if (occ_check(none, B, To, none, none, none, big, -1, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_INVALID) OCC_FAIL("L_stride < 0");
            if (occ_check(none, B, To, none, none, none, big, DSMI_OCC_MAX_TOKENS + big, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_CAPACITY ||
                err.find("DSMI_OCC_MAX_TOKENS") == std::string::npos) OCC_FAIL("L_stride over the limit");
            if (occ_check(none, B, To, none, none, none, (1 << 24) / 1024 + big, 1024, C, blank, sz, tl, frames, base, &L_max, &trellis, err) != DSMI_ERR_CAPACITY ||
                err.find("2^24") == std::string::npos) OCC_FAIL("N * L_stride over 2^24");
        }
    }
    std::printf("%d occupancy calls ok, %ld good, %ld refused, %ld infeasible candidates\n", reps, good, refused, infeasible);
    return good > 0 && refused > 0 ? 0 : 11;
}

// ---- grammarcheck: dsmi_grammar's check and plan (grammar_host.h), every array of the pool a heap block of exactly the size the
// offsets declare
#define GR_FAIL(what) do { std::fprintf(stderr, "grammarcheck: %s (repetition %d, line %d): %s\n", what, rep, __LINE__, err.c_str()); return 11; } while (0)

static int run_grammarcheck(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long good = 0, refused = 0, empty_graphs = 0;
    for (int rep = 0; rep < reps; ++rep) {
        const int C = 2 + (int)(rng() % 127), blank = (int)(rng() % (unsigned)C);
        const int B = 1 + (int)(rng() % 6), To = 1 + (int)(rng() % 40), K = 1 + (int)(rng() % 4);
        std::string err;
        // ---- a whole pool: graph g of n[g] nodes, every node a label, flags, a weight and up to 4 predecessors
        std::vector<int32_t> node_off = exact((size_t)K + 1);
        for (int g = 0; g < K; ++g) node_off[(size_t)g + 1] = node_off[(size_t)g] + (int32_t)(rng() % 4 == 0 ? 0 : 1 + rng() % 9);
        const int total = node_off[(size_t)K];
        std::vector<int32_t> labels = exact((size_t)total), flags = exact((size_t)total), arc_off = exact((size_t)total + 1), empty_ok = exact((size_t)K);
        std::vector<float> weights((size_t)total);
        weights.shrink_to_fit();
        std::vector<int32_t> preds;
        for (int g = 0; g < K; ++g) {
            const int n0 = node_off[(size_t)g], N = node_off[(size_t)g + 1] - n0;
            empty_ok[(size_t)g] = (int32_t)(rng() % 2);
            if (N == 0) ++empty_graphs;
            for (int n = 0; n < N; ++n) {
                int lab = (int)(rng() % (unsigned)C);
                if (lab == blank) lab = (blank + 1) % C;
                labels[(size_t)(n0 + n)] = lab;
                flags[(size_t)(n0 + n)] = (int32_t)(rng() % 4);
                weights[(size_t)(n0 + n)] = -(float)(rng() % 1000) / 250.f;
                const int fan = (int)(rng() % 5);
                for (int j = 0; j < fan; ++j) preds.push_back((int32_t)(rng() % (unsigned)N));      // self-loops and cycles are legal
                arc_off[(size_t)(n0 + n) + 1] = (int32_t)preds.size();
            }
            if (N > 0) { flags[(size_t)n0 + rng() % (unsigned)N] |= DSMI_GRAMMAR_START; flags[(size_t)n0 + rng() % (unsigned)N] |= DSMI_GRAMMAR_FINAL; }
        }
        std::vector<int32_t> arc_pred(preds);
        arc_pred.shrink_to_fit();
        std::vector<int32_t> sizes = exact((size_t)B), clip_graph = exact((size_t)B);
        for (auto& v : sizes) v = (int32_t)(rng() % (unsigned)(To + 1));
        for (auto& v : clip_graph) v = (int32_t)(rng() % (unsigned)K);
        const bool no_sizes = rng() % 5 == 0, no_weights = rng() % 4 == 0, no_clip_graph = rng() % 5 == 0;
        // ---- with `fault` one thing is wrong with the call, and the rule that refuses it is written out here
        int fault = rng() % 2 ? 0 : 1 + (int)(rng() % 10);
        const char* text = "";
        int g_big = -1;                  // a graph with nodes
        for (int g = 0; g < K; ++g) if (node_off[(size_t)g + 1] > node_off[(size_t)g]) g_big = g;
        const int n0 = g_big >= 0 ? node_off[(size_t)g_big] : 0, Nb = g_big >= 0 ? node_off[(size_t)g_big + 1] - n0 : 0;
        if (fault >= 5 && g_big < 0) fault = 0;
        if (fault == 1) { if (no_sizes) fault = 0; else { sizes[rng() % (unsigned)B] = rng() % 2 ? To + 1 : -1; text = "size outside 0 .. T_out"; } }
        if (fault == 2) { if (no_clip_graph) fault = 0; else { clip_graph[rng() % (unsigned)B] = rng() % 2 ? K : -1; text = "graph outside 0 .. K-1"; } }
        if (fault == 3) { node_off[0] = 1; text = "node_off[0] must be 0"; }
        if (fault == 4) { arc_off[0] = -1; text = "arc_off[0] must be 0"; }
        if (fault == 5) {                // the last graph with nodes ends before it starts: nothing behind the offsets is read
            node_off[(size_t)g_big + 1] = node_off[(size_t)g_big] - 1;
            if (node_off[(size_t)g_big + 1] < 0 || g_big + 1 != K) { node_off[(size_t)g_big + 1] = n0 + Nb; fault = 0; } else text = "node offsets not ascending";
        }
        if (fault == 6) { labels[(size_t)n0 + rng() % (unsigned)Nb] = rng() % 2 ? blank : C; text = "is the blank or not a label"; }
        if (fault == 7) {
            const int n = n0 + (int)(rng() % (unsigned)Nb);
            if (arc_off[(size_t)n + 1] == arc_off[(size_t)n]) fault = 0;
            else { arc_pred[(size_t)arc_off[(size_t)n]] = rng() % 2 ? Nb : -1; text = "outside the graph"; }
        }
        if (fault == 8) { if (no_weights) fault = 0; else { weights[(size_t)n0 + rng() % (unsigned)Nb] = rng() % 2 ? NAN : -INFINITY; text = "weight is not finite"; } }
        if (fault == 9) { for (int n = 0; n < Nb; ++n) flags[(size_t)(n0 + n)] &= ~DSMI_GRAMMAR_START; text = "no start node"; }
        if (fault == 10) { for (int n = 0; n < Nb; ++n) flags[(size_t)(n0 + n)] &= ~DSMI_GRAMMAR_FINAL; text = "no final node"; }
        std::vector<int32_t> sz, cg;
        int n_nodes = -7, n_arcs = -7;
        const int rc = grammar_check(no_sizes ? nullptr : sizes.data(), B, To, K, node_off.data(), ptr_or_null(labels), no_weights || weights.empty() ? nullptr : weights.data(),
                                     ptr_or_null(flags), arc_off.data(), ptr_or_null(arc_pred), empty_ok.data(), no_clip_graph ? nullptr : clip_graph.data(),
                                     C, blank, sz, cg, &n_nodes, &n_arcs, err);
        if (fault) {
            if (rc != DSMI_ERR_INVALID) GR_FAIL("a bad call passed");
            if (err.rfind("grammar: ", 0) != 0 || err.find(text) == std::string::npos) GR_FAIL("wrong message");
            ++refused;
        } else {
            if (rc != DSMI_OK) GR_FAIL("a good call refused");
            if ((int)sz.size() != B || (int)cg.size() != B) GR_FAIL("the lengths of what the check hands on");
            int want_nodes = 0, want_arcs = 0;
            for (int g = 0; g < K; ++g) {
                want_nodes = std::max(want_nodes, node_off[(size_t)g + 1] - node_off[(size_t)g]);
                want_arcs = std::max(want_arcs, arc_off[(size_t)node_off[(size_t)g + 1]] - arc_off[(size_t)node_off[(size_t)g]]);
            }
            if (n_nodes != want_nodes || n_arcs != want_arcs) GR_FAIL("the largest graph");
            for (int b = 0; b < B; ++b)
                if (sz[(size_t)b] != (no_sizes ? To : sizes[(size_t)b]) || cg[(size_t)b] != (no_clip_graph ? 0 : clip_graph[(size_t)b])) GR_FAIL("sizes or graphs");
            GrammarPlan plan{};
            if (grammar_plan(B, To, n_nodes, n_arcs, &plan, err) != DSMI_OK) GR_FAIL("the plan of a good call");
            if (plan.node_stride < n_nodes || plan.node_stride % 4 || plan.node_stride < 4 || plan.node_stride > n_nodes + 4) GR_FAIL("the node stride");
            if (plan.bp_bytes != 2 * (int64_t)B * To * plan.node_stride) GR_FAIL("the backpointer bytes");
            if (plan.lds_bytes != 26 * plan.node_stride + 8 + 2 * ((n_arcs + 3) / 4 * 4) + 16384 || plan.lds_bytes > 160 * 1024) GR_FAIL("the LDS bytes");
            ++good;
        }
        // ---- one node and one arc over the limits: a single graph, offsets alone (the check refuses before it reads a node)
        {
            std::vector<int32_t> off2 = exact(2);
            off2[1] = DSMI_GRAMMAR_MAX_NODES + 1;
            std::vector<int32_t> aoff = exact((size_t)DSMI_GRAMMAR_MAX_NODES + 2, 0), one = exact(1, 0);
            const int32_t* none = nullptr;
            if (grammar_check(none, B, To, 1, off2.data(), none, nullptr, none, aoff.data(), none, one.data(), none, C, blank, sz, cg, &n_nodes, &n_arcs, err) != DSMI_ERR_CAPACITY ||
                err.find("DSMI_GRAMMAR_MAX_NODES") == std::string::npos) GR_FAIL("one node over the limit");
            off2[1] = 2;
            std::vector<int32_t> a3 = exact(3, 0);
            a3[1] = 5; a3[2] = DSMI_GRAMMAR_MAX_ARCS + 1;
            if (grammar_check(none, B, To, 1, off2.data(), none, nullptr, none, a3.data(), none, one.data(), none, C, blank, sz, cg, &n_nodes, &n_arcs, err) != DSMI_ERR_CAPACITY ||
                err.find("DSMI_GRAMMAR_MAX_ARCS") == std::string::npos) GR_FAIL("one arc over the limit");
            a3[2] = 4;
            if (grammar_check(none, B, To, 1, off2.data(), none, nullptr, none, a3.data(), none, one.data(), none, C, blank, sz, cg, &n_nodes, &n_arcs, err) != DSMI_ERR_INVALID ||
                err.find("arc offsets not ascending") == std::string::npos) GR_FAIL("arc offsets that descend");
            GrammarPlan plan{};
            if (grammar_plan(B, To, DSMI_GRAMMAR_MAX_NODES + 1, 0, &plan, err) != DSMI_ERR_CAPACITY) GR_FAIL("the plan, one node over");
            if (grammar_plan(B, To, 1, DSMI_GRAMMAR_MAX_ARCS + 1, &plan, err) != DSMI_ERR_CAPACITY) GR_FAIL("the plan, one arc over");
            if (grammar_plan(B, To, DSMI_GRAMMAR_MAX_NODES, DSMI_GRAMMAR_MAX_ARCS, &plan, err) != DSMI_OK || plan.lds_bytes > 160 * 1024) GR_FAIL("the plan at both limits");
            if (grammar_plan(1 << 10, 1 << 10, DSMI_GRAMMAR_MAX_NODES, 0, &plan, err) != DSMI_ERR_CAPACITY || err.find("2^31") == std::string::npos) GR_FAIL("the backpointer cap");
        }
        // ---- refused on the numbers alone: no array exists
        {
            const int32_t* none = nullptr;
            const int big = 1 + (int)(rng() % 1000);
            if (grammar_check(none, 0, To, K, none, none, nullptr, none, none, none, none, none, C, blank, sz, cg, &n_nodes, &n_arcs, err) != DSMI_ERR_INVALID) GR_FAIL("B = 0");
            if (grammar_check(none, B, -big, K, none, none, nullptr, none, none, none, none, none, C, blank, sz, cg, &n_nodes, &n_arcs, err) != DSMI_ERR_INVALID) GR_FAIL("T_out < 0");
            if (grammar_check(none, B, To, 0, none, none, nullptr, none, none, none, none, none, C, blank, sz, cg, &n_nodes, &n_arcs, err) != DSMI_ERR_INVALID) GR_FAIL("K = 0");
            if (grammar_check(none, B, To, -big, none, none, nullptr, none, none, none, none, none, C, blank, sz, cg, &n_nodes, &n_arcs, err) != DSMI_ERR_INVALID) GR_FAIL("K < 0");
            if (grammar_check(none, B, To, (1 << 24) + big, none, none, nullptr, none, none, none, none, none, C, blank, sz, cg, &n_nodes, &n_arcs, err) != DSMI_ERR_CAPACITY) GR_FAIL("K over 2^24");
            GrammarPlan plan{};
            if (grammar_plan(0, To, 1, 1, &plan, err) != DSMI_ERR_INVALID || grammar_plan(B, 0, 1, 1, &plan, err) != DSMI_ERR_INVALID ||
                grammar_plan(B, To, -big, 1, &plan, err) != DSMI_ERR_INVALID || grammar_plan(B, To, 1, -big, &plan, err) != DSMI_ERR_INVALID) GR_FAIL("the plan's numbers");
        }
    }
    std::printf("%d grammar calls ok, %ld good, %ld refused, %ld empty graphs\n", reps, good, refused, empty_graphs);
    return good > 0 && refused > 0 ? 0 : 11;
}

// ---- grammarpostcheck: dsmi_grammar_posterior's check, plan and packing (grammar_post_host.h) -- the transposed arcs, the start
// lists and the label buckets against a plain restatement -- every array of the pool a heap block of exactly the size the
// offsets declare
#define GP_FAIL(what) do { std::fprintf(stderr, "grammarpostcheck: %s (repetition %d, line %d): %s\n", what, rep, __LINE__, err.c_str()); return 11; } while (0)

static int run_grammarpostcheck(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long good = 0, refused = 0, arcs_seen = 0;
    for (int rep = 0; rep < reps; ++rep) {
        const int C = 2 + (int)(rng() % 127), blank = (int)(rng() % (unsigned)C);
        const int B = 1 + (int)(rng() % 6), To = 1 + (int)(rng() % 40), K = 1 + (int)(rng() % 4);
        std::string err;
        std::vector<int32_t> node_off = exact((size_t)K + 1);
        for (int g = 0; g < K; ++g) node_off[(size_t)g + 1] = node_off[(size_t)g] + (int32_t)(rng() % 4 == 0 ? 0 : 1 + rng() % 9);
        const int total = node_off[(size_t)K];
        std::vector<int32_t> labels = exact((size_t)total), flags = exact((size_t)total), arc_off = exact((size_t)total + 1), empty_ok = exact((size_t)K);
        std::vector<float> weights((size_t)total);
        weights.shrink_to_fit();
        std::vector<int32_t> preds;
        int n_most = 0;
        for (int g = 0; g < K; ++g) {
            const int n0 = node_off[(size_t)g], N = node_off[(size_t)g + 1] - n0;
            n_most = std::max(n_most, N);
            empty_ok[(size_t)g] = (int32_t)(rng() % 2);
            for (int n = 0; n < N; ++n) {
                int lab = (int)(rng() % (unsigned)std::min(C, 4));        // few labels: equal neighbours and full buckets
                if (lab == blank) lab = (blank + 1) % C;
                labels[(size_t)(n0 + n)] = lab;
                flags[(size_t)(n0 + n)] = (int32_t)(rng() % 4);
                weights[(size_t)(n0 + n)] = (float)((int)(rng() % 2000) - 1000) / 250.f;
                const int fan = (int)(rng() % 5);
                for (int j = 0; j < fan; ++j) preds.push_back((int32_t)(rng() % (unsigned)N));      // self-loops, cycles, an arc twice
                arc_off[(size_t)(n0 + n) + 1] = (int32_t)preds.size();
            }
            if (N > 0) { flags[(size_t)n0 + rng() % (unsigned)N] |= DSMI_GRAMMAR_START; flags[(size_t)n0 + rng() % (unsigned)N] |= DSMI_GRAMMAR_FINAL; }
        }
        std::vector<int32_t> arc_pred(preds);
        arc_pred.shrink_to_fit();
        std::vector<int32_t> sizes = exact((size_t)B), clip_graph = exact((size_t)B);
        for (auto& v : sizes) v = (int32_t)(rng() % (unsigned)(To + 1));
        for (auto& v : clip_graph) v = (int32_t)(rng() % (unsigned)K);
        const bool want_visits = rng() % 3 != 0;
        int N_stride = n_most + (int)(rng() % 3);
        // ---- with `fault` one thing is wrong with the call
        int fault = rng() % 2 ? 0 : 1 + (int)(rng() % 4), code = DSMI_ERR_INVALID;
        const char* text = "";
        if (fault == 1) { sizes[rng() % (unsigned)B] = To + 1; text = "size outside 0 .. T_out"; }
        if (fault == 2) { if (total == 0) fault = 0; else { labels[rng() % (unsigned)total] = blank; text = "is the blank or not a label"; } }
        if (fault == 3) { if (!want_visits || n_most == 0) fault = 0; else { N_stride = n_most - 1; text = "is below the pool's largest graph"; } }
        if (fault == 4) { if (total == 0) fault = 0; else { clip_graph[rng() % (unsigned)B] = K; text = "graph outside 0 .. K-1"; } }
        std::vector<int32_t> sz, cg;
        int n_nodes = -7, n_arcs = -7;
        GrammarPostPlan plan{};
        const int rc = grammar_post_check(sizes.data(), B, To, K, node_off.data(), ptr_or_null(labels), weights.empty() ? nullptr : weights.data(), ptr_or_null(flags),
                                          arc_off.data(), ptr_or_null(arc_pred), empty_ok.data(), clip_graph.data(), C, blank, want_visits, N_stride, sz, cg,
                                          &n_nodes, &n_arcs, &plan, err);
        if (fault) {
            if (rc != code) GP_FAIL("a bad call passed");
            if (err.rfind("grammar", 0) != 0 || err.find(text) == std::string::npos) GP_FAIL("wrong message");
            ++refused;
        } else {
            if (rc != DSMI_OK) GP_FAIL("a good call refused");
            if (n_nodes != n_most) GP_FAIL("the largest graph");
            // ---- the plan's numbers
            if (plan.node_stride < n_nodes || plan.node_stride % 4 || plan.node_stride < 4 || plan.node_stride > n_nodes + 4) GP_FAIL("the node stride");
            if (plan.ws_bytes != (int64_t)B * To * (32 * plan.node_stride + 16)) GP_FAIL("the workspace bytes");
            if (plan.lds_bytes != 44 * plan.node_stride + 8 + 2 * ((n_arcs + 3) / 4 * 4) + 32768 + 2048 + 2 * (DSMI_GRAMMAR_MAX_ARCS / 25 + 1) + 8 || plan.lds_bytes > 160 * 1024) GP_FAIL("the LDS bytes");
            // ---- the packing against a plain restatement
            GrammarPostPack pk;
            grammar_post_pack(K, node_off.data(), ptr_or_null(labels), ptr_or_null(flags), arc_off.data(), ptr_or_null(arc_pred), C, pk);
            if (pk.words.size() != (size_t)total || pk.arc16.size() != arc_pred.size() || pk.succ16.size() != arc_pred.size() ||
                pk.succ_off.size() != (size_t)total + 1 || pk.start_off.size() != (size_t)K + 1 || pk.bucket_off.size() != (size_t)K * (C + 1) ||
                pk.bucket_nodes.size() != (size_t)total || pk.succ_off[0] != 0 || pk.succ_off[(size_t)total] != (int32_t)arc_pred.size()) GP_FAIL("the sizes of the pack");
            int fan_most = 0;
            for (int g = 0; g < K; ++g) {
                const int n0 = node_off[(size_t)g], N = node_off[(size_t)g + 1] - n0;
                std::vector<int> starts;
                for (int n = 0; n < N; ++n) {
                    const int i = n0 + n;
                    if (pk.words[(size_t)i] != (labels[(size_t)i] | ((flags[(size_t)i] & 1) << 8) | ((flags[(size_t)i] & 2) << 8))) GP_FAIL("a node word");
                    if (flags[(size_t)i] & DSMI_GRAMMAR_START) starts.push_back(n);
                    fan_most = std::max(fan_most, arc_off[(size_t)i + 1] - arc_off[(size_t)i]);
                    // the successors of n: every arc p -> s with p == n, the successors ascending, an arc listed twice twice
                    std::vector<int> want;
                    for (int s2 = 0; s2 < N; ++s2)
                        for (int j = arc_off[(size_t)(n0 + s2)]; j < arc_off[(size_t)(n0 + s2) + 1]; ++j)
                            if (arc_pred[(size_t)j] == n) want.push_back(s2 | (labels[(size_t)(n0 + s2)] != labels[(size_t)i] ? 0x8000 : 0));
                    if (pk.succ_off[(size_t)i + 1] - pk.succ_off[(size_t)i] != (int32_t)want.size()) GP_FAIL("a successor count");
                    for (size_t k = 0; k < want.size(); ++k)
                        if (pk.succ16[(size_t)pk.succ_off[(size_t)i] + k] != want[k]) GP_FAIL("a successor");
                    for (int j = arc_off[(size_t)i]; j < arc_off[(size_t)i + 1]; ++j) {
                        const int p = arc_pred[(size_t)j];
                        if (pk.arc16[(size_t)j] != (p | (labels[(size_t)(n0 + p)] != labels[(size_t)i] ? 0x8000 : 0))) GP_FAIL("a predecessor word");
                    }
                    arcs_seen += (long)want.size();
                }
                if (pk.start_off[(size_t)g + 1] - pk.start_off[(size_t)g] != (int32_t)starts.size()) GP_FAIL("a start count");
                for (size_t k = 0; k < starts.size(); ++k)
                    if (pk.start16[(size_t)pk.start_off[(size_t)g] + k] != starts[k]) GP_FAIL("a start node");
                const int32_t* bo = pk.bucket_off.data() + (size_t)g * (C + 1);
                if (bo[0] != 0 || bo[C] != N) GP_FAIL("the bucket offsets' ends");
                for (int c = 0; c < C; ++c) {
                    std::vector<int> want;
                    for (int n = 0; n < N; ++n) if (labels[(size_t)(n0 + n)] == c) want.push_back(n);
                    if (bo[c + 1] - bo[c] != (int32_t)want.size()) GP_FAIL("a bucket's count");
                    for (size_t k = 0; k < want.size(); ++k)
                        if (pk.bucket_nodes[(size_t)n0 + bo[c] + k] != want[k]) GP_FAIL("a bucket's node");
                }
            }
            if (pk.max_fan_in != fan_most) GP_FAIL("the largest fan-in");
            ++good;
        }
        // ---- the plan: limits, the cap, and what the numbers alone refuse (no array exists)
        {
            const int32_t* none = nullptr;
            const int big = 1 + (int)(rng() % 1000);
            if (grammar_post_plan(B, To, DSMI_GRAMMAR_MAX_NODES + 1, 0, &plan, err) != DSMI_ERR_CAPACITY || err.find("DSMI_GRAMMAR_MAX_NODES") == std::string::npos) GP_FAIL("the plan, one node over");
            if (grammar_post_plan(B, To, 1, DSMI_GRAMMAR_MAX_ARCS + 1, &plan, err) != DSMI_ERR_CAPACITY || err.find("DSMI_GRAMMAR_MAX_ARCS") == std::string::npos) GP_FAIL("the plan, one arc over");
            if (grammar_post_plan(32, 501, DSMI_GRAMMAR_MAX_NODES, DSMI_GRAMMAR_MAX_ARCS, &plan, err) != DSMI_OK || plan.lds_bytes > 160 * 1024 || plan.ws_bytes > ((int64_t)1 << 30)) GP_FAIL("the plan at both limits");
            if (grammar_post_plan(33, 501, DSMI_GRAMMAR_MAX_NODES, 0, &plan, err) != DSMI_ERR_CAPACITY || err.find("2^30") == std::string::npos) GP_FAIL("the cap");
            if (grammar_post_plan(0, To, 1, 1, &plan, err) != DSMI_ERR_INVALID || grammar_post_plan(B, -big, 1, 1, &plan, err) != DSMI_ERR_INVALID ||
                grammar_post_plan(B, To, -big, 1, &plan, err) != DSMI_ERR_INVALID || grammar_post_plan(B, To, 1, -big, &plan, err) != DSMI_ERR_INVALID) GP_FAIL("the plan's numbers");
            if (grammar_post_check(none, 0, To, K, none, none, nullptr, none, none, none, none, none, C, blank, true, 0, sz, cg, &n_nodes, &n_arcs, &plan, err) != DSMI_ERR_INVALID) GP_FAIL("B = 0");
            if (grammar_post_check(none, B, To, 0, none, none, nullptr, none, none, none, none, none, C, blank, true, 0, sz, cg, &n_nodes, &n_arcs, &plan, err) != DSMI_ERR_INVALID) GP_FAIL("K = 0");
            if (grammar_post_check(none, 1 << 12, (1 << 12) + big, K, none, none, nullptr, none, none, none, none, none, C, blank, true, 0, sz, cg, &n_nodes, &n_arcs, &plan, err) != DSMI_ERR_CAPACITY ||
                err.find("stored trellises") == std::string::npos) GP_FAIL("the cap on the numbers alone");
        }
    }
    std::printf("%d posterior calls ok, %ld good, %ld refused, %ld arcs transposed\n", reps, good, refused, arcs_seen);
    return good > 0 && refused > 0 && arcs_seen > 0 ? 0 : 11;
}

// ---- grammarstreamcheck: the plan of a stream's block, the heavy list and the check of an advance call (grammar_stream_host.h),
// every array a heap block of exactly n entries
#define GS_FAIL(what) do { std::fprintf(stderr, "grammarstreamcheck: %s (repetition %d, line %d): %s\n", what, rep, __LINE__, err.c_str()); return 11; } while (0)

static int run_grammarstreamcheck(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long good = 0, refused = 0, heavy_nodes = 0;
    for (int rep = 0; rep < reps; ++rep) {
        std::string err;
        // ---- the plan: the rules written out plainly
        {
            const int N = (int)(rng() % (DSMI_GRAMMAR_MAX_NODES + 1)), A = (int)(rng() % (DSMI_GRAMMAR_MAX_ARCS + 1));
            const int C = 1 + (int)(rng() % kCtcMaxLabels), F = 1 + (int)(rng() % 3000);
            GrammarStreamPlan p{};
            if (grammar_stream_plan(N, A, C, F, &p, err) != DSMI_OK) GS_FAIL("the plan of good numbers");
            const int64_t stride = std::max(4, (N + 3) / 4 * 4);
            const int64_t lds = 16 * stride + 8 * stride + 2 * (stride + 4) + 2 * (int64_t)((A + 3) / 4 * 4) + 2 * 4 * kCtcChunk * kCtcMaxLabels + 512;
            const int64_t bytes = 16 + 8 * stride + 4 * (int64_t)F * C + 2 * (int64_t)F * stride;
            if (p.node_stride != stride || p.lds_bytes != lds || p.block_bytes != bytes) GS_FAIL("the plan's numbers");
            if (p.pairs_at != 16 || p.hist_at != 16 + 8 * stride || p.bp_at != p.hist_at + 4 * (int64_t)F * C || p.bp_at % 4 != 0) GS_FAIL("the block's layout");
            if (grammar_stream_plan(N, A, C, 0, &p, err) != DSMI_ERR_INVALID || grammar_stream_plan(N, A, C, -F, &p, err) != DSMI_ERR_INVALID) GS_FAIL("max_frames < 1");
            if (grammar_stream_plan(N, A, C, DSMI_GRAMMAR_STREAM_MAX_FRAMES + 1, &p, err) != DSMI_ERR_CAPACITY) GS_FAIL("max_frames over the limit");
            if (grammar_stream_plan(N, A, 0, F, &p, err) != DSMI_ERR_INVALID || grammar_stream_plan(N, A, kCtcMaxLabels + 1, F, &p, err) != DSMI_ERR_INVALID) GS_FAIL("n_labels");
            if (grammar_stream_plan(DSMI_GRAMMAR_MAX_NODES + 1, A, C, F, &p, err) != DSMI_ERR_CAPACITY || grammar_stream_plan(N, DSMI_GRAMMAR_MAX_ARCS + 1, C, F, &p, err) != DSMI_ERR_CAPACITY) GS_FAIL("one over a limit");
            if (grammar_stream_plan(-1, A, C, F, &p, err) != DSMI_ERR_INVALID || grammar_stream_plan(N, -1, C, F, &p, err) != DSMI_ERR_INVALID) GS_FAIL("negative counts");
            if (grammar_stream_plan(DSMI_GRAMMAR_MAX_NODES, 0, 128, DSMI_GRAMMAR_STREAM_MAX_FRAMES, &p, err) != DSMI_ERR_CAPACITY || err.find("2^31") == std::string::npos) GS_FAIL("the block cap");
            if (grammar_stream_plan(DSMI_GRAMMAR_MAX_NODES, DSMI_GRAMMAR_MAX_ARCS, 128, 1500, &p, err) != DSMI_OK || p.lds_bytes > 160 * 1024) GS_FAIL("the plan at both limits");
        }
        // ---- the heavy list of a pool: nodes with more than 32 predecessors, graph-local, ascending
        {
            const int K = 1 + (int)(rng() % 3);
            std::vector<int32_t> node_off = exact((size_t)K + 1);
            for (int g = 0; g < K; ++g) node_off[(size_t)g + 1] = node_off[(size_t)g] + (int32_t)(rng() % 12);
            const int total = node_off[(size_t)K];
            std::vector<int32_t> arc_off = exact((size_t)total + 1);
            for (int i = 0; i < total; ++i) arc_off[(size_t)i + 1] = arc_off[(size_t)i] + (int32_t)(rng() % 3 == 0 ? 31 + rng() % 4 : rng() % 5);
            std::vector<int32_t> hoff;
            std::vector<uint16_t> heavy;
            grammar_heavy_list(K, node_off.data(), arc_off.data(), hoff, heavy);
            size_t at = 0;
            if (hoff.size() != (size_t)K + 1 || hoff[0] != 0) GS_FAIL("the heavy offsets");
            for (int g = 0; g < K; ++g) {
                for (int i = node_off[(size_t)g]; i < node_off[(size_t)g + 1]; ++i)
                    if (arc_off[(size_t)i + 1] - arc_off[(size_t)i] >= 33) {
                        if (at >= heavy.size() || heavy[at] != i - node_off[(size_t)g]) GS_FAIL("the heavy list");
                        ++at; ++heavy_nodes;
                    }
                if (hoff[(size_t)g + 1] != (int32_t)at) GS_FAIL("the heavy offsets");
            }
            if (at != heavy.size()) GS_FAIL("the heavy list's length");
        }
        // ---- an advance call of n streams
        const int n = 1 + (int)(rng() % 8);
        std::vector<int> tokens((size_t)n + 1);      // (addresses to stand for handles and nets)
        std::vector<const void*> handles((size_t)n), nets((size_t)n), rows_of((size_t)n);
        handles.shrink_to_fit(); nets.shrink_to_fit(); rows_of.shrink_to_fit();
        std::vector<int64_t> consumed((size_t)n);
        consumed.shrink_to_fit();
        std::vector<int32_t> ended = exact((size_t)n), cap = exact((size_t)n), frames = exact((size_t)n), mode = exact((size_t)n);
        static const float some_rows[1] = {0.f};
        int64_t longest = 0;
        for (int i = 0; i < n; ++i) {
            handles[(size_t)i] = &tokens[(size_t)i]; nets[(size_t)i] = &tokens[(size_t)n];
            cap[(size_t)i] = 1 + (int32_t)(rng() % 200);
            consumed[(size_t)i] = (int64_t)(rng() % (unsigned)(cap[(size_t)i] + 1));
            frames[(size_t)i] = (int32_t)(rng() % (unsigned)(cap[(size_t)i] - consumed[(size_t)i] + 1));
            mode[(size_t)i] = (int32_t)(rng() % 3);
            ended[(size_t)i] = frames[(size_t)i] == 0 && rng() % 3 == 0;
            rows_of[(size_t)i] = frames[(size_t)i] > 0 || rng() % 2 ? some_rows : nullptr;
            if (mode[(size_t)i]) longest = std::max(longest, consumed[(size_t)i] + frames[(size_t)i]);
        }
        int P = (int)longest + (int)(rng() % 3);
        bool outputs = true;
        int n_arg = n, code = DSMI_ERR_INVALID;
        bool due = false;
        for (int i = 0; i < n; ++i) due |= mode[(size_t)i] != 0;
        int fault = rng() % 2 ? 0 : 1 + (int)(rng() % 12);
        const int v = (int)(rng() % (unsigned)n);      // the stream at fault
        std::string text;
        auto at = [&](int i) { return "grammar stream " + std::to_string(i) + ": "; };
        // (a fault is placed so that no earlier stream has one: the check names the first)
        if (fault == 1) { n_arg = rng() % 2 ? 0 : DSMI_GRAMMAR_STREAM_MANY_MAX + 1; text = "n outside 1 .. DSMI_GRAMMAR_STREAM_MANY_MAX"; }
        if (fault == 2) { if (n < 2 || v == 0) fault = 0; else { handles[(size_t)v] = handles[(size_t)(v - 1)]; text = at(v) + "the same handle appears twice"; } }
        if (fault == 3) { if (v == 0) fault = 0; else { nets[(size_t)v] = &tokens[0]; text = at(v) + "the streams of one call must belong to one net"; } }
        if (fault == 4) { frames[(size_t)v] = -1 - (int32_t)(rng() % 5); text = at(v) + "negative frame count"; }
        if (fault == 5) { if (frames[(size_t)v] == 0) fault = 0; else { rows_of[(size_t)v] = nullptr; text = at(v) + "no probabilities for " + std::to_string(frames[(size_t)v]) + " frames"; } }
        if (fault == 6) { mode[(size_t)v] = rng() % 2 ? 3 : -1; text = at(v) + "mode " + std::to_string(mode[(size_t)v]) + " outside 0 .. 2"; }
        if (fault == 7) { if (frames[(size_t)v] == 0) fault = 0; else { ended[(size_t)v] = 1; text = at(v) + "the utterance has ended"; } }
        if (fault == 8) {
            frames[(size_t)v] = cap[(size_t)v] - (int32_t)consumed[(size_t)v] + 1; rows_of[(size_t)v] = some_rows; ended[(size_t)v] = 0;
            code = DSMI_ERR_CAPACITY;
            text = at(v) + "the utterance would reach " + std::to_string(cap[(size_t)v] + 1) + " frames, max_frames is " + std::to_string(cap[(size_t)v]);
        }
        if (fault == 9) {
            if (mode[(size_t)v] == 0 || consumed[(size_t)v] + frames[(size_t)v] == 0) fault = 0;
            else {                       // below this stream's count, and no stream before it is above the stride either
                P = (int)(consumed[(size_t)v] + frames[(size_t)v]) - 1;
                for (int i = 0; i < v; ++i) if (mode[(size_t)i] && consumed[(size_t)i] + frames[(size_t)i] > P) mode[(size_t)i] = 0;
                text = at(v) + "P_stride " + std::to_string(P) + " is below the utterance's " + std::to_string(P + 1) + " frames";
            }
        }
        if (fault == 10) { if (!due) fault = 0; else { outputs = false; text = "an output array is NULL"; } }
        if (fault == 11) { if (!due) fault = 0; else { P = (1 << 24) / n + 1; code = DSMI_ERR_CAPACITY; text = "n * P_stride exceeds 2^24"; } }
        if (fault == 12) {               // the numbers alone: no array is read
            if (grammar_stream_check(nullptr, nullptr, nullptr, nullptr, nullptr, -3, nullptr, nullptr, nullptr, 0, true, err) != DSMI_ERR_INVALID) GS_FAIL("n < 0 with no arrays");
            fault = 0;
        }
        const int rc = grammar_stream_check(handles.data(), nets.data(), consumed.data(), ended.data(), cap.data(), n_arg,
                                            reinterpret_cast<const float* const*>(rows_of.data()), frames.data(), mode.data(), P, outputs, err);
        if (fault) {
            if (rc != code) GS_FAIL("a fault with the wrong code");
            if (err.rfind("grammar stream", 0) != 0 || err.find(text) == std::string::npos) GS_FAIL("wrong message");
            ++refused;
        } else {
            if (rc != DSMI_OK) GS_FAIL("a good call refused");
            ++good;
        }
    }
    std::printf("%d grammar stream calls ok, %ld good, %ld refused, %ld heavy nodes\n", reps, good, refused, heavy_nodes);
    return good > 0 && refused > 0 && heavy_nodes > 0 ? 0 : 11;
}

// ---- alignlong: dsmi_align_long's check and plan (align_long_host.h), the transcript a heap block of exactly L words
#define ALONG_FAIL(what) do { std::fprintf(stderr, "alignlong: %s (repetition %d, line %d)\n", what, rep, __LINE__); return 11; } while (0)

static int run_alignlong(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long good = 0, refused = 0, infeasible = 0;
    for (int rep = 0; rep < reps; ++rep) {
        const int C = 2 + (int)(rng() % 127), blank = (int)(rng() % (unsigned)C);
        const int T = 1 + (int)(rng() % 3000), L = rng() % 4 == 0 ? 0 : (int)(rng() % 2500);
        const int lead = (int)(rng() % 2), tail = (int)(rng() % 2);
        std::string err;
        AlongPlan plan{-7, -7, -7, -7, -7, -7};
        bool feasible = false;
        std::vector<int32_t> tg = exact((size_t)L);
        random_row(rng, tg.data(), L, C, blank, false);
        const int fault = rng() % 2 ? 0 : 1 + (int)(rng() % 2);
        const char* text = nullptr;
        int lead_in = lead, tail_in = tail;
        if (fault == 1 && L > 0) { tg[rng() % (unsigned)L] = rng() % 3 == 0 ? blank : rng() % 2 ? C : -1; text = "is the blank or not a label"; }
        if (fault == 2) { (rng() % 2 ? lead_in : tail_in) = rng() % 2 ? 2 : -1; text = "lead_free and tail_free are 0 or 1"; }
        const int rc = align_long_check(T, L, lead_in, tail_in, ptr_or_null(tg), C, blank, &plan, &feasible, err);
        if (text) {
            if (rc != DSMI_ERR_INVALID) ALONG_FAIL("a bad call passed");
            if (err.rfind("align_long: ", 0) != 0 || err.find(text) == std::string::npos) ALONG_FAIL("wrong message");
            ++refused;
        } else {
            if (rc != DSMI_OK) ALONG_FAIL("a good call refused");
            if (feasible != (min_frames(tg.data(), L, blank) <= T)) ALONG_FAIL("feasibility");
            infeasible += !feasible;
            // the geometry, written out: tiles that cover the states and the frames behind frame 0, one row more than frame tiles
            const int64_t S = 2 * (int64_t)L + 1;
            if (plan.W < 1 || plan.F < 1) ALONG_FAIL("tile sizes");
            if (plan.state_tiles * plan.W < S || (plan.state_tiles - 1) * plan.W >= S) ALONG_FAIL("state tiles");
            if (plan.frame_tiles * plan.F < T - 1 || (plan.frame_tiles > 0 && (plan.frame_tiles - 1) * plan.F >= T - 1)) ALONG_FAIL("frame tiles");
            if (plan.rows != plan.frame_tiles + 1 || plan.bytes != plan.rows * S * 4) ALONG_FAIL("rows or bytes");
            int64_t info[6] = {-7, -7, -7, -7, -7, -7};
            if (align_long_plan(T, L, info) != DSMI_OK || info[0] != plan.W || info[1] != plan.F || info[2] != plan.state_tiles ||
                info[3] != plan.frame_tiles || info[4] != plan.rows || info[5] != plan.bytes) ALONG_FAIL("the plan is not the check's");
            ++good;
        }
        // ---- refused on the numbers alone: no array exists, nothing is written
        {
            const int32_t* none = nullptr;
            const int big = 1 + (int)(rng() % 1000);
            AlongPlan q{-7, -7, -7, -7, -7, -7};
            int64_t info[6] = {-7, -7, -7, -7, -7, -7};
            bool f = true;
            if (align_long_check(0, L, 0, 0, none, C, blank, &q, &f, err) != DSMI_ERR_INVALID) ALONG_FAIL("T = 0");
            if (align_long_check(-big, big, 1, 1, none, C, blank, &q, &f, err) != DSMI_ERR_INVALID) ALONG_FAIL("T < 0");
            if (align_long_check(T, -big, 0, 1, none, C, blank, &q, &f, err) != DSMI_ERR_INVALID) ALONG_FAIL("L < 0");
            if (align_long_check(T, big, 2, 0, none, C, blank, &q, &f, err) != DSMI_ERR_INVALID) ALONG_FAIL("a flag of 2");
            if (align_long_check(T, DSMI_ALIGN_LONG_MAX_TOKENS + big, 0, 0, none, C, blank, &q, &f, err) != DSMI_ERR_CAPACITY ||
                err.find("DSMI_ALIGN_LONG_MAX_TOKENS") == std::string::npos) ALONG_FAIL("L over the limit");
            if (align_long_check(DSMI_ALIGN_LONG_MAX_FRAMES + big, big, 0, 0, none, C, blank, &q, &f, err) != DSMI_ERR_CAPACITY ||
                err.find("DSMI_ALIGN_LONG_MAX_FRAMES") == std::string::npos) ALONG_FAIL("T over the limit");
            // the checkpoint rows on either side of 4 GiB: rows of 2L + 1 floats, one per frame tile and one more
            const int Tl = DSMI_ALIGN_LONG_MAX_FRAMES - (int)(rng() % 100000);
            const int64_t rows = align_long_geometry(Tl, 0).rows;
            const int L_fit = (int)((((int64_t)1 << 30) / rows - 1) / 2);      // the most tokens with rows * (2L + 1) * 4 <= 2^32
            if (align_long_check(Tl, L_fit + 1, 0, 0, none, C, blank, &q, &f, err) != DSMI_ERR_CAPACITY ||
                err.find("DSMI_ALIGN_LONG_MAX_WORKSPACE") == std::string::npos) ALONG_FAIL("the workspace over its cap");
            if (q.W != -7 || q.bytes != -7) ALONG_FAIL("a refusal wrote the plan");
            if (align_long_plan(Tl, L_fit + 1, info) != DSMI_ERR_CAPACITY || info[0] != -7 || info[5] != -7) ALONG_FAIL("a refused plan wrote");
            if (align_long_plan(Tl, L_fit, info) != DSMI_OK || info[5] > (int64_t)DSMI_ALIGN_LONG_MAX_WORKSPACE ||
                info[5] + info[4] * 8 <= (int64_t)DSMI_ALIGN_LONG_MAX_WORKSPACE) ALONG_FAIL("the workspace under its cap");
            if (align_long_plan(0, 0, info) != DSMI_ERR_INVALID || align_long_plan(1, -1, info) != DSMI_ERR_INVALID) ALONG_FAIL("the plan's refusals");
            if (!f) ALONG_FAIL("a refusal wrote the feasibility");
        }
    }
    std::printf("%d align_long calls ok, %ld good, %ld refused, %ld infeasible\n", reps, good, refused, infeasible);
    return good > 0 && refused > 0 ? 0 : 11;
}

// ---- editcheck: the rules of include/dsmi.h written out plainly, beside edit_host.h -------------------------------------------
#define EDIT_FAIL(what) do { std::fprintf(stderr, "editcheck: %s (repetition %d, line %d)\n", what, rep, __LINE__); return 11; } while (0)

// D[la][lb] of the packed recurrence, by the full table
static uint32_t edit_table(const int32_t* a, int la, const int32_t* b, int lb) {
    std::vector<uint32_t> D((size_t)(la + 1) * (size_t)(lb + 1));
    auto at = [&](int i, int j) -> uint32_t& { return D[(size_t)i * (size_t)(lb + 1) + (size_t)j]; };
    for (int i = 0; i <= la; ++i) at(i, 0) = (uint32_t)i << 16;
    for (int j = 0; j <= lb; ++j) at(0, j) = (uint32_t)j << 16;
    for (int i = 1; i <= la; ++i)
        for (int j = 1; j <= lb; ++j)
            at(i, j) = std::min(std::min(at(i - 1, j) + 0x10000u, at(i, j - 1) + 0x10000u), at(i - 1, j - 1) + (a[i - 1] == b[j - 1] ? 0u : 0x10001u));
    return at(la, lb);
}

static int run_editcheck(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long pairs_checked = 0, refused = 0;
    for (int rep = 0; rep < reps; ++rep) {
        std::string err;
        const int32_t* none = nullptr;
        // ---- refused on the numbers alone: no array is there to read
        {
            const int big = 1 + (int)(rng() % 1000);
            if (edit_check(none, rng() % 2 ? 0 : -big, 4, none, none, 3, err) != DSMI_ERR_INVALID || err.empty()) EDIT_FAIL("M <= 0");
            if (edit_check(none, 3, 4, none, none, rng() % 2 ? 0 : -big, err) != DSMI_ERR_INVALID) EDIT_FAIL("N <= 0");
            if (edit_check(none, 3, -big, none, none, 3, err) != DSMI_ERR_INVALID) EDIT_FAIL("negative L_stride");
            if (edit_check(none, 3, DSMI_EDIT_MAX_TOKENS + big, none, none, 3, err) != DSMI_ERR_CAPACITY || err.find("DSMI_EDIT_MAX_TOKENS") == std::string::npos) EDIT_FAIL("L_stride above the limit");
            const int Ls = 1 + (int)(rng() % DSMI_EDIT_MAX_TOKENS);
            if (edit_check(none, (int)(((int64_t)1 << 24) / Ls) + big, Ls, none, none, 3, err) != DSMI_ERR_CAPACITY) EDIT_FAIL("M * L_stride above 2^24");
            if (edit_check(none, 3, 4, none, none, (1 << 24) + big, err) != DSMI_ERR_CAPACITY) EDIT_FAIL("N above 2^24");
            if (edit_check(none, INT32_MAX, DSMI_EDIT_MAX_TOKENS, none, none, INT32_MAX, err) != DSMI_ERR_CAPACITY) EDIT_FAIL("the largest numbers");
        }
        // ---- a random call: a pool of few symbols, lengths around the segment and stripe edges, pairs that share rows
        const int M = 1 + (int)(rng() % 12), N = 1 + (int)(rng() % 40);
        const int edges[10] = {0, 1, 15, 16, 17, 32, 33, 64, 65, 130};
        const int L_stride = rng() % 8 == 0 ? 0 : edges[rng() % 10] + (int)(rng() % 3);
        std::vector<int32_t> seqs = exact((size_t)M * (size_t)L_stride), lens = exact((size_t)M), pa = exact((size_t)N), pb = exact((size_t)N);
        const int symbols = 1 + (int)(rng() % 4);
        for (auto& v : seqs) v = (int32_t)(rng() % (unsigned)symbols) - 1;
        for (auto& v : lens) v = rng() % 4 == 0 ? 0 : (int32_t)(rng() % (unsigned)(L_stride + 1));
        for (auto& v : pa) v = (int32_t)(rng() % (unsigned)M);
        for (auto& v : pb) v = (int32_t)(rng() % (unsigned)M);
        const int spoil = (int)(rng() % 6);
        int want = DSMI_OK;
        if (spoil == 1) { lens[rng() % (unsigned)M] = rng() % 2 ? L_stride + 1 + (int32_t)(rng() % 3) : -1 - (int32_t)(rng() % 3); want = DSMI_ERR_INVALID; }
        if (spoil == 2) { (rng() % 2 ? pa : pb)[rng() % (unsigned)N] = rng() % 2 ? M + (int32_t)(rng() % 3) : -1 - (int32_t)(rng() % 3); want = DSMI_ERR_INVALID; }
        const int rc = edit_check(lens.data(), M, L_stride, pa.data(), pb.data(), N, err);
        if (rc != want) EDIT_FAIL("a call's verdict");
        if (rc != DSMI_OK) {
            if (err.empty()) EDIT_FAIL("a refusal without a message");
            ++refused;
            continue;
        }
        // ---- the plan: seg by len_b, the pairs with both sides non-empty, every neighbouring pair in the documented order
        std::vector<int32_t> la = exact((size_t)N), lb = exact((size_t)N), order = exact((size_t)N + 1, -7), seg = exact((size_t)N + 1, -7);
        for (int n = 0; n < N; ++n) { la[(size_t)n] = lens[(size_t)pa[(size_t)n]]; lb[(size_t)n] = lens[(size_t)pb[(size_t)n]]; }
        const int n_launch = edit_plan(la.data(), lb.data(), N, order.data(), seg.data());
        if (order[(size_t)N] != -7 || seg[(size_t)N] != -7) EDIT_FAIL("plan: a write past its arrays");
        int want_launch = 0;
        for (int n = 0; n < N; ++n) {
            if (seg[(size_t)n] != (lb[(size_t)n] <= 16 ? 16 : lb[(size_t)n] <= 32 ? 32 : 64)) EDIT_FAIL("plan: seg");
            want_launch += la[(size_t)n] > 0 && lb[(size_t)n] > 0;
        }
        if (n_launch != want_launch) EDIT_FAIL("plan: the number launched");
        std::vector<int> seen((size_t)N, 0);
        auto key = [&](int32_t x, long long* k) {
            k[0] = seg[(size_t)x]; k[1] = -(long long)((lb[(size_t)x] + 63) / 64) * (la[(size_t)x] + seg[(size_t)x]); k[2] = x;
        };
        for (int i = 0; i < n_launch; ++i) {
            const int32_t x = order[(size_t)i];
            if (x < 0 || x >= N || seen[(size_t)x]++ || la[(size_t)x] == 0 || lb[(size_t)x] == 0) EDIT_FAIL("plan: not the pairs that need the kernel, once each");
            if (i == 0) continue;
            long long kw[3], kx[3];
            key(order[(size_t)i - 1], kw); key(x, kx);
            if (!std::lexicographical_compare(kw, kw + 3, kx, kx + 3)) EDIT_FAIL("plan: the order");
        }
        // ---- the packing: the upload's parts, every wave's word
        EditLaunch L;
        edit_pack(ptr_or_null(seqs), lens.data(), M, L_stride, pa.data(), pb.data(), N, L);
        if (L.n_launch != n_launch || !std::equal(L.order.begin(), L.order.end(), order.begin())) EDIT_FAIL("pack: another plan");
        if (n_launch == 0) {
            if (!L.words.empty() || L.n_waves) EDIT_FAIL("pack: an upload for nothing");
        } else {
            const size_t pool = (size_t)M * (size_t)L_stride;
            if (L.words.size() != (size_t)M + pool + 2 * (size_t)n_launch + (size_t)L.n_waves) EDIT_FAIL("pack: the upload's size");
            if (!std::equal(lens.begin(), lens.end(), L.words.begin()) || !std::equal(seqs.begin(), seqs.end(), L.words.begin() + (ptrdiff_t)L.off_pool)) EDIT_FAIL("pack: lens or pool");
            int next = 0, col = 0;
            for (int w = 0; w < L.n_waves; ++w) {
                const uint32_t word = (uint32_t)L.words[L.off_waves + (size_t)w];
                const int first = (int)(word & 0xffffffu), s = 16 << ((word >> kEditSegShift) & 3), cnt = (int)(word >> kEditCountShift) & 7;
                if (first != next || cnt < 1 || cnt > 64 / s || first + cnt > n_launch) EDIT_FAIL("pack: a wave's pairs");
                for (int q = 0; q < cnt; ++q) {
                    const int32_t n = order[(size_t)(first + q)];
                    if (seg[(size_t)n] != s) EDIT_FAIL("pack: a wave of two segment widths");
                    if (L.words[L.off_a + (size_t)(first + q)] != pa[(size_t)n] || L.words[L.off_b + (size_t)(first + q)] != pb[(size_t)n]) EDIT_FAIL("pack: a pair's rows");
                    if (lb[(size_t)n] > 64) col = std::max(col, (int)la[(size_t)n] + 1);
                }
                // a wave is full unless the segment width ends behind it
                if (cnt < 64 / s && first + cnt < n_launch && seg[(size_t)order[(size_t)(first + cnt)]] == s) EDIT_FAIL("pack: a wave with room left");
                next = first + cnt;
            }
            if (next != n_launch || col != L.col_words) EDIT_FAIL("pack: the waves do not cover the launch, or the boundary column's size");
        }
        // ---- the unpacking: what the kernel would return (the recurrence, by the full table), against the counts' identities
        std::vector<uint32_t> packed((size_t)n_launch);
        for (int i = 0; i < n_launch; ++i) {
            const int32_t n = order[(size_t)i];
            packed[(size_t)i] = edit_table(seqs.data() + (size_t)pa[(size_t)n] * (size_t)L_stride, la[(size_t)n], seqs.data() + (size_t)pb[(size_t)n] * (size_t)L_stride, lb[(size_t)n]);
        }
        std::vector<int32_t> counts = exact(4 * (size_t)N + 1, -7);
        edit_unpack(L, packed.data(), lens.data(), pa.data(), pb.data(), N, counts.data());
        if (counts[4 * (size_t)N] != -7) EDIT_FAIL("unpack: a write past counts");
        for (int n = 0; n < N; ++n) {
            const int32_t* c = counts.data() + 4 * (size_t)n;
            const int a_ = la[(size_t)n], b_ = lb[(size_t)n];
            if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[3] < 0 || c[1] + c[2] + c[3] != c[0] || c[3] - c[2] != b_ - a_ || c[1] + c[2] > a_ || c[1] + c[3] > b_) EDIT_FAIL("unpack: the identities");
            if ((a_ == 0 || b_ == 0) && (c[0] != a_ + b_ || c[1] != 0 || c[2] != a_ || c[3] != b_)) EDIT_FAIL("unpack: a pair with an empty side");
            if (pa[(size_t)n] == pb[(size_t)n] && c[0] != 0) EDIT_FAIL("unpack: a sequence against itself");
            ++pairs_checked;
        }
    }
    std::printf("%d edit calls ok, %ld refused, %ld pairs checked\n", reps, refused, pairs_checked);
    return 0;
}

// ---- lmscore: the rules of include/dsmi.h written out plainly, beside lm_score_host.h -----------------------------------------
#define LMS_FAIL(what) do { std::fprintf(stderr, "lmscore: %s (repetition %d, line %d)\n", what, rep, __LINE__); return 12; } while (0)

static int run_lmscore(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long slots_checked = 0, refused = 0;
    for (int rep = 0; rep < reps; ++rep) {
        std::string err;
        const int32_t* none = nullptr;
        const int C = 5, blank = 0, space = rng() % 8 == 0 ? -2 : 4;
        // ---- refused on the numbers alone: no array is there to read
        {
            const int big = 1 + (int)(rng() % 1000);
            if (lm_score_check(false, none, none, 3, 4, C, blank, space, false, 0, err) != DSMI_ERR_INVALID || err.empty()) LMS_FAIL("no language model");
            if (lm_score_check(true, none, none, rng() % 2 ? 0 : -big, 4, C, blank, space, false, 0, err) != DSMI_ERR_INVALID) LMS_FAIL("M <= 0");
            if (lm_score_check(true, none, none, 3, -big, C, blank, space, false, 0, err) != DSMI_ERR_INVALID) LMS_FAIL("negative L_stride");
            if (lm_score_check(true, none, none, 3, DSMI_LM_SCORE_MAX_TOKENS + big, C, blank, space, true, 0, err) != DSMI_ERR_CAPACITY || err.find("DSMI_LM_SCORE_MAX_TOKENS") == std::string::npos) LMS_FAIL("L_stride above the limit");
            const int Ls = 1 + (int)(rng() % DSMI_LM_SCORE_MAX_TOKENS);
            if (lm_score_check(true, none, none, (int)(((int64_t)1 << 24) / Ls) + big, Ls, C, blank, space, false, 0, err) != DSMI_ERR_CAPACITY) LMS_FAIL("M * L_stride above 2^24");
            if (lm_score_check(true, none, none, INT32_MAX, DSMI_LM_SCORE_MAX_TOKENS, C, blank, space, true, -1, err) != DSMI_ERR_CAPACITY) LMS_FAIL("the largest numbers");
        }
        // ---- a random call: few labels, many spaces, rows around the pack size, garbage behind every length
        const int M = 1 + (int)(rng() % 40);
        const int edges[8] = {0, 1, 2, 7, 24, 60, 520, 1100};
        const int L_stride = edges[rng() % 8] + (int)(rng() % 3);
        std::vector<int32_t> seqs = exact((size_t)M * (size_t)L_stride), lens = exact((size_t)M);
        const unsigned space_in = 2 + rng() % 3;
        for (auto& v : seqs) v = rng() % space_in == 0 ? 4 : 1 + (int32_t)(rng() % 3);
        for (auto& v : lens) v = rng() % 5 == 0 ? 0 : (int32_t)(rng() % (unsigned)(L_stride + 1));
        // the words by the definition: one begins at every token that is no space and has a space, or nothing, in front of it
        std::vector<std::vector<std::pair<int, int>>> words((size_t)M);
        int most = 0;
        for (int m = 0; m < M; ++m) {
            const int32_t* row = seqs.data() + (size_t)m * (size_t)L_stride;
            for (int k = 0; k < lens[(size_t)m]; ++k) {
                if (row[k] == space) continue;
                if (k == 0 || row[k - 1] == space) words[(size_t)m].push_back({k, 0});
                ++words[(size_t)m].back().second;
            }
            most = std::max(most, (int)words[(size_t)m].size());
        }
        const int most_terms = most > 0 ? most + 1 : 2;
        const bool terms = rng() % 2 == 0;
        const int W_stride = terms ? most_terms - 1 + (int)(rng() % 3) : (rng() % 2 ? 0 : -5);
        const int spoil = (int)(rng() % 7);
        int want = terms && W_stride < most_terms ? DSMI_ERR_CAPACITY : DSMI_OK;
        if (spoil == 1) { lens[rng() % (unsigned)M] = rng() % 2 ? L_stride + 1 + (int32_t)(rng() % 3) : -1 - (int32_t)(rng() % 3); want = DSMI_ERR_INVALID; }
        if (spoil == 2) {
            std::vector<int> rows;
            for (int m = 0; m < M; ++m) if (lens[(size_t)m] > 0) rows.push_back(m);
            if (!rows.empty()) {
                const int m = rows[rng() % rows.size()];
                const int32_t bad[4] = {blank, C, -1, C + 7};
                seqs[(size_t)m * (size_t)L_stride + rng() % (unsigned)lens[(size_t)m]] = bad[rng() % 4];
                want = DSMI_ERR_INVALID;
            }
        }
        const int rc = lm_score_check(true, ptr_or_null(seqs), lens.data(), M, L_stride, C, blank, space, terms, W_stride, err);
        if (rc != want) LMS_FAIL("a call's verdict");
        if (rc != DSMI_OK) {
            if (err.empty()) LMS_FAIL("a refusal without a message");
            ++refused;
            continue;
        }
        // ---- the plan: the words by the definition; nothing written past a row's count, past the arrays, or on a refusal
        {
            const int Ws = most + (int)(rng() % 2);
            std::vector<int32_t> nw = exact((size_t)M + 1, -7), wf = exact((size_t)M * (size_t)Ws + 1, -7), wl = exact((size_t)M * (size_t)Ws + 1, -7);
            if (lm_score_plan(ptr_or_null(seqs), lens.data(), M, L_stride, space, nw.data(), wf.data(), wl.data(), Ws) != most) LMS_FAIL("plan: the largest n_words");
            if (nw[(size_t)M] != -7 || wf[(size_t)M * (size_t)Ws] != -7 || wl[(size_t)M * (size_t)Ws] != -7) LMS_FAIL("plan: a write past its arrays");
            for (int m = 0; m < M; ++m) {
                const auto& w = words[(size_t)m];
                if (nw[(size_t)m] != (int)w.size()) LMS_FAIL("plan: n_words");
                for (int k = 0; k < Ws; ++k) {
                    const int32_t f = wf[(size_t)m * (size_t)Ws + (size_t)k], l = wl[(size_t)m * (size_t)Ws + (size_t)k];
                    if (k < (int)w.size() ? (f != w[(size_t)k].first || l != w[(size_t)k].second) : (f != -7 || l != -7)) LMS_FAIL("plan: a word's span");
                }
            }
            if (most > 0) {
                std::vector<int32_t> nw2 = exact((size_t)M, -7), wf2 = exact((size_t)M * (size_t)(most - 1), -7), wl2 = wf2;
                if (lm_score_plan(ptr_or_null(seqs), lens.data(), M, L_stride, space, nw2.data(), wf2.data(), wl2.data(), most - 1) >= 0) LMS_FAIL("plan: a W_stride too small");
                for (int32_t v : nw2) if (v != -7) LMS_FAIL("plan: a refusal that wrote");
                for (int32_t v : wf2) if (v != -7) LMS_FAIL("plan: a refusal that wrote");
            }
        }
        // ---- the packing
        LmScoreLaunch L;
        lm_score_pack(ptr_or_null(seqs), lens.data(), M, L_stride, space, L);
        size_t n_tok = 0, n_slots = 0;
        for (int m = 0; m < M; ++m) {
            for (const auto& w : words[(size_t)m]) n_tok += (size_t)w.second;
            n_slots += words[(size_t)m].empty() ? 2 : words[(size_t)m].size() + 1;
        }
        if (L.n_tok != n_tok || L.n_slots != n_slots || (int)L.order.size() != M) LMS_FAIL("pack: the totals");
        if (L.words.size() != n_tok + 3 * n_slots + (size_t)M + 1 + (size_t)L.n_packs + 1) LMS_FAIL("pack: the upload's size");
        const int32_t* tok = L.words.data();
        const int32_t *s_first = tok + L.off_first, *s_len = tok + L.off_len, *s_sent = tok + L.off_sent, *sent_slot = tok + L.off_sent_slot, *pack_sent = tok + L.off_pack;
        std::vector<int> seen((size_t)M, 0);
        size_t slot = 0, at_tok = 0;
        for (int s = 0; s < M; ++s) {
            const int m = L.order[(size_t)s];
            if (m < 0 || m >= M || seen[(size_t)m]++) LMS_FAIL("pack: the order is no permutation");
            const auto& w = words[(size_t)m];
            if (L.n_words[(size_t)m] != (int)w.size()) LMS_FAIL("pack: n_words");
            if (s > 0) {
                const int p = L.order[(size_t)s - 1];
                if (words[(size_t)p].size() < w.size() || (words[(size_t)p].size() == w.size() && p > m)) LMS_FAIL("pack: not by n_words descending, then index");
            }
            if (sent_slot[s] != (int32_t)slot) LMS_FAIL("pack: a sentence's first slot");
            const int32_t* row = seqs.data() + (size_t)m * (size_t)L_stride;
            for (const auto& sp : w) {
                if (s_sent[slot] != s || s_len[slot] != sp.second || s_first[slot] != (int32_t)at_tok) LMS_FAIL("pack: a word's slot");
                if (!std::equal(row + sp.first, row + sp.first + sp.second, tok + at_tok)) LMS_FAIL("pack: a word's tokens");
                at_tok += (size_t)sp.second; ++slot;
            }
            if (w.empty()) { if (s_sent[slot] != s || s_len[slot] != kLmSlotBos) LMS_FAIL("pack: the <s> slot of an empty sentence"); ++slot; }
            if (s_sent[slot] != s || s_len[slot] != kLmSlotEos) LMS_FAIL("pack: the </s> slot");
            ++slot;
        }
        if (sent_slot[M] != (int32_t)n_slots || slot != n_slots || at_tok != n_tok) LMS_FAIL("pack: the slots do not cover the call");
        if (L.n_packs < 1 || pack_sent[0] != 0 || pack_sent[L.n_packs] != M) LMS_FAIL("pack: the packs do not cover the sentences");
        for (int p = 0; p < L.n_packs; ++p) {
            const int s0 = pack_sent[p], s1 = pack_sent[p + 1];
            if (s1 <= s0) LMS_FAIL("pack: an empty pack");
            const int n = sent_slot[s1] - sent_slot[s0];
            if (n > kLmScoreMaxSlots || (n > kLmScoreThreads && s1 - s0 != 1)) LMS_FAIL("pack: too many slots");
            // a pack is full: the next sentence would not have fitted
            if (s1 < M && n + (sent_slot[s1 + 1] - sent_slot[s1]) <= kLmScoreThreads) LMS_FAIL("pack: a pack with room left");
        }
        // ---- the unpacking: results coded by sentence and slot come back under the caller's indices, nothing else is written
        std::vector<double> d_ln((size_t)M), d_terms(n_slots);
        std::vector<int32_t> d_oov = exact((size_t)M);
        for (int s = 0; s < M; ++s) { d_ln[(size_t)s] = 1000.0 + L.order[(size_t)s]; d_oov[(size_t)s] = 7 * L.order[(size_t)s]; }
        for (size_t g = 0; g < n_slots; ++g) d_terms[g] = 0.5 + (double)g;
        const size_t Wt = terms ? (size_t)W_stride : 0;
        std::vector<double> ln((size_t)M + 1, -7.0), tm((size_t)M * Wt + 1, -7.0);
        std::vector<int32_t> nw = exact((size_t)M + 1, -7), no = exact((size_t)M + 1, -7), nt = exact((size_t)M + 1, -7);
        ln.shrink_to_fit(); tm.shrink_to_fit();
        lm_score_unpack(L, M, d_ln.data(), d_terms.data(), d_oov.data(), ln.data(), nw.data(), no.data(), nt.data(), terms ? tm.data() : nullptr, W_stride);
        if (ln[(size_t)M] != -7.0 || tm[(size_t)M * Wt] != -7.0 || nw[(size_t)M] != -7 || no[(size_t)M] != -7 || nt[(size_t)M] != -7) LMS_FAIL("unpack: a write past an array");
        for (int s = 0; s < M; ++s) {
            const int m = L.order[(size_t)s], n = (int)words[(size_t)m].size(), want_terms = n > 0 ? n + 1 : 2;
            if (ln[(size_t)m] != 1000.0 + m || no[(size_t)m] != 7 * m || nw[(size_t)m] != n || nt[(size_t)m] != want_terms) LMS_FAIL("unpack: a sentence's results");
            for (size_t t = 0; t < Wt; ++t) {
                const double v = tm[(size_t)m * Wt + t];
                if ((int)t < want_terms ? v != 0.5 + (double)(sent_slot[s] + (int)t) : v != -7.0) LMS_FAIL("unpack: a sentence's terms");
            }
            slots_checked += want_terms;
        }
    }
    std::printf("%d lmscore calls ok, %ld refused, %ld slots checked\n", reps, refused, slots_checked);
    return 0;
}

// ---- spotwatch: the rule of include/dsmi.h written out plainly, beside spot_pick.h ---------------------------------------------
#define SW_FAIL(what) do { std::fprintf(stderr, "spotwatch: %s (repetition %d, line %d)\n", what, rep, __LINE__); return 13; } while (0)

struct PlainEvent { int s, e; float v; int at; };
static std::vector<PlainEvent> plain_pick(const std::vector<float>& E, const std::vector<int32_t>& ST, float floor_, int settle, bool flush) {
    std::vector<PlainEvent> out;
    bool pending = false;
    float pv = 0; int ps = 0, pe = 0, last_end = -1;
    const int T = (int)E.size();
    for (int f = 0; f < T; ++f) {
        if (pending && (long long)f - pe >= settle) { out.push_back({ps, pe + 1, pv, f}); last_end = pe; pending = false; }
        if (!(E[(size_t)f] > -INFINITY) || !(E[(size_t)f] >= floor_ * (float)(f - ST[(size_t)f] + 1)) || !(ST[(size_t)f] > last_end)) continue;
        if (pending && ST[(size_t)f] <= pe) { if (E[(size_t)f] > pv) { pv = E[(size_t)f]; ps = ST[(size_t)f]; pe = f; } continue; }
        if (pending) { out.push_back({ps, pe + 1, pv, f}); last_end = pe; }
        pending = true; pv = E[(size_t)f]; ps = ST[(size_t)f]; pe = f;
    }
    if (flush && pending) out.push_back({ps, pe + 1, pv, T});
    return out;
}

static int run_spotwatch(int argc, char** argv) {
    std::mt19937 rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
    const int reps = argc > 3 ? std::atoi(argv[3]) : 200;
    long events = 0, refused = 0;
    for (int rep = 0; rep < reps; ++rep) {
        std::string err;
        // ---- the rule: random tracks with few distinct scores (ties), cut into random chunks with empty ones, exactly sized arrays
        {
            const int T = (int)(rng() % 120), settle = rng() % 4 ? 1 + (int)(rng() % 30) : INT32_MAX;
            const float floors[4] = {-INFINITY, -1.f, -0.5f, -2.f};
            const float floor_ = floors[rng() % 4];
            std::vector<float> E((size_t)T); std::vector<int32_t> ST((size_t)T);
            for (int f = 0; f < T; ++f) {
                const bool dead = rng() % 4 == 0;
                ST[(size_t)f] = dead ? -1 : f - (int)(rng() % (unsigned)(std::min(f, 6) + 1));
                E[(size_t)f] = dead ? -INFINITY : -(float)(1 + rng() % 5);
            }
            const bool flush = rng() % 4 != 0;
            const std::vector<PlainEvent> want = plain_pick(E, ST, floor_, settle, flush);
            SpotPick p = spot_pick_fresh();
            std::vector<PlainEvent> got;
            for (int at = 0, last = 0; !last;) {
                const int c = std::min(T - at, (int)(rng() % 3 ? rng() % 34 : 0));
                last = at + c == T && rng() % 2;
                const int M = (int)(rng() % 6);
                std::vector<float> e(E.begin() + at, E.begin() + at + c); e.shrink_to_fit();
                std::vector<int32_t> st(ST.begin() + at, ST.begin() + at + c); st.shrink_to_fit();
                std::vector<int32_t> hits = exact(2 * (size_t)M + 1, -7), fired = exact((size_t)M + 1, -7);
                std::vector<float> sc((size_t)M + 1, -7.f); sc.shrink_to_fit();
                // the events of this chunk, all of them, from a copy of the state; then the call under test with M slots
                SpotPick q = p;
                std::vector<int32_t> ah = exact(2 * (size_t)c + 2), af = exact((size_t)c + 1);
                std::vector<float> as((size_t)c + 1);
                const int all = spot_pick_chunk(q, e.data(), st.data(), c, at, last && flush, floor_, settle, c + 1, ah.data(), as.data(), af.data());
                const int n = spot_pick_chunk(p, e.data(), st.data(), c, at, last && flush, floor_, settle, M, hits.data(), sc.data(), fired.data());
                if (n != all || n > c + 1 || std::memcmp(&p, &q, sizeof p)) SW_FAIL("the count or the state depends on max_events");
                if (hits[2 * (size_t)M] != -7 || fired[(size_t)M] != -7 || sc[(size_t)M] != -7.f) SW_FAIL("a write past max_events");
                for (int i = 0; i < M; ++i) {
                    if (i < n ? hits[2 * (size_t)i] != ah[2 * (size_t)i] || hits[2 * (size_t)i + 1] != ah[2 * (size_t)i + 1] || sc[(size_t)i] != as[(size_t)i] || fired[(size_t)i] != af[(size_t)i]
                              : hits[2 * (size_t)i] != -7 || fired[(size_t)i] != -7) SW_FAIL("the stored events are not the first");
                }
                for (int i = 0; i < all; ++i) got.push_back({ah[2 * (size_t)i], ah[2 * (size_t)i + 1], as[(size_t)i], af[(size_t)i]});
                at += c;
            }
            if (got.size() != want.size()) SW_FAIL("the number of events");
            for (size_t i = 0; i < want.size(); ++i) {
                if (got[i].s != want[i].s || got[i].e != want[i].e || got[i].v != want[i].v || got[i].at != want[i].at) SW_FAIL("an event differs from the rule");
                if (got[i].s >= got[i].e || (i && (got[i - 1].e > got[i].s || got[i - 1].at > got[i].at))) SW_FAIL("events overlap or are out of order");
            }
            events += (long)want.size();
        }
        // ---- the watch's check: a good list, then one fault
        {
            const int C = 2 + (int)(rng() % 127), blank = (int)(rng() % (unsigned)C);
            const int K = 1 + (int)(rng() % 20), L_stride = 1 + (int)(rng() % 12);
            std::vector<int32_t> lens = exact((size_t)K), ph = exact((size_t)K * L_stride);
            for (int k = 0; k < K; ++k) {
                lens[(size_t)k] = 1 + (int32_t)(rng() % (unsigned)L_stride);
                random_row(rng, ph.data() + (size_t)k * L_stride, lens[(size_t)k], C, blank, false);
            }
            if (spot_watch_check(ph.data(), lens.data(), K, L_stride, -1.f, 1 + (int)(rng() % 50), C, blank, err) != DSMI_OK) SW_FAIL("watch: a good list refused");
            const int32_t* none = nullptr;
            const int big = 1 + (int)(rng() % 1000);
            if (spot_watch_check(none, none, rng() % 2 ? 0 : -big, 3, -1.f, 5, C, blank, err) != DSMI_ERR_INVALID) SW_FAIL("watch: K <= 0");
            if (spot_watch_check(none, none, K, 3, -1.f, rng() % 2 ? 0 : -big, C, blank, err) != DSMI_ERR_INVALID) SW_FAIL("watch: settle_frames < 1");
            if (spot_watch_check(none, none, K, 3, std::nanf(""), 5, C, blank, err) != DSMI_ERR_INVALID) SW_FAIL("watch: NaN floor");
            if (spot_watch_check(none, none, K, DSMI_SPOT_MAX_TOKENS + big, -1.f, 5, C, blank, err) != DSMI_ERR_CAPACITY) SW_FAIL("watch: L_stride over the limit");
            if (spot_watch_check(none, none, DSMI_SPOT_MAX_PHRASES + big, 3, -1.f, 5, C, blank, err) != DSMI_ERR_CAPACITY) SW_FAIL("watch: K over the limit");
            const int k = (int)(rng() % (unsigned)K);
            if (rng() % 2) lens[(size_t)k] = rng() % 2 ? 0 : L_stride + 1;
            else random_row(rng, ph.data() + (size_t)k * L_stride, lens[(size_t)k], C, blank, true);
            if (spot_watch_check(ph.data(), lens.data(), K, L_stride, -1.f, 5, C, blank, err) != DSMI_ERR_INVALID ||
                err.find("spot watch: phrase " + std::to_string(k) + ": ") != 0) SW_FAIL("watch: a spoilt phrase passed or another one was named");
            refused += 6;
        }
        // ---- one advance: a good call, then one fault, the stream named
        {
            const int n = 1 + (int)(rng() % 12), K = 1 + (int)(rng() % 9), M = 1 + (int)(rng() % DSMI_SPOT_MAX_HITS), F = (int)(rng() % 40);
            std::vector<char> objects((size_t)n + 2), watches(2);
            std::vector<const void*> handles((size_t)n), watch_of((size_t)n);
            std::vector<int64_t> consumed((size_t)n);
            std::vector<int32_t> frames = exact((size_t)n);
            std::vector<const float*> probs((size_t)n);
            static const float some = 0.f;
            for (int i = 0; i < n; ++i) {
                handles[(size_t)i] = &objects[(size_t)i]; watch_of[(size_t)i] = &watches[0];
                consumed[(size_t)i] = rng() % 3 ? (int64_t)(rng() % 1000) : (int64_t)INT32_MAX - F - (int64_t)(rng() % 3);
                frames[(size_t)i] = (int32_t)(rng() % (unsigned)(F + 1));
                probs[(size_t)i] = frames[(size_t)i] ? &some : nullptr;
            }
            handles.shrink_to_fit(); watch_of.shrink_to_fit(); consumed.shrink_to_fit(); probs.shrink_to_fit();
            auto check = [&](bool tracks) { return spot_stream_check(handles.data(), watch_of.data(), consumed.data(), n, probs.data(), frames.data(), K, M, tracks, F, err); };
            if (check(true) != DSMI_OK || check(false) != DSMI_OK) SW_FAIL("advance: a good call refused");
            const void* const* no_h = nullptr; const int64_t* no_c = nullptr; const float* const* no_p = nullptr; const int32_t* no_f = nullptr;
            const int big = 1 + (int)(rng() % 1000);
            if (spot_stream_check(no_h, no_h, no_c, rng() % 2 ? 0 : DSMI_SPOT_STREAM_MANY_MAX + big, no_p, no_f, K, M, true, F, err) != DSMI_ERR_INVALID) SW_FAIL("advance: n out of range");
            if (spot_stream_check(no_h, no_h, no_c, n, no_p, no_f, K, rng() % 2 ? 0 : DSMI_SPOT_MAX_HITS + big, true, F, err) != DSMI_ERR_INVALID) SW_FAIL("advance: max_events out of range");
            if (spot_stream_check(no_h, no_h, no_c, n, no_p, no_f, K, M, true, -big, err) != DSMI_ERR_INVALID) SW_FAIL("advance: negative F_stride");
            if (spot_stream_check(no_h, no_h, no_c, DSMI_SPOT_STREAM_MANY_MAX, no_p, no_f, DSMI_SPOT_MAX_PHRASES, DSMI_SPOT_MAX_HITS, false, F, err) != DSMI_ERR_CAPACITY) SW_FAIL("advance: the event cap");
            if (spot_stream_check(no_h, no_h, no_c, n, no_p, no_f, K, M, true, (1 << 27) / (n * K) + big, err) != DSMI_ERR_CAPACITY) SW_FAIL("advance: the track cap");
            const int i = (int)(rng() % (unsigned)n);
            const std::string named = "spot stream " + std::to_string(i) + ": ";
            int want = DSMI_ERR_INVALID;
            bool tracks = true;
            switch (rng() % 6) {
                case 0: if (n < 2) continue; handles[(size_t)i] = handles[(size_t)(i ? i - 1 : n - 1)]; if (!i) { std::swap(handles[0], handles[(size_t)n - 1]); } break;
                case 1: if (i == 0) continue; watch_of[(size_t)i] = &watches[1]; break;
                case 2: frames[(size_t)i] = -1 - (int32_t)(rng() % 5); break;
                case 3: frames[(size_t)i] = 1 + (int32_t)(rng() % (unsigned)(F + 1)); probs[(size_t)i] = nullptr; tracks = false; consumed[(size_t)i] = 0; break;
                case 4: frames[(size_t)i] = F + 1; probs[(size_t)i] = &some; consumed[(size_t)i] = 0; break;
                default: consumed[(size_t)i] = (int64_t)INT32_MAX - frames[(size_t)i] + 1; want = DSMI_ERR_CAPACITY; break;
            }
            const int rc = check(tracks);
            if (rc != want) SW_FAIL("advance: a fault passed or got the wrong code");
            if (err.find(named) != 0 && !(n >= 2 && err.find("the same handle appears twice") != std::string::npos)) SW_FAIL("advance: another stream was named");
            refused += 6;
        }
    }
    std::printf("%d spotwatch calls ok, %ld events checked, %ld refusals\n", reps, events, refused);
    return 0;
}

// ---- streampass: one session's schedule per line, from a fresh handle, through stream_pass_plan / stream_pass_commit -----------
// Per pass "code padl padr ctxl tin0 tin1 to0 to1 buffering ncat nout keep : has_left has_hidden la_init la_rows pbase0 pbase1" (the flags
// and two layers' parities after the pass), a refused pass "code why=SENTENCE : ..." with nothing committed; passes joined by " | ".
static int run_streampass(int argc, char** argv) {
    std::FILE* f = argc > 2 ? std::fopen(argv[2], "r") : nullptr;
    if (!f) return 2;
    int rc = 0;
    char line[4096];
    while (!rc && std::fgets(line, sizeof line, f)) {
        int context, cap, have_probs, used = 0;
        if (std::sscanf(line, "%d %d %d%n", &context, &cap, &have_probs, &used) != 3 || context < 1) { rc = 2; break; }
        StreamFlags flags;
        int pbase[2] = {0, 0};
        std::string out;
        const char* at = line + used;
        int T, first, last;
        while (std::sscanf(at, " | %d %d %d%n", &T, &first, &last, &used) == 3) {
            at += used;
            if (T < 1) { rc = 2; break; }      // both entry points refuse it before they plan
            StreamPass p, untouched;
            std::memset(&p, 0x5a, sizeof p);
            std::memset(&untouched, 0x5a, sizeof untouched);
            const StreamFlags before = flags;
            const char* why = nullptr;
            const int code = stream_pass_plan(flags, T, first != 0, last != 0, context, have_probs != 0, cap, &p, &why);
            char buf[400];
            if (code) {
                if (!why || std::memcmp(&p, &untouched, sizeof p) || flags.has_left != before.has_left || flags.has_hidden != before.has_hidden ||
                    flags.la_init != before.la_init || flags.la_rows != before.la_rows) { std::fprintf(stderr, "streampass: a refusal wrote something\n"); rc = 12; break; }
                std::snprintf(buf, sizeof buf, "%d why=%s", code, why);
            } else {
                if (why) { std::fprintf(stderr, "streampass: a reason without a refusal\n"); rc = 12; break; }
                std::snprintf(buf, sizeof buf, "0 %d %d %d %d %d %d %d %d %d %d %d", p.padl, p.padr, p.ctxl, p.tin[0], p.tin[1], p.to[0], p.to[1],
                              (int)p.buffering, p.ncat, p.nout, p.keep);
                stream_pass_commit(flags, pbase, 2, p, last != 0);
            }
            out += out.empty() ? "" : " | ";
            out += buf;
            std::snprintf(buf, sizeof buf, " : %d %d %d %d %d %d", (int)flags.has_left, (int)flags.has_hidden, (int)flags.la_init, flags.la_rows, pbase[0], pbase[1]);
            out += buf;
        }
        std::printf("%s\n", out.c_str());
    }
    std::fclose(f);
    return rc;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "lm")) return run_lm(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return run_plan(argc, argv);
    if (argc >= 3 && !std::strcmp(argv[1], "rnnplan")) return run_rnnplan(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "rnnforms")) return run_rnnforms();
    if (argc >= 2 && !std::strcmp(argv[1], "gate")) return run_gate(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "scoreplan")) return run_scoreplan(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "ctccheck")) return run_ctccheck(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "occcheck")) return run_occcheck(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "grammarcheck")) return run_grammarcheck(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "grammarpostcheck")) return run_grammarpostcheck(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "grammarstreamcheck")) return run_grammarstreamcheck(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "alignlong")) return run_alignlong(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "editcheck")) return run_editcheck(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "lmscore")) return run_lmscore(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "spotwatch")) return run_spotwatch(argc, argv);
    if (argc >= 3 && !std::strcmp(argv[1], "streampass")) return run_streampass(argc, argv);
    std::fprintf(stderr, "usage: host_fuzz lm FILE... | host_fuzz plan [SEED [N]] | host_fuzz rnnplan FILE|grid | host_fuzz rnnforms | host_fuzz gate [SEED [N]] | host_fuzz scoreplan [SEED [N]] | host_fuzz ctccheck [SEED [N]] | host_fuzz occcheck [SEED [N]] | host_fuzz grammarcheck [SEED [N]] | host_fuzz grammarpostcheck [SEED [N]] | host_fuzz grammarstreamcheck [SEED [N]] | host_fuzz alignlong [SEED [N]] | host_fuzz editcheck [SEED [N]] | host_fuzz lmscore [SEED [N]] | host_fuzz spotwatch [SEED [N]] | host_fuzz streampass FILE\n");
    return 2;
}
