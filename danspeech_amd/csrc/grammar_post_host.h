// The host half of the CTC grammar posterior (dsmi_grammar_posterior, dsmi_grammar_posterior_plan: ctc_tools.hip; the kernels:
// grammar_post.hip): the geometry of a call, its refusals beyond grammar_check's (grammar_host.h), and what the host builds once
// per call for the kernels -- the transposed arcs (each node's successors, for the backward pass), each graph's start nodes and
// its nodes bucketed by label (for the output kernel).  No HIP: a plain C++ compiler takes it, and tools/asan/host_fuzz.cpp
// (grammarpostcheck) runs it under ASan + UBSan on exactly sized arrays.
#pragma once
#include "grammar_host.h"

namespace dsmi {

constexpr int kGrammarPostThreads = 256;
// a node with more arcs than this in a pass's lists (predecessors forward, successors backward) is reduced by a wave, not by the
// thread that owns it; there are at most DSMI_GRAMMAR_MAX_ARCS / (kGrammarPostHeavy + 1) of them
constexpr int kGrammarPostHeavy = 24;
constexpr int kGrammarPostMaxHeavy = DSMI_GRAMMAR_MAX_ARCS / (kGrammarPostHeavy + 1) + 1;
// the two stored trellises of a call, kept on the handle: per clip and frame a (tok, blk) pair of doubles per node of the node
// stride, forward and backward, and the two doubles of lead.  32 clips of 501 frames fit at DSMI_GRAMMAR_MAX_NODES (1002 MiB).
constexpr uint64_t kGrammarPostCap = (uint64_t)1 << 30;

// The geometry of a call whose largest graph has n_nodes nodes and n_arcs arcs.
struct GrammarPostPlan {
    int64_t node_stride;      // nodes per trellis row and per LDS row: n_nodes rounded up to a multiple of 4, at least 4
    int64_t lds_bytes;        // a trellis workgroup's LDS: the dynamic carve and the feeder's float64 image
    int64_t ws_bytes;         // B * T_out * (32 * node_stride + 16): the stored trellises
};

// the dynamic carve: tok / blk pairs of doubles [2][stride] (16 bytes each), node words and weights [stride] (4 bytes each), arc
// offsets [stride + 4], the start nodes [stride] and the arcs (2 bytes each)
inline int64_t grammar_post_carve_bytes(int64_t stride, int n_arcs) {
    return 32 * stride + 8 * stride + 2 * (stride + 4) + 2 * stride + 2 * grammar_arc_words(n_arcs);
}
inline int64_t grammar_post_lds_bytes(int64_t stride, int n_arcs) {
    return grammar_post_carve_bytes(stride, n_arcs) + 2 * (int64_t)sizeof(double) * kCtcChunk * kCtcMaxLabels +
           (int64_t)sizeof(double) * kGrammarPostThreads + 2 * (int64_t)kGrammarPostMaxHeavy + 8;      // (and the end's reduction, a double per thread; the wave-reduced nodes and their count)
}
static_assert(32 * DSMI_GRAMMAR_MAX_NODES + 8 * DSMI_GRAMMAR_MAX_NODES + 2 * (DSMI_GRAMMAR_MAX_NODES + 4) + 2 * DSMI_GRAMMAR_MAX_NODES +
              2 * DSMI_GRAMMAR_MAX_ARCS + 2 * 8 * kCtcChunk * kCtcMaxLabels + 8 * kGrammarPostThreads + 2 * kGrammarPostMaxHeavy + 8 <= 160 * 1024,
              "the float64 rows of the largest graph fit a workgroup's LDS");

inline int grammar_post_plan(int B, int To, int n_nodes, int n_arcs, GrammarPostPlan* plan, std::string& err) {
    if (B <= 0 || To <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar posterior: B and T_out must be positive");
    const int64_t stride = std::max<int64_t>(4, ((int64_t)std::max(n_nodes, 0) + 3) & ~(int64_t)3);
    const uint64_t BT = (uint64_t)B * (uint64_t)To;
    // (the cap first: it is far below dsmi_grammar's on its backpointers, which grammar_plan would name otherwise)
    if (n_nodes <= DSMI_GRAMMAR_MAX_NODES && (BT > kGrammarPostCap || BT * (32 * (uint64_t)stride + 16) > kGrammarPostCap))
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar posterior: the stored trellises, B * T_out * (32 * node stride + 16) bytes, exceed 2^30 (B * T_out = " +
                                                      std::to_string(BT) + ", node stride " + std::to_string(stride) + ")");
    GrammarPlan gp;
    if (int rc = grammar_plan(1, 1, n_nodes, n_arcs, &gp, err)) return rc;      // the node and arc limits, by dsmi_grammar's messages
    plan->node_stride = stride;
    plan->lds_bytes = grammar_post_lds_bytes(stride, n_arcs);
    plan->ws_bytes = (int64_t)(BT * (32 * (uint64_t)stride + 16));
    return DSMI_OK;
}

// What the kernels need beside the pool, for a pool that grammar_check has passed.
struct GrammarPostPack {
    std::vector<int32_t> words;          // [nodes] label | kGrammarStart | kGrammarFinal
    std::vector<uint16_t> arc16;         // [arcs] predecessor | kGrammarArcTok where the two labels differ, at arc_off (dsmi_grammar's)
    std::vector<int32_t> succ_off;       // [nodes + 1] where each node's successors lie in succ16: the transposed CSR
    std::vector<uint16_t> succ16;        // [arcs] successor | kGrammarArcTok where the two labels differ; a node's successors
                                         // ascending, an arc listed twice twice
    std::vector<int32_t> start_off;      // [K + 1] where each graph's start nodes lie in start16
    std::vector<uint16_t> start16;       // the start nodes of each graph, ascending, graph-local
    std::vector<int32_t> bucket_off;     // [K][C + 1] where the nodes of label c lie in bucket_nodes, from the graph's first node
    std::vector<int32_t> bucket_nodes;   // [nodes] each graph's nodes sorted by label, ascending within a label, graph-local
    int max_fan_in = 0;                  // the most predecessors of one node
};

inline void grammar_post_pack(int K, const int32_t* node_off, const int32_t* labels, const int32_t* flags, const int32_t* arc_off,
                              const int32_t* arc_pred, int C, GrammarPostPack& out) {
    const size_t total = (size_t)node_off[K], n_arcs = (size_t)arc_off[total];
    out.words.assign(total, 0);
    out.arc16.assign(n_arcs, 0);
    out.succ_off.assign(total + 1, 0);
    out.succ16.assign(n_arcs, 0);
    out.start_off.assign((size_t)K + 1, 0);
    out.start16.clear();
    out.bucket_off.assign((size_t)K * ((size_t)C + 1), 0);
    out.bucket_nodes.assign(total, 0);
    out.max_fan_in = 0;
    std::vector<int32_t> fill;
    for (int g = 0; g < K; ++g) {
        const int n0 = node_off[g], N = node_off[g + 1] - n0;
        int32_t* boff = out.bucket_off.data() + (size_t)g * ((size_t)C + 1);
        // ---- counts: a node's successors, a label's nodes
        for (int n = 0; n < N; ++n) {
            const int i = n0 + n;
            out.words[i] = labels[i] | ((flags[i] & DSMI_GRAMMAR_START) ? kGrammarStart : 0) | ((flags[i] & DSMI_GRAMMAR_FINAL) ? kGrammarFinal : 0);
            if (flags[i] & DSMI_GRAMMAR_START) out.start16.push_back((uint16_t)n);
            out.max_fan_in = std::max(out.max_fan_in, arc_off[i + 1] - arc_off[i]);
            for (int j = arc_off[i]; j < arc_off[i + 1]; ++j) ++out.succ_off[(size_t)n0 + arc_pred[j] + 1];
            ++boff[labels[i] + 1];
        }
        out.start_off[(size_t)g + 1] = (int32_t)out.start16.size();
        for (int c = 0; c < C; ++c) boff[c + 1] += boff[c];
    }
    for (size_t i = 0; i < total; ++i) out.succ_off[i + 1] += out.succ_off[i];
    // ---- the lists, the nodes ascending: so are a node's successors and a label's nodes
    fill.assign(out.succ_off.begin(), out.succ_off.end() - 1);
    for (int g = 0; g < K; ++g) {
        const int n0 = node_off[g], N = node_off[g + 1] - n0;
        const int32_t* boff = out.bucket_off.data() + (size_t)g * ((size_t)C + 1);
        std::vector<int32_t> bfill(boff, boff + C);
        for (int n = 0; n < N; ++n) {
            const int i = n0 + n;
            for (int j = arc_off[i]; j < arc_off[i + 1]; ++j) {
                const int p = arc_pred[j];
                const int tok = labels[n0 + p] != labels[i] ? kGrammarArcTok : 0;
                out.arc16[j] = (uint16_t)(p | tok);
                out.succ16[(size_t)fill[(size_t)n0 + p]++] = (uint16_t)(n | tok);
            }
            out.bucket_nodes[(size_t)n0 + bfill[labels[i]]++] = n;
        }
    }
}

// Everything dsmi_grammar_posterior refuses, in its order: what the numbers alone refuse (before any array is read), the pool
// and the clips by grammar_check, the stored trellises of the pool's largest graph, then N_stride.
inline int grammar_post_check(const int32_t* sizes, int B, int To, int K, const int32_t* node_off, const int32_t* labels, const float* weights,
                              const int32_t* flags, const int32_t* arc_off, const int32_t* arc_pred, const int32_t* empty_ok,
                              const int32_t* clip_graph, int C, int blank, bool want_visits, int N_stride, std::vector<int32_t>& sz,
                              std::vector<int32_t>& cg, int* n_nodes, int* n_arcs, GrammarPostPlan* plan, std::string& err) {
    if (int rc = grammar_post_plan(B, To, 0, 0, plan, err)) return rc;
    if (int rc = grammar_check(sizes, B, To, K, node_off, labels, weights, flags, arc_off, arc_pred, empty_ok, clip_graph, C, blank, sz, cg,
                               n_nodes, n_arcs, err)) return rc;
    if (int rc = grammar_post_plan(B, To, *n_nodes, *n_arcs, plan, err)) return rc;
    if (want_visits && N_stride < *n_nodes)
        return ctc_refuse(err, DSMI_ERR_INVALID, "grammar posterior: N_stride " + std::to_string(N_stride) + " is below the pool's largest graph (" +
                                                     std::to_string(*n_nodes) + " nodes)");
    return DSMI_OK;
}

}  // namespace dsmi
