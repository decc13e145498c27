// The host half of CTC grammar decoding (dsmi_grammar, dsmi_grammar_plan: ctc_tools.hip; the kernel: grammar.hip): the limits, the
// geometry of a call and the check of everything a caller hands in.  No HIP: a plain C++ compiler takes it, and
// tools/asan/host_fuzz.cpp (grammarcheck) runs it under ASan + UBSan on exactly sized arrays.  A check returns DSMI_OK or a
// DSMI_ERR_* code with the message in `err`; what the numbers alone refuse is refused before any array is read.
#pragma once
#include "ctc_host.h"

namespace dsmi {

constexpr int kGrammarThreads = 256;
// a node's word in LDS: its label in the low byte, then
constexpr int kGrammarStart = 1 << 8;
constexpr int kGrammarFinal = 1 << 9;
// an arc in LDS, 16 bits: the predecessor's graph-local id, and whether its token state may enter (the labels differ)
constexpr int kGrammarArcNode = 0x7ff;
constexpr int kGrammarArcTok = 0x8000;
static_assert(DSMI_GRAMMAR_MAX_NODES - 1 <= kGrammarArcNode, "an arc keeps a node id in 11 bits");
static_assert(DSMI_GRAMMAR_MAX_ARCS <= 0xffff, "a node's arc offset is a 16-bit word");
// a backpointer, 16 bits per (frame, node): where tok(n) came from -- the kind in bits 11..12, the predecessor's id below -- and in
// bit 15 whether blk(n) came from tok(n) (0: it stayed)
constexpr int kGrammarStay = 0, kGrammarLead = 1, kGrammarFromBlk = 2, kGrammarFromTok = 3;
constexpr int kGrammarKindShift = 11;
constexpr int kGrammarBlkFromTok = 0x8000;

constexpr uint64_t kGrammarPoolCap = (uint64_t)1 << 24;      // nodes, and arcs, of all graphs of a call: the upload
constexpr uint64_t kGrammarBpCap = (uint64_t)1 << 31;        // bytes of backpointers of a call, kept on the handle

// The geometry of a call whose largest graph has n_nodes nodes and n_arcs arcs.
struct GrammarPlan {
    int64_t node_stride;      // nodes per backpointer row and per LDS row: n_nodes rounded up to a multiple of 4, at least 4
    int64_t lds_bytes;        // the kernel's LDS: the dynamic carve and the feeder's image
    int64_t bp_bytes;         // B * T_out * node_stride 16-bit backpointers
};

inline int64_t grammar_arc_words(int n_arcs) { return ((int64_t)n_arcs + 3) & ~(int64_t)3; }
// the dynamic carve: tok / blk pairs [2][stride] (8 bytes each), node words and weights [stride] (4 bytes each), arc offsets
// [stride + 4] and arcs (2 bytes each)
inline int64_t grammar_carve_bytes(int64_t stride, int n_arcs) { return 16 * stride + 8 * stride + 2 * (stride + 4) + 2 * grammar_arc_words(n_arcs); }

inline int grammar_plan(int B, int To, int n_nodes, int n_arcs, GrammarPlan* plan, std::string& err) {
    if (B <= 0 || To <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar: B and T_out must be positive");
    if (n_nodes < 0 || n_arcs < 0) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar: negative node or arc count");
    if (n_nodes > DSMI_GRAMMAR_MAX_NODES)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar: " + std::to_string(n_nodes) + " nodes exceed DSMI_GRAMMAR_MAX_NODES (" + std::to_string(DSMI_GRAMMAR_MAX_NODES) + ")");
    if (n_arcs > DSMI_GRAMMAR_MAX_ARCS)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar: " + std::to_string(n_arcs) + " arcs exceed DSMI_GRAMMAR_MAX_ARCS (" + std::to_string(DSMI_GRAMMAR_MAX_ARCS) + ")");
    const int64_t stride = std::max<int64_t>(4, ((int64_t)n_nodes + 3) & ~(int64_t)3);
    const uint64_t bp = 2 * (uint64_t)B * (uint64_t)To * (uint64_t)stride;
    if ((uint64_t)B * (uint64_t)To > kGrammarBpCap || bp > kGrammarBpCap)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar: the backpointers, 2 * B * T_out * node stride bytes, exceed 2^31 (" + std::to_string(bp) + ")");
    plan->node_stride = stride;
    plan->lds_bytes = grammar_carve_bytes(stride, n_arcs) + 2 * (int64_t)sizeof(float) * kCtcChunk * kCtcMaxLabels;
    plan->bp_bytes = (int64_t)bp;
    return DSMI_OK;
}

// The pool of a call, as dsmi_grammar_pool holds it (include/dsmi.h), and the call's clips.  sz [B] = the frames of each clip, cg [B]
// = its graph, *n_nodes / *n_arcs = the most nodes / arcs of one graph of the pool.
inline int grammar_check(const int32_t* sizes, int B, int To, int K, const int32_t* node_off, const int32_t* labels, const float* weights,
                         const int32_t* flags, const int32_t* arc_off, const int32_t* arc_pred, const int32_t* empty_ok,
                         const int32_t* clip_graph, int C, int blank, std::vector<int32_t>& sz, std::vector<int32_t>& cg, int* n_nodes,
                         int* n_arcs, std::string& err) {
    if (B <= 0 || To <= 0 || K <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar: B, T_out and K must be positive");
    if ((uint64_t)K > kGrammarPoolCap) return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar: K exceeds 2^24");
    auto at = [](int g) { return "grammar: graph " + std::to_string(g) + ": "; };      // (only a refusal pays for text)
    // ---- the offsets: nodes first, since they say how long arc_off is
    if (node_off[0] != 0) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar: node_off[0] must be 0");
    *n_nodes = 0;
    for (int g = 0; g < K; ++g) {
        if (node_off[g + 1] < node_off[g]) return ctc_refuse(err, DSMI_ERR_INVALID, at(g) + "node offsets not ascending");
        const int64_t n = (int64_t)node_off[g + 1] - node_off[g];
        if (n > DSMI_GRAMMAR_MAX_NODES)
            return ctc_refuse(err, DSMI_ERR_CAPACITY, at(g) + std::to_string(n) + " nodes exceed DSMI_GRAMMAR_MAX_NODES (" + std::to_string(DSMI_GRAMMAR_MAX_NODES) + ")");
        *n_nodes = std::max(*n_nodes, (int)n);
    }
    const int total = node_off[K];
    if ((uint64_t)total > kGrammarPoolCap) return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar: the pool's nodes exceed 2^24");
    if (arc_off[0] != 0) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar: arc_off[0] must be 0");
    *n_arcs = 0;
    for (int g = 0; g < K; ++g) {
        for (int i = node_off[g]; i < node_off[g + 1]; ++i)
            if (arc_off[i + 1] < arc_off[i]) return ctc_refuse(err, DSMI_ERR_INVALID, at(g) + "arc offsets not ascending at node " + std::to_string(i - node_off[g]));
        const int64_t n = (int64_t)arc_off[node_off[g + 1]] - arc_off[node_off[g]];
        if (n > DSMI_GRAMMAR_MAX_ARCS)
            return ctc_refuse(err, DSMI_ERR_CAPACITY, at(g) + std::to_string(n) + " arcs exceed DSMI_GRAMMAR_MAX_ARCS (" + std::to_string(DSMI_GRAMMAR_MAX_ARCS) + ")");
        *n_arcs = std::max(*n_arcs, (int)n);
    }
    if ((uint64_t)arc_off[total] > kGrammarPoolCap) return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar: the pool's arcs exceed 2^24");
    GrammarPlan plan;
    if (int rc = grammar_plan(B, To, *n_nodes, *n_arcs, &plan, err)) return rc;
    // ---- the clips
    sz.assign((size_t)B, 0); cg.assign((size_t)B, 0);
    constexpr CtcRows kGrammarRows{"grammar", "clip", "", "", "", 0, 0};
    if (int rc = ctc_check_sizes(kGrammarRows, sizes, B, To, sz.data(), err)) return rc;
    for (int b = 0; b < B; ++b) {
        cg[b] = clip_graph ? clip_graph[b] : 0;
        if (cg[b] < 0 || cg[b] >= K) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar: clip " + std::to_string(b) + ": graph outside 0 .. K-1");
    }
    // ---- the graphs
    for (int g = 0; g < K; ++g) {
        const int n0 = node_off[g], N = node_off[g + 1] - n0;
        bool any_start = false, any_final = false;
        for (int n = 0; n < N; ++n) {
            const int i = n0 + n;
            if (labels[i] < 0 || labels[i] >= C || labels[i] == blank)
                return ctc_refuse(err, DSMI_ERR_INVALID, at(g) + "node " + std::to_string(n) + ": label " + std::to_string(labels[i]) + " is the blank or not a label");
            if (weights && !std::isfinite(weights[i])) return ctc_refuse(err, DSMI_ERR_INVALID, at(g) + "node " + std::to_string(n) + ": weight is not finite");
            any_start |= (flags[i] & DSMI_GRAMMAR_START) != 0;
            any_final |= (flags[i] & DSMI_GRAMMAR_FINAL) != 0;
            for (int j = arc_off[i]; j < arc_off[i + 1]; ++j)
                if (arc_pred[j] < 0 || arc_pred[j] >= N)
                    return ctc_refuse(err, DSMI_ERR_INVALID, at(g) + "node " + std::to_string(n) + ": predecessor " + std::to_string(arc_pred[j]) + " outside the graph");
        }
        if (N > 0 && !any_start) return ctc_refuse(err, DSMI_ERR_INVALID, at(g) + "no start node");
        if (N > 0 && !any_final) return ctc_refuse(err, DSMI_ERR_INVALID, at(g) + "no final node");
    }
    (void)empty_ok;      // (any value: non-zero accepts the empty sentence)
    return DSMI_OK;
}

}  // namespace dsmi
