// The host half of streaming grammar decoding (dsmi_grammar_net_*, dsmi_grammar_stream_*: grammar_net.hip; the kernel:
// grammar_stream.hip): the layout of a stream's device block, the list of heavy nodes and the check of everything an advance call
// hands in.  No HIP: a plain C++ compiler takes it, and tools/asan/host_fuzz.cpp (grammarstreamcheck) runs it under ASan + UBSan
// on exactly sized arrays.  A check returns DSMI_OK or a DSMI_ERR_* code with the message in `err`.
#pragma once
#include "grammar_host.h"

#include <algorithm>

namespace dsmi {

// a node's word in LDS, beside kGrammarStart and kGrammarFinal: the node is on the heavy list (the owner thread leaves it alone)
constexpr int kGrammarHeavy = 1 << 10;
// a node with more predecessors than this is entered by a whole wave, its lanes striding the arc list
constexpr int kGrammarHeavyFan = 32;
constexpr int kGrammarHeavyMax = DSMI_GRAMMAR_MAX_ARCS / (kGrammarHeavyFan + 1);      // the most heavy nodes of one graph
static_assert(kGrammarHeavyMax <= 256, "the heavy list is 256 16-bit words of LDS");

constexpr uint64_t kGrammarStreamBlockCap = (uint64_t)1 << 31;      // bytes of one stream's device block
constexpr uint64_t kGrammarStreamOutCap = (uint64_t)1 << 24;        // n * P_stride of a call: the output image

// A stream's device block: a header, then the tok / blk pairs of the last frame consumed, the probability rows consumed and the
// backpointer rows of the frames consumed.
struct GrammarStreamHead {
    float lead;               // the blank before the first token, as of the last frame consumed
    int32_t frames;           // frames consumed since the utterance began
    int32_t pad[2];
};
struct GrammarStreamPlan {
    int64_t node_stride;      // grammar_plan's
    int64_t lds_bytes;        // grammar_plan's and the heavy list
    int64_t block_bytes;      // the whole block
    int64_t pairs_at, hist_at, bp_at;      // byte offsets within the block
};

inline int grammar_stream_plan(int n_nodes, int n_arcs, int n_labels, int max_frames, GrammarStreamPlan* plan, std::string& err) {
    if (max_frames < 1) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar stream: max_frames must be positive");
    if (max_frames > DSMI_GRAMMAR_STREAM_MAX_FRAMES)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar stream: max_frames " + std::to_string(max_frames) + " exceeds DSMI_GRAMMAR_STREAM_MAX_FRAMES (" +
                                                      std::to_string(DSMI_GRAMMAR_STREAM_MAX_FRAMES) + ")");
    if (n_labels < 1 || n_labels > kCtcMaxLabels)
        return ctc_refuse(err, DSMI_ERR_INVALID, "grammar stream: n_labels outside 1 .. " + std::to_string(kCtcMaxLabels));
    GrammarPlan gp;
    if (int rc = grammar_plan(1, max_frames, n_nodes, n_arcs, &gp, err)) return rc;
    plan->node_stride = gp.node_stride;
    plan->lds_bytes = gp.lds_bytes + 2 * 256;
    plan->pairs_at = (int64_t)sizeof(GrammarStreamHead);
    plan->hist_at = plan->pairs_at + 8 * gp.node_stride;
    plan->bp_at = plan->hist_at + 4 * (int64_t)max_frames * n_labels;
    plan->block_bytes = plan->bp_at + 2 * (int64_t)max_frames * gp.node_stride;
    if ((uint64_t)plan->block_bytes > kGrammarStreamBlockCap)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar stream: the stream's block exceeds 2^31 bytes (" + std::to_string(plan->block_bytes) + ")");
    return DSMI_OK;
}

// The heavy nodes of a checked pool: heavy_off [K + 1], and per graph the graph-local ids, ascending, of the nodes with more than
// kGrammarHeavyFan predecessors.
inline void grammar_heavy_list(int K, const int32_t* node_off, const int32_t* arc_off, std::vector<int32_t>& heavy_off, std::vector<uint16_t>& heavy) {
    heavy_off.assign((size_t)K + 1, 0);
    heavy.clear();
    for (int g = 0; g < K; ++g) {
        for (int i = node_off[g]; i < node_off[g + 1]; ++i)
            if (arc_off[i + 1] - arc_off[i] > kGrammarHeavyFan) heavy.push_back((uint16_t)(i - node_off[g]));
        heavy_off[g + 1] = (int32_t)heavy.size();
    }
}

// An advance call.  handles / net_of [n] = each stream and its net, consumed / ended / max_frames [n] = each stream's state;
// outputs = all six output arrays are there.
inline int grammar_stream_check(const void* const* handles, const void* const* net_of, const int64_t* consumed, const int32_t* ended,
                                const int32_t* max_frames, int n, const float* const* probs, const int32_t* frames, const int32_t* mode,
                                int P_stride, bool outputs, std::string& err) {
    if (n < 1 || n > DSMI_GRAMMAR_STREAM_MANY_MAX)
        return ctc_refuse(err, DSMI_ERR_INVALID, "grammar stream: n outside 1 .. DSMI_GRAMMAR_STREAM_MANY_MAX (" + std::to_string(DSMI_GRAMMAR_STREAM_MANY_MAX) + ")");
    auto at = [](int i) { return "grammar stream " + std::to_string(i) + ": "; };
    {
        std::vector<const void*> sorted(handles, handles + n);
        std::sort(sorted.begin(), sorted.end());
        const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
        if (twice != sorted.end()) {
            int i = n - 1;
            while (handles[i] != *twice) --i;      // (the later of the two)
            return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "the same handle appears twice in one call");
        }
    }
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (net_of[i] != net_of[0]) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "the streams of one call must belong to one net");
        if (frames[i] < 0) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "negative frame count");
        if (frames[i] > 0 && (!probs || !probs[i])) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "no probabilities for " + std::to_string(frames[i]) + " frames");
        if (mode[i] < 0 || mode[i] > 2) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "mode " + std::to_string(mode[i]) + " outside 0 .. 2");
        if (frames[i] > 0 && ended[i])
            return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "the utterance has ended (mode 2): dsmi_grammar_stream_reset comes before more frames");
        const int64_t after = consumed[i] + (int64_t)frames[i];
        if (after > (int64_t)max_frames[i])
            return ctc_refuse(err, DSMI_ERR_CAPACITY, at(i) + "the utterance would reach " + std::to_string(after) + " frames, max_frames is " + std::to_string(max_frames[i]));
        if (mode[i] != 0) {
            any = true;
            if ((int64_t)P_stride < after) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "P_stride " + std::to_string(P_stride) + " is below the utterance's " + std::to_string(after) + " frames");
        }
    }
    if (any && !outputs) return ctc_refuse(err, DSMI_ERR_INVALID, "grammar stream: a result is due and an output array is NULL");
    if (any && (uint64_t)n * (uint64_t)P_stride > kGrammarStreamOutCap) return ctc_refuse(err, DSMI_ERR_CAPACITY, "grammar stream: n * P_stride exceeds 2^24 (the results)");
    return DSMI_OK;
}

}  // namespace dsmi
