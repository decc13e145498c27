// CTC grammar decoding (grammar.hip): the Viterbi path through the CTC trellis of a token graph, one workgroup per clip.
// Launched by dsmi_grammar (ctc_tools.hip), which checks every argument first (grammar_host.h).
#pragma once
#include "common.h"
#include "grammar_host.h"

namespace dsmi {

struct GrammarArgs {
    const float* probs;                 // [B][T_out][C] softmax probabilities
    int T_out, C, blank;
    const int32_t* sizes;               // [B] frames of each clip (<= T_out)
    const int32_t* clip_graph;          // [B] the graph of each clip
    const int32_t* node_off;            // [K + 1] where each graph's nodes lie in the pool
    const int32_t* words;               // [nodes] label | kGrammarStart | kGrammarFinal
    const float* weights;               // [nodes]
    const int32_t* arc_off;             // [nodes + 1] where each node's predecessors lie in arc_words16
    const uint16_t* arc_words16;        // [arcs] the predecessor's graph-local id | kGrammarArcTok where the two labels differ
    const int32_t* empty_ok;            // [K]
    int node_stride;                    // multiple of 4, >= the most nodes of a graph
    int arc_words;                      // multiple of 4, >= the most arcs of a graph
    uint16_t* bp;                       // [B][T_out][node_stride] backpointers
    int32_t* path_lens;                 // [B]
    int32_t* path_nodes;                // [B][T_out]
    int32_t* path_spans;                // [B][T_out][2]
    float* token_probs;                 // [B][T_out]
    float* path_logp;                   // [B]
    int32_t* status;                    // [B]
    int trace_form;                     // (experiments build) 1: the backtrace by one lane, a load per frame; 2: no backtrace at all
};

hipError_t launch_grammar(const GrammarArgs& a, int B, hipStream_t s);

}  // namespace dsmi
