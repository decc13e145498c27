// Streaming grammar decoding (grammar_stream.hip): dsmi_grammar's graph search carried from chunk to chunk of N live sessions in
// one launch, one workgroup per stream.  Launched by dsmi_grammar_stream_advance_many (grammar_net.hip), which checks every
// argument first (grammar_stream_host.h).
#pragma once
#include "common.h"
#include "grammar_stream_host.h"

namespace dsmi {

struct GrammarStreamDesc {              // one stream of a launch
    const float* probs;                 // [T][C] this call's rows (NULL with T = 0)
    GrammarStreamHead* head;            // the stream's block: lead and the frame count,
    float2* pairs;                      // the tok / blk pairs [ns] of the last frame consumed,
    float* hist;                        // the rows consumed [max_frames][C],
    uint16_t* bp;                       // the backpointers [max_frames][ns]
    int32_t T, t0;                      // frames of this call, frames consumed before it
    int32_t graph, ns;                  // the stream's graph and its own node stride
    int32_t mode, pad;                  // 0 advance only, 1 then the partial result, 2 then the final result
};

struct GrammarStreamArgs {
    const GrammarStreamDesc* desc;      // [n]
    int C, blank;
    const int32_t* node_off;            // [K + 1] where each graph's nodes lie in the net
    const int32_t* words;               // [nodes] label | kGrammarStart | kGrammarFinal | kGrammarHeavy
    const float* weights;               // [nodes]
    const int32_t* arc_off;             // [nodes + 1]
    const uint16_t* arc_words16;        // [arcs] as dsmi_grammar packs them
    const int32_t* empty_ok;            // [K]
    const int32_t* heavy_off;           // [K + 1] where each graph's heavy nodes lie in `heavy`
    const uint16_t* heavy;              // graph-local ids of the nodes with more than kGrammarHeavyFan predecessors
    int node_stride;                    // of the LDS rows: multiple of 4, >= the most nodes of a graph of the net
    int arc_words;                      // multiple of 4, >= the most arcs of a graph of the net
    int P_stride;                       // row stride of the three path arrays
    int32_t* path_lens;                 // [n]
    int32_t* path_nodes;                // [n][P_stride]
    int32_t* path_spans;                // [n][P_stride][2]
    float* token_probs;                 // [n][P_stride]
    float* path_logp;                   // [n]
    int32_t* status;                    // [n]
    int32_t* complete;                  // [n]
};

hipError_t launch_grammar_stream(const GrammarStreamArgs& a, int n, hipStream_t s);

}  // namespace dsmi
