// CTC grammar posterior (grammar_post.hip): the summed probability of every path a token graph accepts, and from alpha + beta
// over the graph's trellis in float64 the per-frame label posteriors and each node's expected number of entries.  Launched by
// dsmi_grammar_posterior (ctc_tools.hip), which checks every argument first and builds the transposed arcs, the start lists and
// the label buckets (grammar_post_host.h).
#pragma once
#include "common.h"
#include "grammar_post_host.h"

namespace dsmi {

struct GrammarPostArgs {
    const float* probs;                 // [B][T_out][C] softmax probabilities
    int B, T_out, C, blank;
    const int32_t* sizes;               // [B] frames of each clip (<= T_out)
    const int32_t* clip_graph;          // [B] the graph of each clip
    const int32_t* node_off;            // [K + 1] where each graph's nodes lie in the pool
    const int32_t* words;               // [nodes] label | kGrammarStart | kGrammarFinal
    const float* weights;               // [nodes]
    const int32_t* arc_off;             // [nodes + 1] where each node's predecessors lie in arc16
    const uint16_t* arc16;              // [arcs] the predecessor's graph-local id | kGrammarArcTok where the two labels differ
    const int32_t* succ_off;            // [nodes + 1] where each node's successors lie in succ16
    const uint16_t* succ16;             // [arcs] the successor's graph-local id | kGrammarArcTok where the two labels differ
    const int32_t* start_off;           // [K + 1] where each graph's start nodes lie in start16
    const uint16_t* start16;            // the start nodes, graph-local
    const int32_t* bucket_off;          // [K][C + 1] where the nodes of a label lie in bucket_nodes, from the graph's first node
    const int32_t* bucket_nodes;        // [nodes] each graph's nodes by label, graph-local
    const int32_t* empty_ok;            // [K]
    int node_stride;                    // multiple of 4, >= the most nodes of a graph
    int arc_words;                      // multiple of 4, >= the most arcs of a graph
    // the stored trellises, (tok, blk) pairs [B][T_out][node_stride] and lead [B][T_out]:
    double2* fwd;                       // alpha_t
    double2* bwd;                       // beta_t - lp(t, the state's label)
    double* lead_fwd;
    double* lead_bwd;
    bool both;                          // visits or occ is asked for: false = the forward pass alone, for logp
    double* logp;                       // [B]
    int32_t* status;                    // [B]
    double* visits;                     // [B][N_stride], or null: columns n < the graph's nodes are written
    int N_stride;
    double* occ;                        // [B][T_out][C], or null: written in full
};

hipError_t launch_grammar_post(const GrammarPostArgs& a, hipStream_t s);

}  // namespace dsmi
