// Streaming grammar decoding's handles (include/dsmi.h): dsmi_grammar_net, a pool of graphs checked, packed and uploaded once,
// and dsmi_grammar_stream, one live utterance's carried search over one graph of a net (the kernel: grammar_stream.hip).
// dsmi_grammar_stream_advance_many hands every number and array to grammar_stream_check (grammar_stream_host.h) -- a refusal
// comes before any launch, before any state changes and before any output write -- then uploads one table of descriptors,
// launches once and copies the results of the streams whose mode asks for one back.
#include "decoder.h"
#include "grammar_stream.h"

#include <cstring>

using namespace dsmi;

struct dsmi_grammar_net {
    dsmi_decoder* d = nullptr;
    int device = 0, C = 0, blank = 0, K = 0, max_nodes = 0, max_arcs = 0;
    std::vector<int32_t> nodes_of, arcs_of;      // [K] the nodes and arcs of each graph
    int32_t* up = nullptr;              // device: the packed pool, laid out as `at` says
    size_t at_no = 0, at_eo = 0, at_wd = 0, at_wt = 0, at_ao = 0, at_ho = 0, at_hv = 0, at_ar = 0;      // int32 words
    std::string err;
    // one call at a time: the descriptor table and the results of a launch
    std::mutex mu;
    DevBuf io;
};

struct dsmi_grammar_stream {
    dsmi_grammar_net* n = nullptr;
    int graph = 0, max_frames = 0;
    int64_t frames = 0;                 // frames consumed since the utterance began
    bool ended = false;                 // a final result was taken: no more frames before a reset
    GrammarStreamPlan plan{};
    unsigned char* block = nullptr;
    std::string err;
};

static thread_local std::string g_gs_error;

#define GS_HIP(expr)                                                                                      \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) { g_gs_error = std::string(#expr) + ": " + hipGetErrorString(e_); return DSMI_ERR_HIP; } \
    } while (0)

extern "C" int dsmi_grammar_stream_plan(int n_nodes, int n_arcs, int n_labels, int max_frames, int64_t* info) {
    if (!info) return DSMI_ERR_INVALID;
    GrammarStreamPlan plan;
    std::string err;
    if (int rc = grammar_stream_plan(n_nodes, n_arcs, n_labels, max_frames, &plan, err)) return rc;
    info[0] = plan.node_stride; info[1] = plan.lds_bytes; info[2] = plan.block_bytes;
    return DSMI_OK;
}

extern "C" int dsmi_grammar_net_create(dsmi_decoder* d, const dsmi_grammar_pool* pool, dsmi_grammar_net** out) {
    if (!d || !pool || !out) { g_gs_error = "bad grammar net arguments"; return DSMI_ERR_INVALID; }
    const int C = (int)d->labels.size(), K = pool->K;
    if (K > 0 && (!pool->node_off || !pool->labels || !pool->flags || !pool->arc_off || !pool->arc_pred || !pool->empty_ok)) {
        g_gs_error = "grammar: a NULL array in the pool"; return DSMI_ERR_INVALID;
    }
    // dsmi_grammar's rules for the pool, on one clip of one frame (the clip rules have nothing to refuse)
    std::vector<int32_t> sz, cg;
    int n_nodes = 0, n_arcs = 0;
    if (int rc = grammar_check(nullptr, 1, 1, K, pool->node_off, pool->labels, pool->weights, pool->flags, pool->arc_off, pool->arc_pred,
                               pool->empty_ok, nullptr, C, d->blank, sz, cg, &n_nodes, &n_arcs, g_gs_error)) return rc;
    // ---- the upload, int32 words: node_off [K + 1], empty_ok [K], node words [nodes], weights [nodes], arc_off [nodes + 1],
    // heavy_off [K + 1], the heavy list and the arcs as 16-bit words (dsmi_grammar's, and kGrammarHeavy on the listed nodes)
    const size_t total = (size_t)pool->node_off[K], n_arc_all = (size_t)pool->arc_off[total];
    std::vector<int32_t> heavy_off;
    std::vector<uint16_t> heavy;
    grammar_heavy_list(K, pool->node_off, pool->arc_off, heavy_off, heavy);
    dsmi_grammar_net* n = new dsmi_grammar_net();
    n->d = d; n->device = d->device; n->C = C; n->blank = d->blank; n->K = K; n->max_nodes = n_nodes; n->max_arcs = n_arcs;
    n->at_no = 0; n->at_eo = n->at_no + K + 1; n->at_wd = n->at_eo + K; n->at_wt = n->at_wd + total; n->at_ao = n->at_wt + total;
    n->at_ho = n->at_ao + total + 1; n->at_hv = n->at_ho + K + 1; n->at_ar = n->at_hv + (heavy.size() + 1) / 2;
    const size_t in_words = n->at_ar + (n_arc_all + 1) / 2 + 1;
    std::vector<int32_t> up(in_words, 0);
    std::memcpy(up.data() + n->at_no, pool->node_off, sizeof(int32_t) * (K + 1));
    std::memcpy(up.data() + n->at_eo, pool->empty_ok, sizeof(int32_t) * K);
    std::memcpy(up.data() + n->at_ao, pool->arc_off, sizeof(int32_t) * (total + 1));
    std::memcpy(up.data() + n->at_ho, heavy_off.data(), sizeof(int32_t) * (K + 1));
    if (!heavy.empty()) std::memcpy(up.data() + n->at_hv, heavy.data(), sizeof(uint16_t) * heavy.size());
    if (pool->weights && total) std::memcpy(up.data() + n->at_wt, pool->weights, sizeof(float) * total);
    uint16_t* arc16 = reinterpret_cast<uint16_t*>(up.data() + n->at_ar);
    n->nodes_of.resize(K); n->arcs_of.resize(K);
    for (int g = 0; g < K; ++g) {
        const int n0 = pool->node_off[g];
        n->nodes_of[g] = pool->node_off[g + 1] - n0;
        n->arcs_of[g] = pool->arc_off[pool->node_off[g + 1]] - pool->arc_off[n0];
        for (int i = n0; i < pool->node_off[g + 1]; ++i) {
            up[n->at_wd + i] = pool->labels[i] | ((pool->flags[i] & DSMI_GRAMMAR_START) ? kGrammarStart : 0) |
                               ((pool->flags[i] & DSMI_GRAMMAR_FINAL) ? kGrammarFinal : 0) |
                               (pool->arc_off[i + 1] - pool->arc_off[i] > kGrammarHeavyFan ? kGrammarHeavy : 0);
            for (int j = pool->arc_off[i]; j < pool->arc_off[i + 1]; ++j) {
                const int p = pool->arc_pred[j];
                arc16[j] = (uint16_t)(p | (pool->labels[n0 + p] != pool->labels[i] ? kGrammarArcTok : 0));
            }
        }
    }
    if (hipSetDevice(d->device) != hipSuccess || hipMalloc((void**)&n->up, sizeof(int32_t) * in_words) != hipSuccess ||
        hipMemcpy(n->up, up.data(), sizeof(int32_t) * in_words, hipMemcpyHostToDevice) != hipSuccess) {
        dsmi_grammar_net_destroy(n);
        g_gs_error = "grammar net: HIP allocation or upload failed"; return DSMI_ERR_NOMEM;
    }
    *out = n;
    return DSMI_OK;
}

extern "C" void dsmi_grammar_net_destroy(dsmi_grammar_net* n) {
    if (!n) return;
    (void)hipSetDevice(n->device);
    (void)hipDeviceSynchronize();
    if (n->up) (void)hipFree(n->up);
    n->io.release();
    delete n;
}

extern "C" const char* dsmi_grammar_net_last_error(const dsmi_grammar_net* n) { return n ? n->err.c_str() : g_gs_error.c_str(); }

extern "C" int dsmi_grammar_net_info(const dsmi_grammar_net* n, int* K, int* max_nodes, int* max_arcs) {
    if (!n) return DSMI_ERR_INVALID;
    if (K) *K = n->K;
    if (max_nodes) *max_nodes = n->max_nodes;
    if (max_arcs) *max_arcs = n->max_arcs;
    return DSMI_OK;
}

extern "C" int dsmi_grammar_stream_create(dsmi_grammar_net* n, int graph, int max_frames, dsmi_grammar_stream** out) {
    if (!n || !out) { g_gs_error = "bad grammar stream arguments"; return DSMI_ERR_INVALID; }
    if (graph < 0 || graph >= n->K) { g_gs_error = "grammar stream: graph outside 0 .. K-1"; return DSMI_ERR_INVALID; }
    GrammarStreamPlan plan;
    if (int rc = grammar_stream_plan(n->nodes_of[graph], n->arcs_of[graph], n->C, max_frames, &plan, g_gs_error)) return rc;
    GS_HIP(hipSetDevice(n->device));
    dsmi_grammar_stream* s = new dsmi_grammar_stream();
    s->n = n; s->graph = graph; s->max_frames = max_frames; s->plan = plan;
    if (hipMalloc((void**)&s->block, (size_t)plan.block_bytes) != hipSuccess) {
        delete s;
        g_gs_error = "grammar stream: HIP allocation failed"; return DSMI_ERR_NOMEM;
    }
    *out = s;
    return DSMI_OK;
}

extern "C" void dsmi_grammar_stream_destroy(dsmi_grammar_stream* s) {
    if (!s) return;
    (void)hipSetDevice(s->n->device);
    (void)hipDeviceSynchronize();
    if (s->block) (void)hipFree(s->block);
    delete s;
}

extern "C" const char* dsmi_grammar_stream_last_error(const dsmi_grammar_stream* s) { return s ? s->err.c_str() : g_gs_error.c_str(); }

extern "C" int dsmi_grammar_stream_reset(dsmi_grammar_stream* s) {
    if (!s) return DSMI_ERR_INVALID;
    s->frames = 0;        // the next advance starts at t0 = 0: nothing of the block is read
    s->ended = false;
    return DSMI_OK;
}

extern "C" int dsmi_grammar_stream_frames(const dsmi_grammar_stream* s, int64_t* frames) {
    if (!s || !frames) return DSMI_ERR_INVALID;
    *frames = s->frames;
    return DSMI_OK;
}

extern "C" int dsmi_grammar_stream_advance_many(dsmi_grammar_stream* const* ss, int n, const float* const* probs_dev, const int32_t* frames,
                                                const int32_t* mode, int P_stride, int32_t* path_lens, int32_t* path_nodes,
                                                int32_t* path_spans, float* token_probs, float* path_logp, int32_t* status,
                                                int32_t* complete, void* stream) {
    // ---- refusals, before any state changes
    if (!ss || !frames || !mode || n < 1 || n > DSMI_GRAMMAR_STREAM_MANY_MAX) { g_gs_error = "bad grammar stream arguments"; return DSMI_ERR_INVALID; }
    std::vector<const void*> handles(n), net_of(n);
    std::vector<int64_t> consumed(n);
    std::vector<int32_t> ended(n), cap(n);
    for (int i = 0; i < n; ++i) {
        if (!ss[i]) { g_gs_error = "grammar stream " + std::to_string(i) + ": null handle"; return DSMI_ERR_INVALID; }
        handles[i] = ss[i]; net_of[i] = ss[i]->n; consumed[i] = ss[i]->frames; ended[i] = ss[i]->ended ? 1 : 0; cap[i] = ss[i]->max_frames;
    }
    const bool outputs = path_lens && path_nodes && path_spans && token_probs && path_logp && status;
    if (int rc = grammar_stream_check(handles.data(), net_of.data(), consumed.data(), ended.data(), cap.data(), n, probs_dev, frames, mode,
                                      P_stride, outputs, g_gs_error)) return rc;
    bool work = false, results = false;
    for (int i = 0; i < n; ++i) { work |= frames[i] > 0 || mode[i] != 0; results |= mode[i] != 0; }
    if (!work) return DSMI_OK;
    dsmi_grammar_net* net = ss[0]->n;
    std::lock_guard<std::mutex> lock(net->mu);
    GS_HIP(hipSetDevice(net->device));
    hipStream_t st = (hipStream_t)stream;
    // ---- workspace: the descriptors [n], then path_lens [n], path_nodes [n][P], path_spans [n][P][2], token_probs [n][P], logp [n],
    // status [n], complete [n]
    const size_t nP = results ? (size_t)n * P_stride : 0, out_words = 4 * nP + 4 * (size_t)n;
    const size_t tab_bytes = (sizeof(GrammarStreamDesc) * (size_t)n + 255) & ~(size_t)255;
    const size_t io_bytes = tab_bytes + sizeof(int32_t) * out_words;
    if (!net->io.holds(io_bytes)) {
        GS_HIP(hipDeviceSynchronize());      // (a launch in flight may still read a buffer that is about to be freed)
        GS_HIP(net->io.reserve(io_bytes));
    }
    std::vector<GrammarStreamDesc> tab(n);
    for (int i = 0; i < n; ++i) {
        GrammarStreamDesc& q = tab[i];
        dsmi_grammar_stream* s = ss[i];
        q.probs = frames[i] > 0 ? probs_dev[i] : nullptr;
        q.head = reinterpret_cast<GrammarStreamHead*>(s->block);
        q.pairs = reinterpret_cast<float2*>(s->block + s->plan.pairs_at);
        q.hist = reinterpret_cast<float*>(s->block + s->plan.hist_at);
        q.bp = reinterpret_cast<uint16_t*>(s->block + s->plan.bp_at);
        q.T = frames[i]; q.t0 = (int32_t)s->frames; q.graph = s->graph; q.ns = (int32_t)s->plan.node_stride; q.mode = mode[i]; q.pad = 0;
    }
    unsigned char* io = net->io.as<unsigned char>();
    int32_t* w_out = reinterpret_cast<int32_t*>(io + tab_bytes);
    GS_HIP(hipMemcpyAsync(io, tab.data(), sizeof(GrammarStreamDesc) * (size_t)n, hipMemcpyHostToDevice, st));
    GS_HIP(hipMemsetAsync(w_out, 0, sizeof(int32_t) * out_words, st));
    GrammarPlan gp;
    if (int rc = grammar_plan(1, 1, net->max_nodes, net->max_arcs, &gp, g_gs_error)) return rc;
    GrammarStreamArgs a{};
    a.desc = reinterpret_cast<const GrammarStreamDesc*>(io); a.C = net->C; a.blank = net->blank;
    a.node_off = net->up + net->at_no; a.empty_ok = net->up + net->at_eo; a.words = net->up + net->at_wd;
    a.weights = reinterpret_cast<const float*>(net->up + net->at_wt); a.arc_off = net->up + net->at_ao;
    a.heavy_off = net->up + net->at_ho; a.heavy = reinterpret_cast<const uint16_t*>(net->up + net->at_hv);
    a.arc_words16 = reinterpret_cast<const uint16_t*>(net->up + net->at_ar);
    a.node_stride = (int)gp.node_stride; a.arc_words = (int)grammar_arc_words(net->max_arcs); a.P_stride = P_stride;
    a.path_lens = w_out; a.path_nodes = a.path_lens + n; a.path_spans = a.path_nodes + nP;
    a.token_probs = reinterpret_cast<float*>(a.path_spans + 2 * nP); a.path_logp = a.token_probs + nP;
    a.status = reinterpret_cast<int32_t*>(a.path_logp + n); a.complete = a.status + n;
    GS_HIP(launch_grammar_stream(a, n, st));
    // ---- from here on the handles change: the launch is in the stream
    for (int i = 0; i < n; ++i) {
        ss[i]->frames += frames[i];
        if (mode[i] == 2) ss[i]->ended = true;
    }
    if (!results) { GS_HIP(hipStreamSynchronize(st)); return DSMI_OK; }
    // the results come back into an image of the call's own; a stream with mode 0 has nothing written for it
    std::vector<int32_t> out(out_words);
    GS_HIP(hipMemcpyAsync(out.data(), w_out, sizeof(int32_t) * out_words, hipMemcpyDeviceToHost, st));
    GS_HIP(hipStreamSynchronize(st));
    const int32_t* o_len = out.data();
    const int32_t* o_nod = o_len + n;
    const int32_t* o_spn = o_nod + nP;
    const int32_t* o_tok = o_spn + 2 * nP;
    const int32_t* o_lp = o_tok + nP;
    const int32_t* o_st = o_lp + n;
    const int32_t* o_cp = o_st + n;
    const size_t P = (size_t)P_stride;
    for (int i = 0; i < n; ++i) {
        if (mode[i] == 0) continue;
        path_lens[i] = o_len[i];
        std::memcpy(path_nodes + i * P, o_nod + i * P, sizeof(int32_t) * P);
        std::memcpy(path_spans + 2 * i * P, o_spn + 2 * i * P, sizeof(int32_t) * 2 * P);
        std::memcpy(token_probs + i * P, o_tok + i * P, sizeof(float) * P);
        std::memcpy(path_logp + i, o_lp + i, sizeof(float));
        status[i] = o_st[i];
        if (complete) complete[i] = o_cp[i];
    }
    return DSMI_OK;
}
