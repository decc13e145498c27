// The six tools over the CTC trellis of probabilities that are already on the device: forced alignment of known transcripts
// (dsmi_align; the kernel: align.hip), of one long recording (dsmi_align_long; align_long.hip), phrase search (dsmi_spot; spot.hip), transcript scoring (dsmi_score; score.hip),
// token confidence (dsmi_alternatives; alt.hip), occupancy (dsmi_occupancy; occ.hip), grammar decoding (dsmi_grammar; grammar.hip) and the grammar posterior (dsmi_grammar_posterior; grammar_post.hip) -- and, on the same handle and by the
// same conventions, the batched edit distance of token sequences (dsmi_edit_distance; edit.hip) and the language-model score of
// known sentences (dsmi_lm_score; lmscore.hip), which need no probabilities.
// Each entry checks its pointers, hands every number and array to its check (ctc_host.h: a refusal comes before any launch and
// before any output write), grows its workspaces, uploads, launches and copies the results back.  A clip or candidate whose
// transcript cannot fit its frames (one frame per token, one more between two equal tokens) is skipped and marked.
#include "decoder.h"
#include "align.h"
#include "align_long.h"
#include "spot.h"
#include "score.h"
#include "alt.h"
#include "occ.h"
#include "grammar.h"
#include "grammar_post.h"
#include "edit.h"
#include "lmscore.h"

#include <cmath>
#include <cstring>

using namespace dsmi;

// The workspaces of one call: nothing happens when every capacity suffices; otherwise ONE device synchronise (a launch in flight
// may still read a buffer that is about to be freed), then each buffer that is too small is replaced.
static int reserve_all(dsmi_decoder* d, DevBuf& a, size_t a_bytes, DevBuf* b = nullptr, size_t b_bytes = 0, DevBuf* c = nullptr,
                       size_t c_bytes = 0) {
    if (a.holds(a_bytes) && (!b || b->holds(b_bytes)) && (!c || c->holds(c_bytes))) return DSMI_OK;
    DEC_HIP(d, hipDeviceSynchronize());
    DEC_HIP(d, a.reserve(a_bytes));
    if (b) DEC_HIP(d, b->reserve(b_bytes));
    if (c) DEC_HIP(d, c->reserve(c_bytes));
    return DSMI_OK;
}

extern "C" int dsmi_align(dsmi_decoder* d, const float* probs, const int32_t* sizes, int B, int To, const int32_t* targets,
                          const int32_t* target_lens, int L_stride, int32_t* spans, float* token_probs, float* path_logp,
                          int32_t* status, void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    const int C = (int)d->labels.size();
    if (!probs || !target_lens || !path_logp || !status || (L_stride > 0 && (!targets || !spans || !token_probs))) {
        d->err = "bad align arguments"; return DSMI_ERR_INVALID;
    }
    std::vector<int32_t> sz, tl;
    int L_max = 0;
    if (int rc = align_check(sizes, B, To, targets, target_lens, L_stride, C, d->blank, sz, tl, &L_max, d->err)) return rc;
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- workspaces: io = sizes [B], lens [B], targets [B][L], spans [B][L][2], token probs [B][L], logp [B]
    const int S_max = 2 * L_max + 1, S_stride = round_up(S_max, 4);
    const size_t BL = (size_t)B * L_stride, io_words = 3 * (size_t)B + 4 * BL;
    if (int rc = reserve_all(d, d->al_io, sizeof(int32_t) * io_words, &d->al_bp, (size_t)B * To * S_stride + kAlignBpSlack)) return rc;
    int32_t* w_sz = d->al_io.as<int32_t>(); int32_t* w_tl = w_sz + B; int32_t* w_tg = w_tl + B;
    int32_t* w_sp = w_tg + BL; float* w_tp = reinterpret_cast<float*>(w_sp + 2 * BL); float* w_lp = w_tp + BL;
    DEC_HIP(d, hipMemcpyAsync(w_sz, sz.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_tl, tl.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    if (BL) DEC_HIP(d, hipMemcpyAsync(w_tg, targets, sizeof(int32_t) * BL, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemsetAsync(w_sp, 0, sizeof(int32_t) * (3 * BL + B), s));
    AlignArgs a{};
    a.probs = probs; a.T_out = To; a.C = C; a.blank = d->blank;
    a.sizes = w_sz; a.tlen = w_tl; a.targets = w_tg; a.L_stride = L_stride; a.S_max = S_max;
    a.bp = d->al_bp.as<unsigned char>(); a.S_stride = S_stride;
    a.spans = w_sp; a.token_probs = w_tp; a.path_logp = w_lp;
    DEC_HIP(d, launch_align(a, B, s));
    if (BL) {
        DEC_HIP(d, hipMemcpyAsync(spans, w_sp, sizeof(int32_t) * 2 * BL, hipMemcpyDeviceToHost, s));
        DEC_HIP(d, hipMemcpyAsync(token_probs, w_tp, sizeof(float) * BL, hipMemcpyDeviceToHost, s));
    }
    DEC_HIP(d, hipMemcpyAsync(path_logp, w_lp, sizeof(float) * B, hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        status[b] = tl[b] < 0 ? 1 : 0;
        if (tl[b] < 0) path_logp[b] = -INFINITY;
    }
    return DSMI_OK;
}

extern "C" int dsmi_align_long_plan(int T, int L, int64_t* info) {
    if (!info) return DSMI_ERR_INVALID;
    return align_long_plan(T, L, info);
}

extern "C" int dsmi_align_long(dsmi_decoder* d, const float* probs, int T, const int32_t* targets, int L, int lead_free, int tail_free,
                               int32_t* spans, float* token_probs, float* path_logp, int32_t* status, void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    const int C = (int)d->labels.size();
    if (!probs || !path_logp || !status || (L > 0 && (!targets || !spans || !token_probs))) {
        d->err = "bad align_long arguments"; return DSMI_ERR_INVALID;
    }
    AlongPlan plan;
    bool feasible = false;
    if (int rc = align_long_check(T, L, lead_free, tail_free, targets, C, d->blank, &plan, &feasible, d->err)) return rc;
    if (!feasible) {
        for (int k = 0; k < L; ++k) { spans[2 * k] = spans[2 * k + 1] = 0; token_probs[k] = 0.f; }
        path_logp[0] = -INFINITY;
        status[0] = 1;
        return DSMI_OK;
    }
#ifdef DSMI_EXPERIMENTS
    // DSMI_DEBUG_ALONG_FORM=w1792f128 | w896f64 | w128f64: the geometries that were measured and not adopted; the plan
    // entry does not follow
    if (const char* form = exp_env("DSMI_DEBUG_ALONG_FORM")) {
        if (std::string(form) == "w1792f128") plan = align_long_geometry(T, L, 1792, 128);
        if (std::string(form) == "w896f64") plan = align_long_geometry(T, L, 896, 64);
        if (std::string(form) == "w128f64") plan = align_long_geometry(T, L, 128, 64);
    }
#endif
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- workspaces: io = targets [L], spans [L][2], token probs [L], logp [1]; the checkpoint rows [plan.rows][S] floats
    const size_t Ls = (size_t)L;
    if (int rc = reserve_all(d, d->along_io, sizeof(int32_t) * (4 * Ls + 1), &d->along_rows, (size_t)plan.bytes)) return rc;
    int32_t* w_tg = d->along_io.as<int32_t>(); int32_t* w_sp = w_tg + Ls;
    float* w_tp = reinterpret_cast<float*>(w_sp + 2 * Ls); float* w_lp = w_tp + Ls;
    if (L) DEC_HIP(d, hipMemcpyAsync(w_tg, targets, sizeof(int32_t) * Ls, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemsetAsync(w_sp, 0, sizeof(int32_t) * (3 * Ls + 1), s));
    AlongArgs a{};
    a.probs = probs; a.T = T; a.C = C; a.blank = d->blank; a.L = L; a.S = 2 * L + 1;
    a.lead_free = lead_free; a.tail_free = tail_free; a.targets = w_tg; a.rows = d->along_rows.as<float>();
    a.W = (int)plan.W; a.F = (int)plan.F; a.frame_tiles = (int)plan.frame_tiles; a.state_tiles = (int)plan.state_tiles;
    a.spans = w_sp; a.token_probs = w_tp; a.path_logp = w_lp;
    DEC_HIP(d, launch_align_long(a, s));
    // the results come back into an image of the call's own and reach the caller's arrays only when everything has succeeded
    std::vector<int32_t> out(3 * Ls + 1);
    DEC_HIP(d, hipMemcpyAsync(out.data(), w_sp, sizeof(int32_t) * out.size(), hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    if (L) {
        std::memcpy(spans, out.data(), sizeof(int32_t) * 2 * Ls);
        std::memcpy(token_probs, out.data() + 2 * Ls, sizeof(float) * Ls);
    }
    std::memcpy(path_logp, out.data() + 3 * Ls, sizeof(float));
    status[0] = 0;
    return DSMI_OK;
}

extern "C" int dsmi_spot_plan(const int32_t* phrase_lens, int K, int32_t* group_of, int32_t* first_state) {
    if (!phrase_lens || !group_of || !first_state || K < 1 || K > DSMI_SPOT_MAX_PHRASES) return DSMI_ERR_INVALID;
    for (int k = 0; k < K; ++k)
        if (phrase_lens[k] < 1 || phrase_lens[k] > DSMI_SPOT_MAX_TOKENS) return DSMI_ERR_INVALID;
    return spot_plan(phrase_lens, K, group_of, first_state);
}

extern "C" int dsmi_spot(dsmi_decoder* d, const float* probs, const int32_t* sizes, int B, int To, const int32_t* phrases,
                         const int32_t* phrase_lens, int K, int L_stride, int max_hits, float min_mean_logp, int32_t* hits,
                         float* scores, int32_t* counts, float* track_scores, int32_t* track_starts, void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    const int C = (int)d->labels.size();
    if (!probs || !phrases || !phrase_lens || !hits || !scores || !counts) { d->err = "bad spot arguments"; return DSMI_ERR_INVALID; }
    std::vector<int32_t> sz;
    if (int rc = spot_check(sizes, B, To, phrases, phrase_lens, K, L_stride, max_hits, min_mean_logp, C, d->blank, sz, d->err)) return rc;
    // ---- the packing: per state its label and flags, groups of kSpotThreads states
    std::vector<int32_t> group_of(K), first_state(K);
    const int n_groups = spot_plan(phrase_lens, K, group_of.data(), first_state.data());
    std::vector<int32_t> words((size_t)n_groups * kSpotThreads, 0);
    spot_pack(phrases, phrase_lens, K, L_stride, d->blank, group_of.data(), first_state.data(), words.data());
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- workspaces: io = sizes [B], words [n_groups][256], hits [B][K][M][2], scores [B][K][M], counts [B][K]
    const size_t BK = (size_t)B * K, BKM = BK * max_hits, n_words = words.size(), n_tr = BK * To;
    const size_t io_words = (size_t)B + n_words + 3 * BKM + BK;
    if (int rc = reserve_all(d, d->sp_io, sizeof(int32_t) * io_words, &d->sp_tr, sizeof(int32_t) * 2 * n_tr)) return rc;
    int32_t* w_sz = d->sp_io.as<int32_t>(); int32_t* w_wd = w_sz + B; int32_t* w_hit = w_wd + n_words;
    float* w_sc = reinterpret_cast<float*>(w_hit + 2 * BKM); int32_t* w_cnt = w_hit + 3 * BKM;
    DEC_HIP(d, hipMemcpyAsync(w_sz, sz.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_wd, words.data(), sizeof(int32_t) * n_words, hipMemcpyHostToDevice, s));
    SpotArgs a{};
    a.probs = probs; a.T_out = To; a.C = C; a.K = K; a.n_groups = n_groups;
    a.sizes = w_sz; a.words = w_wd;
    a.E = d->sp_tr.as<float>(); a.ST = d->sp_tr.as<int32_t>() + n_tr;
    a.max_hits = max_hits; a.min_mean_logp = min_mean_logp;
    a.hits = w_hit; a.scores = w_sc; a.counts = w_cnt;
    DEC_HIP(d, launch_spot(a, B, s));
    // hits, scores and counts lie back to back: one copy into a host image, then the caller's three arrays
    std::vector<int32_t> out(3 * BKM + BK);
    DEC_HIP(d, hipMemcpyAsync(out.data(), w_hit, sizeof(int32_t) * out.size(), hipMemcpyDeviceToHost, s));
    if (track_scores) DEC_HIP(d, hipMemcpyAsync(track_scores, a.E, sizeof(float) * n_tr, hipMemcpyDeviceToHost, s));
    if (track_starts) DEC_HIP(d, hipMemcpyAsync(track_starts, a.ST, sizeof(int32_t) * n_tr, hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    std::memcpy(hits, out.data(), sizeof(int32_t) * 2 * BKM);
    std::memcpy(scores, out.data() + 2 * BKM, sizeof(float) * BKM);
    std::memcpy(counts, out.data() + 3 * BKM, sizeof(int32_t) * BK);
    return DSMI_OK;
}

extern "C" int dsmi_score_plan(const int32_t* cand_clip, const int32_t* cand_frames, const int32_t* target_lens, int N, int32_t* order) {
    if (!cand_clip || !cand_frames || !target_lens || !order || N <= 0) return DSMI_ERR_INVALID;
    for (int n = 0; n < N; ++n)
        if (cand_clip[n] < 0 || cand_frames[n] < 0 || target_lens[n] < 0) return DSMI_ERR_INVALID;
    return score_plan(cand_clip, cand_frames, target_lens, N, order);
}

extern "C" int dsmi_score(dsmi_decoder* d, const float* probs, const int32_t* sizes, int B, int To, const int32_t* cand_clip,
                          const int32_t* targets, const int32_t* target_lens, int N, int L_stride, double* logp, int32_t* status,
                          void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    const int C = (int)d->labels.size();
    if (!probs || !cand_clip || !target_lens || !logp || !status || (L_stride > 0 && !targets)) {
        d->err = "bad score arguments"; return DSMI_ERR_INVALID;
    }
    std::vector<int32_t> sz, tl, frames;
    int L_max = 0;
    if (int rc = score_check(sizes, B, To, cand_clip, targets, target_lens, N, L_stride, C, d->blank, sz, tl, frames, &L_max, d->err)) return rc;
    std::vector<int32_t> order(N);
    score_plan(cand_clip, frames.data(), target_lens, N, order.data());
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- the workspace: sizes [B], order [N], clips [N], lens [N], targets [N][L], then logp [N] doubles
    const size_t NL = (size_t)N * L_stride, in_words = ((size_t)B + 3 * (size_t)N + NL + 1) & ~(size_t)1;
    if (int rc = reserve_all(d, d->sc_io, sizeof(int32_t) * (in_words + 2 * (size_t)N))) return rc;
    int32_t* w_sz = d->sc_io.as<int32_t>(); int32_t* w_or = w_sz + B; int32_t* w_cl = w_or + N; int32_t* w_tl = w_cl + N; int32_t* w_tg = w_tl + N;
    double* w_lp = reinterpret_cast<double*>(w_sz + in_words);
    DEC_HIP(d, hipMemcpyAsync(w_sz, sz.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_or, order.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_cl, cand_clip, sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_tl, tl.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    if (NL) DEC_HIP(d, hipMemcpyAsync(w_tg, targets, sizeof(int32_t) * NL, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemsetAsync(w_lp, 0, sizeof(double) * N, s));
    ScoreArgs a{};
    a.probs = probs; a.T_out = To; a.C = C; a.blank = d->blank;
    a.sizes = w_sz; a.order = w_or; a.cand_clip = w_cl; a.tlen = w_tl; a.targets = w_tg; a.L_stride = L_stride;
    a.S_max = 2 * L_max + 1; a.logp = w_lp;
    DEC_HIP(d, launch_score(a, N, s));
    std::vector<double> out(N);
    DEC_HIP(d, hipMemcpyAsync(out.data(), w_lp, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    for (int n = 0; n < N; ++n) {
        status[n] = tl[n] < 0 ? 1 : 0;
        logp[n] = tl[n] < 0 ? -INFINITY : out[n];
    }
    return DSMI_OK;
}

extern "C" int dsmi_alternatives(dsmi_decoder* d, const float* probs, const int32_t* sizes, int B, int To, const int32_t* cand_clip,
                                 const int32_t* targets, const int32_t* target_lens, int N, int L_stride, double* logp,
                                 double* alt_logp, int32_t* status, void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    const int C = (int)d->labels.size();
    if (!probs || !cand_clip || !target_lens || !logp || !status || (L_stride > 0 && (!targets || !alt_logp))) {
        d->err = "bad alternatives arguments"; return DSMI_ERR_INVALID;
    }
    std::vector<int32_t> sz, tl, frames, base;
    int L_max = 0;
    uint64_t trellis = 0;
    if (int rc = alt_check(sizes, B, To, cand_clip, targets, target_lens, N, L_stride, C, d->blank, sz, tl, frames, base, &L_max, &trellis, d->err)) return rc;
    std::vector<int32_t> order(N);
    score_plan(cand_clip, frames.data(), target_lens, N, order.data());
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- the workspaces: sizes [B], order [N], clips [N], lens [N], bases [N], targets [N][L], then logp [N] doubles; the results
    // [N][L][C]; the stored trellises: forward pairs and backward of `trellis` elements each, the backward pair sums of half as many
    const size_t NL = (size_t)N * L_stride, NLC = NL * C, in_words = ((size_t)B + 4 * (size_t)N + NL + 1) & ~(size_t)1;
    const size_t ws_elems = 2 * (size_t)trellis + (size_t)trellis / 2 + 1;
    if (int rc = reserve_all(d, d->alt_io, sizeof(int32_t) * (in_words + 2 * (size_t)N), &d->alt_out, sizeof(double) * NLC, &d->alt_ws,
                             sizeof(double) * ws_elems)) return rc;
    int32_t* w_sz = d->alt_io.as<int32_t>(); int32_t* w_or = w_sz + B; int32_t* w_cl = w_or + N; int32_t* w_tl = w_cl + N;
    int32_t* w_ba = w_tl + N; int32_t* w_tg = w_ba + N;
    double* w_lp = reinterpret_cast<double*>(w_sz + in_words);
    DEC_HIP(d, hipMemcpyAsync(w_sz, sz.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_or, order.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_cl, cand_clip, sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_tl, tl.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_ba, base.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    if (NL) DEC_HIP(d, hipMemcpyAsync(w_tg, targets, sizeof(int32_t) * NL, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemsetAsync(w_lp, 0, sizeof(double) * N, s));
    AltArgs a{};
    a.probs = probs; a.T_out = To; a.C = C; a.blank = d->blank;
    a.sizes = w_sz; a.order = w_or; a.cand_clip = w_cl; a.tlen = w_tl; a.targets = w_tg; a.base = w_ba; a.L_stride = L_stride;
    a.S_max = 2 * L_max + 1; a.n_blocks = (L_max * C + kAltThreads - 1) / kAltThreads;
    a.fwd = d->alt_ws.as<double>(); a.bwd = a.fwd + trellis; a.bwd_pair = a.bwd + trellis;
    a.logp = w_lp; a.alt = d->alt_out.as<double>();
    DEC_HIP(d, launch_alt(a, N, s));
    // the results come back into images of the call's own and reach the caller's arrays only when everything has succeeded
    std::vector<double> out(N), rows(NLC);
    DEC_HIP(d, hipMemcpyAsync(out.data(), w_lp, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    if (NLC) DEC_HIP(d, hipMemcpyAsync(rows.data(), a.alt, sizeof(double) * NLC, hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    for (int n = 0; n < N; ++n) {
        status[n] = tl[n] < 0 ? 1 : 0;
        logp[n] = tl[n] < 0 ? -INFINITY : out[n];
        const size_t written = tl[n] < 0 ? 0 : (size_t)tl[n] * C, row = (size_t)L_stride * C;      // (the kernel writes rows k < length)
        double* dst = alt_logp ? alt_logp + (size_t)n * row : nullptr;
        for (size_t i = 0; i < row; ++i) dst[i] = i < written ? rows[(size_t)n * row + i] : -INFINITY;
    }
    return DSMI_OK;
}

extern "C" int dsmi_occupancy(dsmi_decoder* d, const float* probs, const int32_t* sizes, int B, int To, const int32_t* cand_clip,
                              const int32_t* targets, const int32_t* target_lens, int N, int L_stride, double* logp, double* occ,
                              double* tok, int32_t* status, void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    const int C = (int)d->labels.size();
    if (!probs || !cand_clip || !target_lens || !logp || !status || (L_stride > 0 && !targets)) {
        d->err = "bad occupancy arguments"; return DSMI_ERR_INVALID;
    }
    std::vector<int32_t> sz, tl, frames, base;
    int L_max = 0;
    uint64_t trellis = 0;
    if (int rc = occ_check(sizes, B, To, cand_clip, targets, target_lens, N, L_stride, C, d->blank, sz, tl, frames, base, &L_max, &trellis, d->err)) return rc;
    std::vector<int32_t> order(N);
    score_plan(cand_clip, frames.data(), target_lens, N, order.data());
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- the workspaces: sizes [B], order [N], clips [N], lens [N], bases [N], targets [N][L], then logp [N] doubles; the stored
    // trellises, forward and backward of `trellis` doubles each.  occ and tok are the caller's.
    const size_t NL = (size_t)N * L_stride, in_words = ((size_t)B + 4 * (size_t)N + NL + 1) & ~(size_t)1;
    if (int rc = reserve_all(d, d->occ_io, sizeof(int32_t) * (in_words + 2 * (size_t)N), &d->occ_ws, sizeof(double) * (2 * (size_t)trellis + 1))) return rc;
    int32_t* w_sz = d->occ_io.as<int32_t>(); int32_t* w_or = w_sz + B; int32_t* w_cl = w_or + N; int32_t* w_tl = w_cl + N;
    int32_t* w_ba = w_tl + N; int32_t* w_tg = w_ba + N;
    double* w_lp = reinterpret_cast<double*>(w_sz + in_words);
    DEC_HIP(d, hipMemcpyAsync(w_sz, sz.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_or, order.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_cl, cand_clip, sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_tl, tl.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemcpyAsync(w_ba, base.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice, s));
    if (NL) DEC_HIP(d, hipMemcpyAsync(w_tg, targets, sizeof(int32_t) * NL, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemsetAsync(w_lp, 0, sizeof(double) * N, s));
    OccArgs a{};
    a.probs = probs; a.T_out = To; a.C = C; a.blank = d->blank; a.N = N;
    a.sizes = w_sz; a.order = w_or; a.cand_clip = w_cl; a.tlen = w_tl; a.targets = w_tg; a.base = w_ba; a.L_stride = L_stride;
    a.S_max = 2 * L_max + 1; a.fwd = d->occ_ws.as<double>(); a.bwd = a.fwd + trellis;
    a.logp = w_lp; a.occ = occ; a.tok = L_stride > 0 ? tok : nullptr; a.both = a.occ || a.tok;
    DEC_HIP(d, launch_occ(a, s));
    std::vector<double> out(N);
    DEC_HIP(d, hipMemcpyAsync(out.data(), w_lp, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    for (int n = 0; n < N; ++n) {
        status[n] = tl[n] < 0 ? 1 : 0;
        logp[n] = tl[n] < 0 ? -INFINITY : out[n];
    }
    return DSMI_OK;
}

extern "C" int dsmi_grammar_plan(int B, int To, int n_nodes, int n_arcs, int64_t* info) {
    if (!info) return DSMI_ERR_INVALID;
    GrammarPlan plan;
    std::string err;
    if (int rc = grammar_plan(B, To, n_nodes, n_arcs, &plan, err)) return rc;
    info[0] = plan.node_stride; info[1] = plan.lds_bytes; info[2] = plan.bp_bytes;
    return DSMI_OK;
}

extern "C" int dsmi_grammar(dsmi_decoder* d, const float* probs, const int32_t* sizes, int B, int To, const dsmi_grammar_pool* pool,
                            const int32_t* clip_graph, int32_t* path_lens, int32_t* path_nodes, int32_t* path_spans, float* token_probs,
                            float* path_logp, int32_t* status, void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    const int C = (int)d->labels.size();
    if (!probs || !pool || !path_lens || !path_nodes || !path_spans || !token_probs || !path_logp || !status) {
        d->err = "bad grammar arguments"; return DSMI_ERR_INVALID;
    }
    const int K = pool->K;
    if (K > 0 && (!pool->node_off || !pool->labels || !pool->flags || !pool->arc_off || !pool->arc_pred || !pool->empty_ok)) {
        d->err = "grammar: a NULL array in the pool"; return DSMI_ERR_INVALID;
    }
    std::vector<int32_t> sz, cg;
    int n_nodes = 0, n_arcs = 0;
    if (int rc = grammar_check(sizes, B, To, K, pool->node_off, pool->labels, pool->weights, pool->flags, pool->arc_off, pool->arc_pred,
                               pool->empty_ok, clip_graph, C, d->blank, sz, cg, &n_nodes, &n_arcs, d->err)) return rc;
    GrammarPlan plan;
    if (int rc = grammar_plan(B, To, n_nodes, n_arcs, &plan, d->err)) return rc;
    // ---- the upload, int32 words: sizes [B], graphs [B], node_off [K + 1], empty_ok [K], node words [nodes], weights [nodes],
    // arc_off [nodes + 1], then the arcs as 16-bit words (the predecessor | kGrammarArcTok where the two labels differ)
    const size_t total = (size_t)pool->node_off[K], n_arc_all = (size_t)pool->arc_off[total], BT = (size_t)B * To;
    const size_t o_cg = B, o_no = o_cg + B, o_eo = o_no + K + 1, o_wd = o_eo + K, o_wt = o_wd + total, o_ao = o_wt + total, o_ar = o_ao + total + 1;
    const size_t in_words = o_ar + (n_arc_all + 1) / 2, out_words = 4 * BT + 3 * (size_t)B;
    std::vector<int32_t> up(in_words, 0);
    std::memcpy(up.data(), sz.data(), sizeof(int32_t) * B);
    std::memcpy(up.data() + o_cg, cg.data(), sizeof(int32_t) * B);
    std::memcpy(up.data() + o_no, pool->node_off, sizeof(int32_t) * (K + 1));
    std::memcpy(up.data() + o_eo, pool->empty_ok, sizeof(int32_t) * K);
    std::memcpy(up.data() + o_ao, pool->arc_off, sizeof(int32_t) * (total + 1));
    if (pool->weights && total) std::memcpy(up.data() + o_wt, pool->weights, sizeof(float) * total);
    uint16_t* arc16 = reinterpret_cast<uint16_t*>(up.data() + o_ar);
    for (int g = 0; g < K; ++g) {
        const int n0 = pool->node_off[g];
        for (int i = n0; i < pool->node_off[g + 1]; ++i) {
            up[o_wd + i] = pool->labels[i] | ((pool->flags[i] & DSMI_GRAMMAR_START) ? kGrammarStart : 0) | ((pool->flags[i] & DSMI_GRAMMAR_FINAL) ? kGrammarFinal : 0);
            for (int j = pool->arc_off[i]; j < pool->arc_off[i + 1]; ++j) {
                const int p = pool->arc_pred[j];
                arc16[j] = (uint16_t)(p | (pool->labels[n0 + p] != pool->labels[i] ? kGrammarArcTok : 0));
            }
        }
    }
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- workspaces: io = the upload, then path_lens [B], path_nodes [B][T], path_spans [B][T][2], token_probs [B][T], logp [B],
    // status [B]; the backpointers [B][T_out][node stride] of 16 bits
    if (int rc = reserve_all(d, d->gr_io, sizeof(int32_t) * (in_words + out_words), &d->gr_bp, (size_t)plan.bp_bytes)) return rc;
    int32_t* w = d->gr_io.as<int32_t>();
    int32_t* w_out = w + in_words;
    DEC_HIP(d, hipMemcpyAsync(w, up.data(), sizeof(int32_t) * in_words, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemsetAsync(w_out, 0, sizeof(int32_t) * out_words, s));
    GrammarArgs a{};
    a.probs = probs; a.T_out = To; a.C = C; a.blank = d->blank;
    a.sizes = w; a.clip_graph = w + o_cg; a.node_off = w + o_no; a.empty_ok = w + o_eo; a.words = w + o_wd;
    a.weights = reinterpret_cast<const float*>(w + o_wt); a.arc_off = w + o_ao; a.arc_words16 = reinterpret_cast<const uint16_t*>(w + o_ar);
    a.node_stride = (int)plan.node_stride; a.arc_words = (int)grammar_arc_words(n_arcs);
    a.bp = d->gr_bp.as<uint16_t>();
    a.path_lens = w_out; a.path_nodes = a.path_lens + B; a.path_spans = a.path_nodes + BT;
    a.token_probs = reinterpret_cast<float*>(a.path_spans + 2 * BT); a.path_logp = a.token_probs + BT;
    a.status = reinterpret_cast<int32_t*>(a.path_logp + B);
#ifdef DSMI_EXPERIMENTS
    // DSMI_DEBUG_GRAMMAR_TRACE=serial: the backtrace by one lane with a load per frame, measured and not adopted;
    // =none: no backtrace (timing only: what the forward pass costs alone)
    if (const char* form = exp_env("DSMI_DEBUG_GRAMMAR_TRACE")) a.trace_form = std::string(form) == "serial" ? 1 : std::string(form) == "none" ? 2 : 0;
#endif
    DEC_HIP(d, launch_grammar(a, B, s));
    // the results come back into an image of the call's own and reach the caller's arrays only when everything has succeeded
    std::vector<int32_t> out(out_words);
    DEC_HIP(d, hipMemcpyAsync(out.data(), w_out, sizeof(int32_t) * out_words, hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    std::memcpy(path_lens, out.data(), sizeof(int32_t) * B);
    std::memcpy(path_nodes, out.data() + B, sizeof(int32_t) * BT);
    std::memcpy(path_spans, out.data() + B + BT, sizeof(int32_t) * 2 * BT);
    std::memcpy(token_probs, out.data() + B + 3 * BT, sizeof(float) * BT);
    std::memcpy(path_logp, out.data() + B + 4 * BT, sizeof(float) * B);
    std::memcpy(status, out.data() + 2 * B + 4 * BT, sizeof(int32_t) * B);
    return DSMI_OK;
}

extern "C" int dsmi_grammar_posterior_plan(int B, int To, int n_nodes, int n_arcs, int64_t* info) {
    if (!info) return DSMI_ERR_INVALID;
    GrammarPostPlan plan;
    std::string err;
    if (int rc = grammar_post_plan(B, To, n_nodes, n_arcs, &plan, err)) return rc;
    info[0] = plan.node_stride; info[1] = plan.lds_bytes; info[2] = plan.ws_bytes;
    return DSMI_OK;
}

extern "C" int dsmi_grammar_posterior(dsmi_decoder* d, const float* probs, const int32_t* sizes, int B, int To, const dsmi_grammar_pool* pool,
                                      const int32_t* clip_graph, int N_stride, double* logp, double* visits, double* occ, int32_t* status,
                                      void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    const int C = (int)d->labels.size();
    if (!probs || !pool || !logp || !status) { d->err = "bad grammar posterior arguments"; return DSMI_ERR_INVALID; }
    const int K = pool->K;
    if (K > 0 && (!pool->node_off || !pool->labels || !pool->flags || !pool->arc_off || !pool->arc_pred || !pool->empty_ok)) {
        d->err = "grammar: a NULL array in the pool"; return DSMI_ERR_INVALID;
    }
    std::vector<int32_t> sz, cg;
    int n_nodes = 0, n_arcs = 0;
    GrammarPostPlan plan;
    if (int rc = grammar_post_check(sizes, B, To, K, pool->node_off, pool->labels, pool->weights, pool->flags, pool->arc_off, pool->arc_pred,
                                    pool->empty_ok, clip_graph, C, d->blank, visits != nullptr, N_stride, sz, cg, &n_nodes, &n_arcs, &plan, d->err))
        return rc;
    GrammarPostPack pk;
    grammar_post_pack(K, pool->node_off, pool->labels, pool->flags, pool->arc_off, pool->arc_pred, C, pk);
    // ---- the upload, int32 words: sizes [B], graphs [B], node_off [K + 1], empty_ok [K], start_off [K + 1], bucket_off [K][C + 1],
    // node words [nodes], weights [nodes], bucket_nodes [nodes], arc_off [nodes + 1], succ_off [nodes + 1]; then the 16-bit words:
    // arcs, successors, start nodes
    const size_t total = (size_t)pool->node_off[K], n_arc_all = (size_t)pool->arc_off[total], n_start = pk.start16.size();
    const size_t NS = (size_t)plan.node_stride, BT = (size_t)B * To;
    const size_t o_cg = B, o_no = o_cg + B, o_eo = o_no + K + 1, o_so = o_eo + K, o_bo = o_so + K + 1, o_wd = o_bo + (size_t)K * (C + 1);
    const size_t o_wt = o_wd + total, o_bn = o_wt + total, o_ao = o_bn + total, o_su = o_ao + total + 1, o_16 = o_su + total + 1;
    const size_t h_ar = 0, h_su = h_ar + n_arc_all, h_st = h_su + n_arc_all, n_half = h_st + n_start;
    const size_t in_words = (o_16 + (n_half + 1) / 2 + 1) & ~(size_t)1;      // (the doubles behind it on 8 bytes)
    std::vector<int32_t> up(in_words, 0);
    std::memcpy(up.data(), sz.data(), sizeof(int32_t) * B);
    std::memcpy(up.data() + o_cg, cg.data(), sizeof(int32_t) * B);
    std::memcpy(up.data() + o_no, pool->node_off, sizeof(int32_t) * (K + 1));
    std::memcpy(up.data() + o_eo, pool->empty_ok, sizeof(int32_t) * K);
    std::memcpy(up.data() + o_so, pk.start_off.data(), sizeof(int32_t) * (K + 1));
    std::memcpy(up.data() + o_bo, pk.bucket_off.data(), sizeof(int32_t) * pk.bucket_off.size());
    if (total) {
        std::memcpy(up.data() + o_wd, pk.words.data(), sizeof(int32_t) * total);
        if (pool->weights) std::memcpy(up.data() + o_wt, pool->weights, sizeof(float) * total);
        std::memcpy(up.data() + o_bn, pk.bucket_nodes.data(), sizeof(int32_t) * total);
    }
    std::memcpy(up.data() + o_ao, pool->arc_off, sizeof(int32_t) * (total + 1));
    std::memcpy(up.data() + o_su, pk.succ_off.data(), sizeof(int32_t) * (total + 1));
    uint16_t* half = reinterpret_cast<uint16_t*>(up.data() + o_16);
    if (n_arc_all) {
        std::memcpy(half + h_ar, pk.arc16.data(), sizeof(uint16_t) * n_arc_all);
        std::memcpy(half + h_su, pk.succ16.data(), sizeof(uint16_t) * n_arc_all);
    }
    if (n_start) std::memcpy(half + h_st, pk.start16.data(), sizeof(uint16_t) * n_start);
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- workspaces: io = the upload, then logp [B] and visits [B][node stride] doubles, then status [B]; ws = the stored
    // trellises, (tok, blk) pairs [B][T_out][node stride] forward and backward, then lead [B][T_out] forward and backward
    const size_t out_doubles = (size_t)B + (size_t)B * NS;
    if (int rc = reserve_all(d, d->gp_io, sizeof(int32_t) * (in_words + (size_t)B) + sizeof(double) * out_doubles, &d->gp_ws, (size_t)plan.ws_bytes)) return rc;
    int32_t* w = d->gp_io.as<int32_t>();
    double* w_lp = reinterpret_cast<double*>(w + in_words);
    int32_t* w_st = reinterpret_cast<int32_t*>(w_lp + out_doubles);
    DEC_HIP(d, hipMemcpyAsync(w, up.data(), sizeof(int32_t) * in_words, hipMemcpyHostToDevice, s));
    DEC_HIP(d, hipMemsetAsync(w_lp, 0, sizeof(double) * out_doubles + sizeof(int32_t) * B, s));
    const uint16_t* dh = reinterpret_cast<const uint16_t*>(w + o_16);
    GrammarPostArgs a{};
    a.probs = probs; a.B = B; a.T_out = To; a.C = C; a.blank = d->blank;
    a.sizes = w; a.clip_graph = w + o_cg; a.node_off = w + o_no; a.empty_ok = w + o_eo; a.start_off = w + o_so; a.bucket_off = w + o_bo;
    a.words = w + o_wd; a.weights = reinterpret_cast<const float*>(w + o_wt); a.bucket_nodes = w + o_bn; a.arc_off = w + o_ao; a.succ_off = w + o_su;
    a.arc16 = dh + h_ar; a.succ16 = dh + h_su; a.start16 = dh + h_st;
    a.node_stride = (int)NS; a.arc_words = (int)grammar_arc_words(n_arcs);
    a.fwd = d->gp_ws.as<double2>(); a.bwd = a.fwd + BT * NS;
    a.lead_fwd = reinterpret_cast<double*>(a.bwd + BT * NS); a.lead_bwd = a.lead_fwd + BT;
    a.logp = w_lp; a.status = w_st; a.visits = visits ? w_lp + B : nullptr; a.N_stride = (int)NS; a.occ = occ;
    a.both = a.visits || a.occ;
    DEC_HIP(d, launch_grammar_post(a, s));
    // the results come back into an image of the call's own and reach the caller's arrays only when everything has succeeded
    std::vector<double> out(visits ? out_doubles : (size_t)B);
    std::vector<int32_t> st(B);
    DEC_HIP(d, hipMemcpyAsync(out.data(), w_lp, sizeof(double) * out.size(), hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipMemcpyAsync(st.data(), w_st, sizeof(int32_t) * B, hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    std::memcpy(logp, out.data(), sizeof(double) * B);
    std::memcpy(status, st.data(), sizeof(int32_t) * B);
    if (visits) {
        for (int b = 0; b < B; ++b) {
            double* row = visits + (size_t)b * N_stride;
            const int N = pool->node_off[cg[b] + 1] - pool->node_off[cg[b]];
            for (int n = 0; n < N_stride; ++n) row[n] = n < N ? out[(size_t)B + (size_t)b * NS + n] : 0.0;
        }
    }
    return DSMI_OK;
}

extern "C" int dsmi_edit_plan(const int32_t* len_a, const int32_t* len_b, int N, int32_t* order, int32_t* seg) {
    if (!len_a || !len_b || !order || !seg || N <= 0) return DSMI_ERR_INVALID;
    for (int n = 0; n < N; ++n)
        if (len_a[n] < 0 || len_b[n] < 0) return DSMI_ERR_INVALID;
    return edit_plan(len_a, len_b, N, order, seg);
}

extern "C" int dsmi_edit_distance(dsmi_decoder* d, const int32_t* seqs, const int32_t* seq_lens, int M, int L_stride, const int32_t* pair_a,
                                  const int32_t* pair_b, int N, int32_t* counts, void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    if (!seq_lens || !pair_a || !pair_b || !counts || (L_stride > 0 && !seqs)) { d->err = "bad edit arguments"; return DSMI_ERR_INVALID; }
    if (int rc = edit_check(seq_lens, M, L_stride, pair_a, pair_b, N, d->err)) return rc;
    EditLaunch L;
    edit_pack(seqs, seq_lens, M, L_stride, pair_a, pair_b, N, L);
    std::vector<uint32_t> packed((size_t)L.n_launch);
    if (L.n_launch) {
        DEC_HIP(d, hipSetDevice(d->device));
        hipStream_t s = (hipStream_t)stream;
        // ---- the workspace: the upload (edit_pack: lens, pool, pairs in launch order, waves), then the packed results [n_launch]
        const size_t in_words = L.words.size();
        if (int rc = reserve_all(d, d->ed_io, sizeof(int32_t) * (in_words + (size_t)L.n_launch))) return rc;
        int32_t* w = d->ed_io.as<int32_t>();
        DEC_HIP(d, hipMemcpyAsync(w, L.words.data(), sizeof(int32_t) * in_words, hipMemcpyHostToDevice, s));
        EditArgs a{};
        a.lens = w; a.pool = w + L.off_pool; a.L_stride = L_stride; a.pair_a = w + L.off_a; a.pair_b = w + L.off_b;
        a.waves = w + L.off_waves; a.n_waves = L.n_waves; a.col_words = L.col_words;
        a.packed = reinterpret_cast<uint32_t*>(w + in_words);
        DEC_HIP(d, launch_edit(a, s));
        DEC_HIP(d, hipMemcpyAsync(packed.data(), a.packed, sizeof(uint32_t) * packed.size(), hipMemcpyDeviceToHost, s));
        DEC_HIP(d, hipStreamSynchronize(s));
    }
    edit_unpack(L, packed.data(), seq_lens, pair_a, pair_b, N, counts);
    return DSMI_OK;
}

extern "C" int dsmi_lm_score_plan(const int32_t* seqs, const int32_t* seq_lens, int M, int L_stride, int space, int32_t* n_words,
                                  int32_t* word_first, int32_t* word_len, int W_stride) {
    if (!seq_lens || !n_words || M <= 0 || L_stride < 0 || W_stride < 0 || (L_stride > 0 && !seqs) || (W_stride > 0 && (!word_first || !word_len)))
        return DSMI_ERR_INVALID;
    return lm_score_plan(seqs, seq_lens, M, L_stride, space, n_words, word_first, word_len, W_stride);
}

extern "C" int dsmi_lm_score(dsmi_decoder* d, const int32_t* seqs, const int32_t* seq_lens, int M, int L_stride, double* lm_ln, int32_t* n_words,
                             int32_t* n_oov, int32_t* n_terms, double* terms, int W_stride, void* stream) {
    if (!d) return DSMI_ERR_INVALID;
    if (!seq_lens || !lm_ln || !n_words || !n_oov || !n_terms || (L_stride > 0 && !seqs)) { d->err = "bad lm_score arguments"; return DSMI_ERR_INVALID; }
    const int C = (int)d->labels.size();
    if (int rc = lm_score_check(d->has_lm, seqs, seq_lens, M, L_stride, C, d->blank, d->space, terms != nullptr, W_stride, d->err)) return rc;
    LmScoreLaunch L;
    lm_score_pack(seqs, seq_lens, M, L_stride, d->space, L);
    DEC_HIP(d, hipSetDevice(d->device));
    hipStream_t s = (hipStream_t)stream;
    // ---- the workspace: the upload (lm_score_pack), then on 8 bytes lm_ln [M] doubles, terms [n_slots] doubles (when wanted),
    // n_oov [M] words: one copy up, one launch, one copy down
    const size_t in_words = (L.words.size() + 1) & ~(size_t)1, n_terms_out = terms ? L.n_slots : 0;
    const size_t out_bytes = sizeof(double) * ((size_t)M + n_terms_out) + sizeof(int32_t) * (size_t)M;
    if (int rc = reserve_all(d, d->lm_io, sizeof(int32_t) * in_words + out_bytes)) return rc;
    int32_t* w = d->lm_io.as<int32_t>();
    DEC_HIP(d, hipMemcpyAsync(w, L.words.data(), sizeof(int32_t) * L.words.size(), hipMemcpyHostToDevice, s));
    LmScoreArgs a{};
    a.lm = d->lm.view(); a.lm.tab = d->d_tab; a.lm.klm.base = d->d_klm; a.trie_next = d->d_next; a.trie_word = d->d_word;
    a.C = C; a.order = d->lm.order; a.unk = d->lm.unk; a.bos = d->lm.bos; a.eos = d->lm.eos;
    a.tok = w; a.slot_first = w + L.off_first; a.slot_len = w + L.off_len; a.slot_sent = w + L.off_sent;
    a.sent_slot = w + L.off_sent_slot; a.pack_sent = w + L.off_pack;
    a.lm_ln = reinterpret_cast<double*>(w + in_words); a.terms = terms ? a.lm_ln + M : nullptr;
    a.n_oov = reinterpret_cast<int32_t*>(a.lm_ln + M + n_terms_out);
    DEC_HIP(d, launch_lm_score(a, L.n_packs, s));
    // the results come back into an image of the call's own and reach the caller's arrays only when everything has succeeded
    std::vector<double> out(out_bytes / sizeof(double) + 1);
    DEC_HIP(d, hipMemcpyAsync(out.data(), a.lm_ln, out_bytes, hipMemcpyDeviceToHost, s));
    DEC_HIP(d, hipStreamSynchronize(s));
    lm_score_unpack(L, M, out.data(), out.data() + M, reinterpret_cast<const int32_t*>(out.data() + M + n_terms_out), lm_ln, n_words, n_oov,
                    n_terms, terms, W_stride);
    return DSMI_OK;
}
