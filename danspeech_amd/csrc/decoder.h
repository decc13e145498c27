// The handle behind dsmi_decoder*, shared by decoder.hip (its life, greedy, beam search, the LM) and ctc_tools.hip (forced
// alignment of clips and of one long recording, phrase search, transcript scoring, token confidence, occupancy, grammar decoding, edit distance, LM sentence scoring).
#pragma once
#include "common.h"
#include "lm.h"

#include <mutex>

// A device buffer grown on demand.  reserve() allocates nothing when the capacity suffices; growing frees the old buffer, which
// work in flight may still read, so the caller synchronises the device before the first reserve() of a call that grows.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;                      // bytes
    bool holds(size_t bytes) const { return bytes <= cap; }
    hipError_t reserve(size_t bytes) {
        if (holds(bytes)) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes; else p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

struct dsmi_decoder {
    int device = 0;
    std::vector<std::string> labels;
    int blank = 0, space = -2;
    std::string err;
    // greedy scratch
    size_t greedy_cap = 0;
    int32_t *g_raw = nullptr, *g_ids = nullptr, *g_offs = nullptr, *g_nout = nullptr, *g_sizes = nullptr;
    // dsmi_greedy_enqueue / _collect: pinned host images of the results and of the sizes, the event behind the last copy
    int32_t* gh = nullptr; size_t gh_cap = 0; hipEvent_t g_done = nullptr; bool greedy_pending = false; int gp_B = 0, gp_T = 0;
    // LM
    bool has_lm = false;
    dsmi::HostLM lm;
    double alpha = 0, beta = 0;
    dsmi::LmEntry* d_tab = nullptr; int32_t *d_next = nullptr, *d_word = nullptr;
    unsigned char* d_klm = nullptr;      // device copy of a KenLM probing binary's search memory
    // beam workspace
    size_t ws_bytes = 0;
    unsigned char* ws = nullptr;
    // the beam search between dsmi_beam_enqueue and dsmi_beam_collect: geometry, pinned copies of its outputs, completion event
    bool beam_pending = false;
    int pb_B = 0, pb_To = 0, pb_beam = 0;
    size_t pb_out = 0, pb_out_bytes = 0; hipStream_t pb_stream = nullptr;
    int32_t stats[4] = {0, 0, 0, 0};      // of the last collected search: see dsmi_decoder_beam_stats
    uint64_t stamps[64 * 8] = {0};
    int32_t* pin_sz = nullptr; size_t pin_sz_cap = 0;
    unsigned char* pin = nullptr; size_t pin_bytes = 0;
    hipEvent_t beam_done = nullptr;
    hipStream_t copy_stream = nullptr;      // the collect's device-to-host copies: the device's collect stream (collect_stream)
    // resumable searches (dsmi_beam_stream): bumped by every dsmi_decoder_set_lm, so that a stream can tell that the scorer it was
    // created with is gone; the launch table and result staging of dsmi_beam_stream_advance_many (not the offline workspace above)
    uint64_t lm_gen = 0;
    std::mutex bs_mu;
    unsigned char *bs_dev = nullptr, *bs_pin = nullptr; size_t bs_dev_cap = 0, bs_pin_cap = 0;
    // ctc_tools.hip -- dsmi_align: inputs and outputs of the launch (int32 words), backpointers [B][T_out][S_stride] bytes
    DevBuf al_io, al_bp;
    // dsmi_align_long: targets and outputs of the call (int32 words), the checkpoint rows [frame tiles + 1][S] floats
    DevBuf along_io, along_rows;
    // dsmi_spot: inputs and hits of the launch (int32 words), the E and ST tracks 2 x [B][K][T_out] words
    DevBuf sp_io, sp_tr;
    // dsmi_score: inputs of the launch (int32 words) and, behind them on 8 bytes, the results [N] doubles
    DevBuf sc_io;
    // dsmi_alternatives: inputs of the launch and logp [N] as dsmi_score's, the results [N][L_stride][n_labels] doubles, the
    // stored trellises (doubles: forward pairs, backward, backward pair sums)
    DevBuf alt_io, alt_out, alt_ws;
    // dsmi_occupancy: inputs of the launch and logp [N] as dsmi_score's, the two stored trellises (doubles: forward, backward)
    DevBuf occ_io, occ_ws;
    // dsmi_grammar: the upload and the results of the launch (int32 words), the backpointers [B][T_out][node stride] of 16 bits
    DevBuf gr_io, gr_bp;
    // dsmi_grammar_posterior: the upload and, behind it on 8 bytes, logp, visits and the status; the two stored trellises (doubles)
    DevBuf gp_io, gp_ws;
    // dsmi_edit_distance: the upload of the launch (int32 words: lens, pool, pairs, waves) and, behind it, the packed results
    DevBuf ed_io;
    // dsmi_lm_score: the upload of the launch (int32 words: lm_score_pack) and, behind it on 8 bytes, the results
    DevBuf lm_io;
};

#define DEC_HIP(d, expr)                                                                  \
    do {                                                                                  \
        hipError_t e_ = (expr);                                                           \
        if (e_ != hipSuccess) { (d)->err = std::string(#expr) + ": " + hipGetErrorString(e_); return DSMI_ERR_HIP; } \
    } while (0)
