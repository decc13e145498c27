// LM sentence scoring (lmscore.hip): for each of M known sentences (label ids) its words through the dictionary trie, the n-gram
// term of every window of HostLM::sent_ln, their sum in window order and the number of out-of-vocabulary words.  Launched by
// dsmi_lm_score (ctc_tools.hip), which checks every argument and packs whole sentences into workgroups with lm_score_pack
// (lm_score_host.h).  lm_window_ln is the one function behind a term, on the device and on the host (dsmi_lm_sentence_ln).
#pragma once
#include "common.h"
#include "lm.h"
#include "lm_score_host.h"

namespace dsmi {

// Scorer::get_log_cond_prob of one window of `order` word ids (-1 = out of vocabulary): natural log, float32 back-off sum, one
// IEEE double division.
__host__ __device__ inline double lm_window_ln(const LmView& v, const int32_t* win, int order, int32_t unk) {
    for (int j = 0; j < order; ++j)
        if (win[j] < 0 || win[j] == unk) return kOovScore;
    return (double)lm_cond_log10(v, win, order - 1, win[order - 1], unk) / (double)kLog10E;
}

// Member k of the sentence s = [<s>] * (order - 1) + slots, where the slots are a sentence's word ids and </s> (no words: <s>, </s>)
__host__ __device__ inline int32_t lm_sentence_at(const int32_t* slots, int k, int order, int32_t bos) { return k < order - 1 ? bos : slots[k - (order - 1)]; }

// HostLM::sent_ln with the terms exposed: terms [n + 1] (2 for n = 0), or null.  Returns their sum in window order.
inline double lm_sentence_ln(const HostLM& lm, const int32_t* word_ids, int n, double* terms) {
    std::vector<int32_t> slots(word_ids, word_ids + n);
    if (n == 0) slots.push_back(lm.bos);
    slots.push_back(lm.eos);
    const LmView v = lm.view();
    double sum = 0.0;
    for (int t = 0; t < (int)slots.size(); ++t) {
        int32_t win[kMaxOrder];
        for (int j = 0; j < lm.order; ++j) win[j] = lm_sentence_at(slots.data(), t + j, lm.order, lm.bos);
        const double term = lm_window_ln(v, win, lm.order, lm.unk);
        if (terms) terms[t] = term;
        sum += term;
    }
    return sum;
}

struct LmScoreArgs {
    LmView lm;                          // device view of the tables
    const int32_t *trie_next, *trie_word;
    int C, order;
    int32_t unk, bos, eos;
    const int32_t* tok;                 // the upload of lm_score_pack
    const int32_t *slot_first, *slot_len, *slot_sent, *sent_slot, *pack_sent;
    double* lm_ln;                      // [M] in launch order
    double* terms;                      // [n_slots], or null
    int32_t* n_oov;                     // [M] in launch order
};

hipError_t launch_lm_score(const LmScoreArgs& a, int n_packs, hipStream_t s);

}  // namespace dsmi
