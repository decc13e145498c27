// The host half of LM sentence scoring (dsmi_lm_score, dsmi_lm_score_plan: ctc_tools.hip; the kernel: lmscore.hip): the check of
// everything a caller hands in, the word segmentation, the packing of whole sentences into workgroups and of the upload, and the
// unpacking of the results.  No HIP: a plain C++ compiler takes it, and tools/asan/host_fuzz.cpp (lmscore) runs it under ASan +
// UBSan on exactly sized arrays.  The check returns DSMI_OK or a DSMI_ERR_* code with the message in `err`; what the numbers
// alone refuse is refused before any array is read.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dsmi.h"

namespace dsmi {

constexpr uint64_t kLmScorePoolCap = (uint64_t)1 << 24;      // M * L_stride
constexpr int kLmScoreThreads = 256;
// A sentence of n words takes n + 1 slots, one per window: its words, then </s> (no words: <s>, </s>).  Words are separated by
// at least one space, so a row of DSMI_LM_SCORE_MAX_TOKENS tokens holds at most half as many words.
constexpr int kLmScoreMaxSlots = DSMI_LM_SCORE_MAX_TOKENS / 2 + 1;
constexpr int32_t kLmSlotEos = -1, kLmSlotBos = -2;          // a slot's length word when it holds no word of the row

// The words of one row: maximal runs of tokens other than `space` among row[0 .. len); emit(first, length) for each in order.
// Nothing past len is read.  Returns their number.
template <typename Emit> inline int lm_score_words(const int32_t* row, int len, int space, Emit emit) {
    int n = 0;
    for (int k = 0; k < len;) {
        if (row[k] == space) { ++k; continue; }
        const int first = k;
        while (k < len && row[k] != space) ++k;
        emit(first, k - first);
        ++n;
    }
    return n;
}

inline int lm_score_terms(int n_words) { return n_words > 0 ? n_words + 1 : 2; }

// row m of the pool (which may be null when it has no column)
inline const int32_t* lm_score_row(const int32_t* seqs, int m, int L_stride) { return L_stride > 0 ? seqs + (size_t)m * (size_t)L_stride : seqs; }

// dsmi_lm_score_plan behind its null-pointer test: n_words [M], word_first / word_len [M][W_stride] (rows past a row's count are
// left alone).  Returns the largest n_words, or DSMI_ERR_INVALID with nothing written for a length outside 0 .. L_stride or a row
// of more than W_stride words.
inline int lm_score_plan(const int32_t* seqs, const int32_t* seq_lens, int M, int L_stride, int space, int32_t* n_words, int32_t* word_first,
                         int32_t* word_len, int W_stride) {
    int most = 0;
    for (int m = 0; m < M; ++m) {
        if (seq_lens[m] < 0 || seq_lens[m] > L_stride) return DSMI_ERR_INVALID;
        const int n = lm_score_words(lm_score_row(seqs, m, L_stride), seq_lens[m], space, [](int, int) {});
        if (n > W_stride) return DSMI_ERR_INVALID;
        most = std::max(most, n);
    }
    for (int m = 0; m < M; ++m) {
        int32_t* wf = word_first + (size_t)m * (size_t)W_stride;
        int32_t* wl = word_len + (size_t)m * (size_t)W_stride;
        int at = 0;
        n_words[m] = lm_score_words(lm_score_row(seqs, m, L_stride), seq_lens[m], space, [&](int first, int length) { wf[at] = first; wl[at] = length; ++at; });
    }
    return most;
}

inline int lm_score_refuse(std::string& err, int code, const std::string& msg) { err = msg; return code; }

// The arguments of dsmi_lm_score behind its null-pointer test.  `terms`: the caller takes the per-window terms, W_stride wide.
inline int lm_score_check(bool has_lm, const int32_t* seqs, const int32_t* seq_lens, int M, int L_stride, int n_labels, int blank, int space,
                          bool terms, int W_stride, std::string& err) {
    if (!has_lm) return lm_score_refuse(err, DSMI_ERR_INVALID, "lm_score: the decoder has no language model");
    if (M <= 0) return lm_score_refuse(err, DSMI_ERR_INVALID, "lm_score: M must be positive");
    if (L_stride < 0) return lm_score_refuse(err, DSMI_ERR_INVALID, "lm_score: negative L_stride");
    if (L_stride > DSMI_LM_SCORE_MAX_TOKENS)
        return lm_score_refuse(err, DSMI_ERR_CAPACITY, "lm_score: L_stride " + std::to_string(L_stride) + " exceeds DSMI_LM_SCORE_MAX_TOKENS (" + std::to_string(DSMI_LM_SCORE_MAX_TOKENS) + ")");
    if ((uint64_t)M * (uint64_t)L_stride > kLmScorePoolCap) return lm_score_refuse(err, DSMI_ERR_CAPACITY, "lm_score: M * L_stride exceeds 2^24");
    int most = 0;
    for (int m = 0; m < M; ++m) {
        if (seq_lens[m] < 0 || seq_lens[m] > L_stride)
            return lm_score_refuse(err, DSMI_ERR_INVALID, "lm_score: sequence " + std::to_string(m) + ": length outside 0 .. L_stride");
        const int32_t* row = lm_score_row(seqs, m, L_stride);
        for (int k = 0; k < seq_lens[m]; ++k)
            if (row[k] < 0 || row[k] >= n_labels || row[k] == blank)
                return lm_score_refuse(err, DSMI_ERR_INVALID, "lm_score: sequence " + std::to_string(m) + ": token " + std::to_string(k) + " is the blank or outside 0 .. n_labels-1");
        most = std::max(most, lm_score_words(row, seq_lens[m], space, [](int, int) {}));
    }
    if (terms && W_stride < lm_score_terms(most))
        return lm_score_refuse(err, DSMI_ERR_CAPACITY, "lm_score: W_stride " + std::to_string(W_stride) + " is below the largest n_terms (" + std::to_string(lm_score_terms(most)) + ")");
    return DSMI_OK;
}

// One call's launch.  The sentences in launch order (`order`: by n_words descending, then by index), each with one slot per
// window; a pack -- one workgroup -- takes consecutive whole sentences: as many as fit kLmScoreThreads slots, or one longer
// sentence alone.  The int32 words of the upload:
//     tok [n_tok]           the tokens of every word, back to back (no spaces, nothing past a row's length)
//     slot_first [n_slots]  where a slot's word begins in tok
//     slot_len [n_slots]    its tokens, or kLmSlotEos / kLmSlotBos
//     slot_sent [n_slots]   the sentence (launch order) a slot belongs to
//     sent_slot [M + 1]     the first slot of each sentence
//     pack_sent [n_packs + 1]  the first sentence of each pack
// behind which the device keeps the results: lm_ln [M] doubles, terms [n_slots] doubles (when wanted), n_oov [M] words.
struct LmScoreLaunch {
    std::vector<int32_t> order, n_words, words;
    int n_packs = 0;
    size_t n_tok = 0, n_slots = 0;
    size_t off_first = 0, off_len = 0, off_sent = 0, off_sent_slot = 0, off_pack = 0;
};

// Of a checked call.
inline void lm_score_pack(const int32_t* seqs, const int32_t* seq_lens, int M, int L_stride, int space, LmScoreLaunch& out) {
    out.n_words.assign((size_t)M, 0);
    size_t n_tok = 0, n_slots = 0;
    for (int m = 0; m < M; ++m) {
        out.n_words[(size_t)m] = lm_score_words(lm_score_row(seqs, m, L_stride), seq_lens[m], space, [&](int, int length) { n_tok += (size_t)length; });
        n_slots += (size_t)lm_score_terms(out.n_words[(size_t)m]);
    }
    // by n_words descending, then by index: one stable counting pass (n_words <= kLmScoreMaxSlots - 1)
    out.order.assign((size_t)M, 0);
    {
        std::vector<int32_t> count((size_t)kLmScoreMaxSlots + 1, 0);
        for (int m = 0; m < M; ++m) ++count[(size_t)(kLmScoreMaxSlots - 1 - out.n_words[(size_t)m]) + 1];
        for (int b = 0; b < kLmScoreMaxSlots; ++b) count[(size_t)b + 1] += count[(size_t)b];
        for (int m = 0; m < M; ++m) out.order[(size_t)count[(size_t)(kLmScoreMaxSlots - 1 - out.n_words[(size_t)m])]++] = m;
    }
    std::vector<int32_t> pack_sent;
    for (int s = 0, room = 0; s < M; ++s) {
        const int need = lm_score_terms(out.n_words[(size_t)out.order[(size_t)s]]);
        if (need > room) { pack_sent.push_back(s); room = kLmScoreThreads; }
        room = need > room ? 0 : room - need;
    }
    out.n_packs = (int)pack_sent.size();
    pack_sent.push_back(M);
    out.n_tok = n_tok; out.n_slots = n_slots;
    out.off_first = n_tok; out.off_len = out.off_first + n_slots; out.off_sent = out.off_len + n_slots;
    out.off_sent_slot = out.off_sent + n_slots; out.off_pack = out.off_sent_slot + (size_t)M + 1;
    out.words.assign(out.off_pack + pack_sent.size(), 0);
    int32_t* w = out.words.data();
    size_t tok = 0, slot = 0;
    for (int s = 0; s < M; ++s) {
        const int m = out.order[(size_t)s];
        const int32_t* row = lm_score_row(seqs, m, L_stride);
        w[out.off_sent_slot + (size_t)s] = (int32_t)slot;
        auto put = [&](int32_t first, int32_t length) { w[out.off_first + slot] = first; w[out.off_len + slot] = length; w[out.off_sent + slot] = s; ++slot; };
        lm_score_words(row, seq_lens[m], space, [&](int first, int length) {
            put((int32_t)tok, length);
            for (int k = 0; k < length; ++k) w[tok + (size_t)k] = row[first + k];      // (words are short: no call)
            tok += (size_t)length;
        });
        if (out.n_words[(size_t)m] == 0) put(0, kLmSlotBos);
        put(0, kLmSlotEos);
    }
    w[out.off_sent_slot + (size_t)M] = (int32_t)slot;
    std::copy(pack_sent.begin(), pack_sent.end(), w + out.off_pack);
}

// The caller's arrays of a checked, packed call from the kernel's results in launch order; terms may be null.
inline void lm_score_unpack(const LmScoreLaunch& L, int M, const double* lm_ln_dev, const double* terms_dev, const int32_t* n_oov_dev, double* lm_ln,
                            int32_t* n_words, int32_t* n_oov, int32_t* n_terms, double* terms, int W_stride) {
    const int32_t* sent_slot = L.words.data() + L.off_sent_slot;
    for (int s = 0; s < M; ++s) {
        const int m = L.order[(size_t)s], nt = lm_score_terms(L.n_words[(size_t)m]);
        lm_ln[m] = lm_ln_dev[s];
        n_words[m] = L.n_words[(size_t)m];
        n_oov[m] = n_oov_dev[s];
        n_terms[m] = nt;
        if (terms) std::copy(terms_dev + sent_slot[s], terms_dev + sent_slot[s] + nt, terms + (size_t)m * (size_t)W_stride);
    }
}

}  // namespace dsmi
