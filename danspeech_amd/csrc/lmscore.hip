// LM sentence scoring on the GPU (gfx950): the n-gram score of known sentences, window for window what HostLM::sent_ln computes
// (the contract: include/dsmi.h).  For a known sentence every word's trie walk and every window's back-off chain is independent
// of the others -- the opposite of the beam search, where both are carried per beam entry -- so the work, which is nothing but
// dependent loads, is laid out wide:
//     walk     one thread per slot: the word's labels down the dictionary trie (trie_next[node * C + label], one dependent 4-byte
//              load per label), its word id (-1 = no such word) to LDS; the </s> and <s> slots take their ids;
//     windows  one thread per slot again: the window that ends in the slot, from LDS, through lm_window_ln (at most 2 * order
//              dependent probes of the table, either kind), the term to LDS and, when wanted, to global memory;
//     sums     one thread per sentence: its terms in window order in float64, its words with id -1 counted.
// One workgroup takes a pack of whole sentences (lm_score_pack, lm_score_host.h): up to kLmScoreThreads slots, or one longer
// sentence alone, which loops.  What a sentence computes depends on its own tokens only; the packing decides where.  Two
// barriers, plain vector stores, no atomics.  ORDER is a template parameter so that the window and the n-gram of lm_cond_log10
// stay in registers.
#include "lmscore.h"

namespace dsmi {

template <int ORDER> __global__ void __launch_bounds__(kLmScoreThreads) lm_score_kernel(LmScoreArgs a) {
    __shared__ int32_t wid[kLmScoreMaxSlots];
    __shared__ double term[kLmScoreMaxSlots];
    const int tid = threadIdx.x;
    const int sent0 = a.pack_sent[blockIdx.x], sent1 = a.pack_sent[blockIdx.x + 1];
    const int slot0 = a.sent_slot[sent0], n_slots = min(a.sent_slot[sent1] - slot0, kLmScoreMaxSlots);

    for (int i = tid; i < n_slots; i += kLmScoreThreads) {
        const int len = a.slot_len[slot0 + i];
        int32_t id;
        if (len < 0) {
            id = len == kLmSlotEos ? a.eos : a.bos;
        } else {
            const int32_t* t = a.tok + a.slot_first[slot0 + i];
            int32_t node = 0;
            for (int k = 0; k < len && node >= 0; ++k) node = a.trie_next[(size_t)node * a.C + t[k]];
            id = node >= 0 ? a.trie_word[node] : -1;
        }
        wid[i] = id;
    }
    __syncthreads();

    for (int i = tid; i < n_slots; i += kLmScoreThreads) {
        const int at = a.sent_slot[a.slot_sent[slot0 + i]] - slot0;      // the sentence's first slot; the window ends in slot i
        int32_t win[ORDER];
#pragma unroll
        for (int j = 0; j < ORDER; ++j) {
            const int k = i - (ORDER - 1) + j;
            win[j] = k < at ? a.bos : wid[k];
        }
        const double v = lm_window_ln(a.lm, win, ORDER, a.unk);
        term[i] = v;
        if (a.terms) a.terms[slot0 + i] = v;
    }
    __syncthreads();

    for (int s = sent0 + tid; s < sent1; s += kLmScoreThreads) {
        const int at = a.sent_slot[s] - slot0, n = a.sent_slot[s + 1] - a.sent_slot[s];
        double sum = 0.0;
        int oov = 0;
        for (int t = 0; t < n; ++t) {
            sum += term[at + t];
            oov += wid[at + t] == -1;       // (<s> and </s> have ids)
        }
        a.lm_ln[s] = sum;
        a.n_oov[s] = oov;
    }
}

template <int ORDER> static hipError_t launch_order(const LmScoreArgs& a, int n_packs, hipStream_t s) {
    hipLaunchKernelGGL(lm_score_kernel<ORDER>, dim3(n_packs), dim3(kLmScoreThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_lm_score(const LmScoreArgs& a, int n_packs, hipStream_t s) {
    static_assert(kMaxOrder == 6, "one instantiation per order");
    switch (a.order) {
        case 1: return launch_order<1>(a, n_packs, s);
        case 2: return launch_order<2>(a, n_packs, s);
        case 3: return launch_order<3>(a, n_packs, s);
        case 4: return launch_order<4>(a, n_packs, s);
        case 5: return launch_order<5>(a, n_packs, s);
        case 6: return launch_order<6>(a, n_packs, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace dsmi
