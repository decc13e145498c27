// The host half of the batched edit distance (dsmi_edit_distance, dsmi_edit_plan: ctc_tools.hip; the kernel: edit.hip): the check
// of everything a caller hands in, the launch order and the lane segments of the pairs, the packing of the upload and the
// unpacking of the results.  No HIP: a plain C++ compiler takes it, and tools/asan/host_fuzz.cpp (editcheck) runs it under ASan +
// UBSan on exactly sized arrays.  The check returns DSMI_OK or a DSMI_ERR_* code with the message in `err`; what the numbers
// alone refuse is refused before any array is read.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dsmi.h"

namespace dsmi {

constexpr uint32_t kEditIndel = 0x10000u;      // a deletion or an insertion: distance + 1
constexpr uint32_t kEditSub = 0x10001u;        // a substitution: distance + 1, substitutions + 1
constexpr uint64_t kEditPoolCap = (uint64_t)1 << 24;      // M * L_stride: the pool's upload, kept on the handle
constexpr uint64_t kEditPairCap = (uint64_t)1 << 24;      // N: a wave's word keeps the launch index of its first pair in 24 bits
constexpr int kEditWavesPerBlock = 4;

// a wave's word: the launch index of its first pair, then
constexpr int kEditSegShift = 24;       // 2 bits: 0 = four segments of 16 lanes, 1 = two of 32, 2 = one of 64
constexpr int kEditCountShift = 26;     // 3 bits: the pairs the wave holds, 1 .. 64 / seg

inline int edit_seg(int len_b) { return len_b <= 16 ? 16 : (len_b <= 32 ? 32 : 64); }
inline int64_t edit_work(int len_a, int len_b) { const int seg = edit_seg(len_b); return (int64_t)((len_b + 63) / 64) * ((int64_t)len_a + seg); }

// seg[n] for every pair; order = the pairs with both lengths > 0, by seg ascending, then by work descending, then by index.
// Every length is >= 0.  Returns the number of pairs in order.
inline int edit_plan(const int32_t* len_a, const int32_t* len_b, int N, int32_t* order, int32_t* seg) {
    int n_launch = 0;
    bool small = true;                   // every length within DSMI_EDIT_MAX_TOKENS: the work fits 19 bits
    for (int n = 0; n < N; ++n) {
        seg[n] = edit_seg(len_b[n]);
        if (len_a[n] > 0 && len_b[n] > 0) order[n_launch++] = n;
        small = small && len_a[n] <= DSMI_EDIT_MAX_TOKENS && len_b[n] <= DSMI_EDIT_MAX_TOKENS;
    }
    if (!small) {                        // (dsmi_edit_plan takes any lengths; dsmi_edit_distance never comes here)
        std::sort(order, order + n_launch, [&](int32_t x, int32_t y) {
            if (seg[x] != seg[y]) return seg[x] < seg[y];
            const int64_t wx = edit_work(len_a[x], len_b[x]), wy = edit_work(len_a[y], len_b[y]);
            if (wx != wy) return wx > wy;
            return x < y;
        });
        return n_launch;
    }
    // order holds the pairs by index ascending: two stable counting passes over the 22-bit key seg code : (2^19 - 1 - work), 11
    // bits each, leave them by seg, then work descending, then index -- in time linear in N (tens of thousands of pairs per call)
    constexpr int kBits = 11, kBuckets = 1 << kBits;
    static_assert((int64_t)(DSMI_EDIT_MAX_TOKENS / 64) * (DSMI_EDIT_MAX_TOKENS + 64) < ((int64_t)1 << 19), "the work fits 19 bits");
    std::vector<uint32_t> key((size_t)n_launch), key2((size_t)n_launch);
    std::vector<int32_t> tmp((size_t)n_launch);
    for (int i = 0; i < n_launch; ++i) {
        const int32_t n = order[i];
        const uint32_t code = seg[n] == 16 ? 0u : (seg[n] == 32 ? 1u : 2u);
        key[(size_t)i] = code << 19 | (uint32_t)(((1 << 19) - 1) - edit_work(len_a[n], len_b[n]));
    }
    for (int pass = 0; pass < 2; ++pass) {
        const int shift = pass * kBits;
        int32_t* src = pass ? tmp.data() : order;
        int32_t* dst = pass ? order : tmp.data();
        const uint32_t* ks = pass ? key2.data() : key.data();
        uint32_t* kd = pass ? key.data() : key2.data();
        int count[kBuckets + 1] = {0};
        for (int i = 0; i < n_launch; ++i) ++count[((ks[i] >> shift) & (kBuckets - 1)) + 1];
        for (int b = 0; b < kBuckets; ++b) count[b + 1] += count[b];
        for (int i = 0; i < n_launch; ++i) {
            const int at = count[(ks[i] >> shift) & (kBuckets - 1)]++;
            dst[at] = src[i]; kd[at] = ks[i];
        }
    }
    return n_launch;
}

inline int edit_refuse(std::string& err, int code, const std::string& msg) { err = msg; return code; }

// The arguments of dsmi_edit_distance behind its null-pointer test (seqs itself is never read here: tokens are any int32).
inline int edit_check(const int32_t* seq_lens, int M, int L_stride, const int32_t* pair_a, const int32_t* pair_b, int N, std::string& err) {
    if (M <= 0 || N <= 0) return edit_refuse(err, DSMI_ERR_INVALID, "edit: M and N must be positive");
    if (L_stride < 0) return edit_refuse(err, DSMI_ERR_INVALID, "edit: negative L_stride");
    if (L_stride > DSMI_EDIT_MAX_TOKENS)
        return edit_refuse(err, DSMI_ERR_CAPACITY, "edit: L_stride " + std::to_string(L_stride) + " exceeds DSMI_EDIT_MAX_TOKENS (" + std::to_string(DSMI_EDIT_MAX_TOKENS) + ")");
    if ((uint64_t)M * (uint64_t)L_stride > kEditPoolCap) return edit_refuse(err, DSMI_ERR_CAPACITY, "edit: M * L_stride exceeds 2^24");
    if ((uint64_t)N > kEditPairCap) return edit_refuse(err, DSMI_ERR_CAPACITY, "edit: N exceeds 2^24");
    for (int m = 0; m < M; ++m)
        if (seq_lens[m] < 0 || seq_lens[m] > L_stride)
            return edit_refuse(err, DSMI_ERR_INVALID, "edit: sequence " + std::to_string(m) + ": length outside 0 .. L_stride");
    for (int n = 0; n < N; ++n)
        if (pair_a[n] < 0 || pair_a[n] >= M || pair_b[n] < 0 || pair_b[n] >= M)
            return edit_refuse(err, DSMI_ERR_INVALID, "edit: pair " + std::to_string(n) + ": sequence index outside 0 .. M-1");
    return DSMI_OK;
}

// One call's launch: the order of its pairs, and the int32 words of the upload
//     lens [M], pool [M][L_stride], a [n_launch], b [n_launch] (pool rows, in launch order), waves [n_waves]
// behind which the device keeps the n_launch packed results.
struct EditLaunch {
    std::vector<int32_t> order, words;
    int n_launch = 0, n_waves = 0;
    int col_words = 0;      // LDS words per wave: the boundary column of the longest a among the pairs of more than one stripe, 0 = none
    size_t off_pool = 0, off_a = 0, off_b = 0, off_waves = 0;
};

// Of a checked call.  A wave takes 64 / seg consecutive pairs of one segment width.
inline void edit_pack(const int32_t* seqs, const int32_t* seq_lens, int M, int L_stride, const int32_t* pair_a, const int32_t* pair_b, int N,
                      EditLaunch& out) {
    std::vector<int32_t> la((size_t)N), lb((size_t)N), seg((size_t)N);
    for (int n = 0; n < N; ++n) { la[(size_t)n] = seq_lens[pair_a[n]]; lb[(size_t)n] = seq_lens[pair_b[n]]; }
    out.order.assign((size_t)N, 0);
    out.n_launch = edit_plan(la.data(), lb.data(), N, out.order.data(), seg.data());
    out.order.resize((size_t)out.n_launch);
    out.n_waves = 0; out.col_words = 0;
    out.words.clear();
    if (!out.n_launch) return;
    std::vector<int32_t> waves;
    for (int i = 0; i < out.n_launch;) {
        const int s = seg[(size_t)out.order[(size_t)i]], per = 64 / s;
        int cnt = 1;
        while (cnt < per && i + cnt < out.n_launch && seg[(size_t)out.order[(size_t)(i + cnt)]] == s) ++cnt;
        waves.push_back((int32_t)((uint32_t)i | (uint32_t)(s == 16 ? 0 : (s == 32 ? 1 : 2)) << kEditSegShift | (uint32_t)cnt << kEditCountShift));
        i += cnt;
    }
    out.n_waves = (int)waves.size();
    const size_t pool = (size_t)M * (size_t)L_stride, n = (size_t)out.n_launch;
    out.off_pool = (size_t)M; out.off_a = out.off_pool + pool; out.off_b = out.off_a + n; out.off_waves = out.off_b + n;
    out.words.resize(out.off_waves + waves.size());
    std::copy(seq_lens, seq_lens + M, out.words.begin());
    if (pool) std::copy(seqs, seqs + pool, out.words.begin() + (ptrdiff_t)out.off_pool);
    for (size_t i = 0; i < n; ++i) {
        const int32_t p = out.order[i];
        out.words[out.off_a + i] = pair_a[p];
        out.words[out.off_b + i] = pair_b[p];
        if (lb[(size_t)p] > 64) out.col_words = std::max(out.col_words, (int)la[(size_t)p] + 1);
    }
    std::copy(waves.begin(), waves.end(), out.words.begin() + (ptrdiff_t)out.off_waves);
}

// {distance, substitutions, deletions, insertions} of a pair of la and lb tokens whose packed cost D[la][lb] is v
inline void edit_counts(uint32_t v, int la, int lb, int32_t* c) {
    const int d = (int)(v >> 16), s = (int)(v & 0xffffu);
    c[0] = d; c[1] = s;
    c[2] = (d - s - (lb - la)) / 2;
    c[3] = c[2] + lb - la;
}

// counts [N][4] of a checked, packed call: the pairs with an empty side here (all insertions or all deletions), the others from
// packed [n_launch], the kernel's results in launch order
inline void edit_unpack(const EditLaunch& L, const uint32_t* packed, const int32_t* seq_lens, const int32_t* pair_a, const int32_t* pair_b, int N,
                        int32_t* counts) {
    for (int n = 0; n < N; ++n) {
        const int la = seq_lens[pair_a[n]], lb = seq_lens[pair_b[n]];
        if (la == 0 || lb == 0) edit_counts((uint32_t)(la + lb) << 16, la, lb, counts + 4 * (size_t)n);
    }
    for (int i = 0; i < L.n_launch; ++i) {
        const int32_t n = L.order[(size_t)i];
        edit_counts(packed[i], seq_lens[pair_a[n]], seq_lens[pair_b[n]], counts + 4 * (size_t)n);
    }
}

}  // namespace dsmi
