// The host half of the five CTC trellis tools (dsmi_align, dsmi_spot, dsmi_score, dsmi_alternatives, dsmi_occupancy: ctc_tools.hip): the checks of everything a
// caller hands in, the packing of phrases into workgroups and the launch order of candidates.  No HIP: a plain C++ compiler
// takes it, and tools/asan/host_fuzz.cpp (ctccheck, occcheck, scoreplan) runs it under ASan + UBSan on exactly sized arrays.  A check
// returns DSMI_OK or a DSMI_ERR_* code with the message in `err`; what the numbers alone refuse is refused before any array is read.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dsmi.h"

namespace dsmi {

constexpr int kCtcChunk = 16;           // frames of probabilities per prefetch (ctc_trellis.h)
constexpr int kCtcMaxLabels = 128;      // dsmi_decoder_create's limit: a chunk's lp image holds kCtcChunk rows of at most this many
static_assert(kCtcMaxLabels <= 256, "a state word keeps its label in the low byte");

// ---- phrase search: the packing
constexpr int kSpotThreads = 256;       // one state per thread: a group of phrases holds at most this many states
static_assert(2 * DSMI_SPOT_MAX_TOKENS - 1 <= kSpotThreads, "the longest phrase fits one group");

// per-state word of a group, [n_groups][kSpotThreads]: label in the low byte, then
constexpr int kSpotSkip = 1 << 8;       // even state >= 2 whose token differs from the token before: s-2 competes
constexpr int kSpotFirst = 1 << 9;      // state 0 of a phrase: always restarts, never looks at s-1 / s-2 (the neighbouring phrase)
constexpr int kSpotLast = 1 << 10;      // state S-1 of a phrase: writes the tracks of phrase (word >> kSpotPhraseShift)
constexpr int kSpotLive = 1 << 11;      // a state at all (the tail of a group is dead)
constexpr int kSpotPhraseShift = 16;

// Phrases in order, S = 2 * len - 1 states each (token, blank, token, ..., token); a phrase that does not fit the group's
// kSpotThreads states opens the next group.  group_of[k], first_state[k] = where phrase k's state 0 sits.  Returns the number of groups.
inline int spot_plan(const int32_t* lens, int K, int32_t* group_of, int32_t* first_state) {
    int g = 0, used = 0;
    for (int k = 0; k < K; ++k) {
        const int S = 2 * lens[k] - 1;
        if (used + S > kSpotThreads) { ++g; used = 0; }
        group_of[k] = g;
        first_state[k] = used;
        used += S;
    }
    return g + 1;
}

// The words of phrases placed by spot_plan, into words [n_groups][kSpotThreads] that the caller zeroed (0 = a dead state).
inline void spot_pack(const int32_t* phrases, const int32_t* lens, int K, int L_stride, int blank, const int32_t* group_of,
                      const int32_t* first_state, int32_t* words) {
    for (int k = 0; k < K; ++k) {
        const int L = lens[k], S = 2 * L - 1;
        const int32_t* ph = phrases + (size_t)k * L_stride;
        int32_t* w = words + (size_t)group_of[k] * kSpotThreads + first_state[k];
        for (int s = 0; s < S; ++s) {
            const int j = s >> 1;
            int32_t q = kSpotLive | ((s & 1) ? blank : ph[j]);
            if (!(s & 1) && j >= 1 && ph[j] != ph[j - 1]) q |= kSpotSkip;
            if (s == 0) q |= kSpotFirst;
            if (s == S - 1) q |= kSpotLast | (k << kSpotPhraseShift);
            w[s] = q;
        }
    }
}

// ---- transcript scoring: the launch order.  Candidates with the most frames first (the longest chains start first), then by
// clip (the candidates of one clip run side by side and share the clip's probabilities in L2), then the most tokens first, then
// by index.  Every entry of the three arrays is >= 0.  order[i] = the candidate workgroup i scores.  Returns N.
inline int score_plan(const int32_t* cand_clip, const int32_t* cand_frames, const int32_t* target_lens, int N, int32_t* order) {
    for (int n = 0; n < N; ++n) order[n] = n;
    std::sort(order, order + N, [&](int32_t x, int32_t y) {
        if (cand_frames[x] != cand_frames[y]) return cand_frames[x] > cand_frames[y];
        if (cand_clip[x] != cand_clip[y]) return cand_clip[x] < cand_clip[y];
        if (target_lens[x] != target_lens[y]) return target_lens[x] > target_lens[y];
        return x < y;
    });
    return N;
}

// ---- the checks every entry shares.  CtcRows: what a tool calls its token rows in its messages, a row's least length, L_stride's limit
struct CtcRows { const char *tool, *unit, *length, *id, *limit_name; int min_len, limit; };
constexpr CtcRows kAlignRows{"align", "clip", "target length", "target id", "DSMI_ALIGN_MAX_TOKENS", 0, DSMI_ALIGN_MAX_TOKENS};
constexpr CtcRows kSpotRows{"spot", "phrase", "length", "token id", "DSMI_SPOT_MAX_TOKENS", 1, DSMI_SPOT_MAX_TOKENS};
constexpr CtcRows kScoreRows{"score", "candidate", "target length", "target id", "DSMI_SCORE_MAX_TOKENS", 0, DSMI_SCORE_MAX_TOKENS};
constexpr CtcRows kAltRows{"alternatives", "candidate", "target length", "target id", "DSMI_ALT_MAX_TOKENS", 0, DSMI_ALT_MAX_TOKENS};

inline int ctc_refuse(std::string& err, int code, const std::string& msg) { err = msg; return code; }
// L_stride against the tool's limit (on the number alone)
inline int ctc_check_stride(const CtcRows& r, int L_stride, std::string& err) {
    if (L_stride <= r.limit) return DSMI_OK;
    return ctc_refuse(err, DSMI_ERR_CAPACITY, std::string(r.tool) + ": L_stride " + std::to_string(L_stride) + " exceeds " + r.limit_name + " (" + std::to_string(r.limit) + ")");
}

// sz[b] = the frames of clip b (sizes null: T_out), each inside 0 .. T_out
inline int ctc_check_sizes(const CtcRows& r, const int32_t* sizes, int B, int To, int32_t* sz, std::string& err) {
    for (int b = 0; b < B; ++b) {
        sz[b] = sizes ? sizes[b] : To;
        if (sz[b] < 0 || sz[b] > To) return ctc_refuse(err, DSMI_ERR_INVALID, std::string(r.tool) + ": clip " + std::to_string(b) + ": size outside 0 .. T_out");
    }
    return DSMI_OK;
}

// One token row, row[0 .. L): L inside min_len .. L_stride, every id a label and not the blank.  *repeats = the pairs of equal
// neighbours (each needs a blank frame between them).  Nothing of the row is read where L is refused.
inline int ctc_check_row(const CtcRows& r, int index, const int32_t* row, int L, int L_stride, int C, int blank, int* repeats, std::string& err) {
    auto where = [&] { return std::string(r.tool) + ": " + r.unit + " " + std::to_string(index) + ": "; };      // (only a refusal pays for text)
    if (L < r.min_len || L > L_stride) return ctc_refuse(err, DSMI_ERR_INVALID, where() + r.length + " outside " + std::to_string(r.min_len) + " .. L_stride");
    int equal = 0;
    for (int k = 0; k < L; ++k) {
        if (row[k] < 0 || row[k] >= C || row[k] == blank) return ctc_refuse(err, DSMI_ERR_INVALID, where() + r.id + " " + std::to_string(row[k]) + " is the blank or not a label");
        if (k > 0 && row[k] == row[k - 1]) ++equal;
    }
    *repeats = equal;
    return DSMI_OK;
}

// The feasibility rule: one frame per token and one more between two equal tokens.  L, or -1 (the kernel skips the row).
inline int ctc_feasible_len(int L, int repeats, int frames) { return L + repeats > frames ? -1 : L; }

// ---- each entry's arguments, behind its null-pointer checks
// sz [B], tl [B] (-1: infeasible), *L_max = the longest feasible transcript
inline int align_check(const int32_t* sizes, int B, int To, const int32_t* targets, const int32_t* target_lens, int L_stride, int C,
                       int blank, std::vector<int32_t>& sz, std::vector<int32_t>& tl, int* L_max, std::string& err) {
    if (B <= 0 || To <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "align: B and T_out must be positive");
    if (L_stride < 0) return ctc_refuse(err, DSMI_ERR_INVALID, "align: negative L_stride");
    if (int rc = ctc_check_stride(kAlignRows, L_stride, err)) return rc;
    sz.assign((size_t)B, 0); tl.assign((size_t)B, 0);
    if (int rc = ctc_check_sizes(kAlignRows, sizes, B, To, sz.data(), err)) return rc;
    *L_max = 0;
    for (int b = 0; b < B; ++b) {
        int repeats = 0;
        if (int rc = ctc_check_row(kAlignRows, b, targets + (size_t)b * L_stride, target_lens[b], L_stride, C, blank, &repeats, err)) return rc;
        tl[b] = ctc_feasible_len(target_lens[b], repeats, sz[b]);
        *L_max = std::max(*L_max, (int)tl[b]);
    }
    return DSMI_OK;
}

inline int spot_check(const int32_t* sizes, int B, int To, const int32_t* phrases, const int32_t* phrase_lens, int K, int L_stride,
                      int max_hits, float min_mean_logp, int C, int blank, std::vector<int32_t>& sz, std::string& err) {
    if (B <= 0 || To <= 0 || K <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "spot: B, T_out and K must be positive");
    if (max_hits < 1 || max_hits > DSMI_SPOT_MAX_HITS)
        return ctc_refuse(err, DSMI_ERR_INVALID, "spot: max_hits outside 1 .. DSMI_SPOT_MAX_HITS (" + std::to_string(DSMI_SPOT_MAX_HITS) + ")");
    if (std::isnan(min_mean_logp)) return ctc_refuse(err, DSMI_ERR_INVALID, "spot: min_mean_logp is not a number");
    if (int rc = ctc_check_stride(kSpotRows, L_stride, err)) return rc;
    if (K > DSMI_SPOT_MAX_PHRASES)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "spot: " + std::to_string(K) + " phrases exceed DSMI_SPOT_MAX_PHRASES (" + std::to_string(DSMI_SPOT_MAX_PHRASES) + ")");
    constexpr uint64_t kTrackCap = (uint64_t)1 << 27;
    if ((uint64_t)B * (uint64_t)K > kTrackCap || (uint64_t)B * (uint64_t)K * (uint64_t)To > kTrackCap)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "spot: B * K * T_out exceeds 2^27 (the track workspace)");
    sz.assign((size_t)B, 0);
    if (int rc = ctc_check_sizes(kSpotRows, sizes, B, To, sz.data(), err)) return rc;
    for (int k = 0; k < K; ++k) {
        int repeats = 0;
        if (int rc = ctc_check_row(kSpotRows, k, phrases + (size_t)k * L_stride, phrase_lens[k], L_stride, C, blank, &repeats, err)) return rc;
    }
    return DSMI_OK;
}

// ---- streaming phrase watch (dsmi_spot_watch_*, dsmi_spot_stream_*: spot_watch.hip)
constexpr CtcRows kWatchRows{"spot watch", "phrase", "length", "token id", "DSMI_SPOT_MAX_TOKENS", 1, DSMI_SPOT_MAX_TOKENS};
constexpr uint64_t kWatchEventCap = (uint64_t)1 << 24;      // n * K * max_events: the events of one call, on the watch and copied back
constexpr uint64_t kWatchTrackCap = (uint64_t)1 << 27;      // n * K * F_stride: the tracks of one call, when asked for

// a watch's phrase list and picking parameters
inline int spot_watch_check(const int32_t* phrases, const int32_t* phrase_lens, int K, int L_stride, float min_mean_logp, int settle_frames,
                            int C, int blank, std::string& err) {
    if (K <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "spot watch: K must be positive");
    if (settle_frames < 1) return ctc_refuse(err, DSMI_ERR_INVALID, "spot watch: settle_frames must be at least 1");
    if (std::isnan(min_mean_logp)) return ctc_refuse(err, DSMI_ERR_INVALID, "spot watch: min_mean_logp is not a number");
    if (int rc = ctc_check_stride(kWatchRows, L_stride, err)) return rc;
    if (K > DSMI_SPOT_MAX_PHRASES)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "spot watch: " + std::to_string(K) + " phrases exceed DSMI_SPOT_MAX_PHRASES (" + std::to_string(DSMI_SPOT_MAX_PHRASES) + ")");
    for (int k = 0; k < K; ++k) {
        int repeats = 0;
        if (int rc = ctc_check_row(kWatchRows, k, phrases + (size_t)k * L_stride, phrase_lens[k], L_stride, C, blank, &repeats, err)) return rc;
    }
    return DSMI_OK;
}

// One dsmi_spot_stream_advance_many, behind its null-pointer checks: handles [n] (each non-null), watch_of [n] = the watch of each,
// consumed [n] = the frames each has taken, probs [n] (may be null itself when no stream has frames), frames [n].  What the
// numbers alone refuse is refused before any array is read.
inline int spot_stream_check(const void* const* handles, const void* const* watch_of, const int64_t* consumed, int n, const float* const* probs,
                             const int32_t* frames, int K, int max_events, bool tracks, int F_stride, std::string& err) {
    if (n < 1 || n > DSMI_SPOT_STREAM_MANY_MAX)
        return ctc_refuse(err, DSMI_ERR_INVALID, "spot stream: n outside 1 .. DSMI_SPOT_STREAM_MANY_MAX (" + std::to_string(DSMI_SPOT_STREAM_MANY_MAX) + ")");
    if (max_events < 1 || max_events > DSMI_SPOT_MAX_HITS)
        return ctc_refuse(err, DSMI_ERR_INVALID, "spot stream: max_events outside 1 .. DSMI_SPOT_MAX_HITS (" + std::to_string(DSMI_SPOT_MAX_HITS) + ")");
    if (tracks && F_stride < 0) return ctc_refuse(err, DSMI_ERR_INVALID, "spot stream: negative F_stride");
    if ((uint64_t)n * (uint64_t)K * (uint64_t)max_events > kWatchEventCap)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "spot stream: n * K * max_events exceeds 2^24 (the events)");
    if (tracks && (uint64_t)n * (uint64_t)K * (uint64_t)F_stride > kWatchTrackCap)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "spot stream: n * K * F_stride exceeds 2^27 (the tracks)");
    auto at = [](int i) { return "spot stream " + std::to_string(i) + ": "; };
    {
        std::vector<const void*> sorted(handles, handles + n);
        std::sort(sorted.begin(), sorted.end());
        const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
        if (twice != sorted.end()) {
            int i = n - 1;
            while (handles[i] != *twice) --i;      // (the later of the two)
            return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "the same handle appears twice in one call");
        }
    }
    for (int i = 0; i < n; ++i) {
        if (watch_of[i] != watch_of[0]) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "the streams of one call must belong to one watch");
        if (frames[i] < 0) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "negative frame count");
        if (frames[i] > 0 && (!probs || !probs[i])) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "no probabilities for " + std::to_string(frames[i]) + " frames");
        if (tracks && frames[i] > F_stride) return ctc_refuse(err, DSMI_ERR_INVALID, at(i) + "F_stride is below the frame count");
        if (consumed[i] + (int64_t)frames[i] > (int64_t)INT32_MAX) return ctc_refuse(err, DSMI_ERR_CAPACITY, at(i) + "the utterance would pass 2^31 - 1 frames");
    }
    return DSMI_OK;
}

// sz [B], tl [N] (-1: infeasible), frames [N] = the frames of each candidate's clip, *L_max = the longest feasible candidate
inline int score_check(const int32_t* sizes, int B, int To, const int32_t* cand_clip, const int32_t* targets, const int32_t* target_lens,
                       int N, int L_stride, int C, int blank, std::vector<int32_t>& sz, std::vector<int32_t>& tl,
                       std::vector<int32_t>& frames, int* L_max, std::string& err) {
    if (B <= 0 || To <= 0 || N <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "score: B, T_out and N must be positive");
    if (L_stride < 0) return ctc_refuse(err, DSMI_ERR_INVALID, "score: negative L_stride");
    if (int rc = ctc_check_stride(kScoreRows, L_stride, err)) return rc;
    if ((uint64_t)N * (uint64_t)L_stride > ((uint64_t)1 << 24)) return ctc_refuse(err, DSMI_ERR_CAPACITY, "score: N * L_stride exceeds 2^24");
    sz.assign((size_t)B, 0); tl.assign((size_t)N, 0); frames.assign((size_t)N, 0);
    if (int rc = ctc_check_sizes(kScoreRows, sizes, B, To, sz.data(), err)) return rc;
    *L_max = 0;
    for (int n = 0; n < N; ++n) {
        const int b = cand_clip[n];
        if (b < 0 || b >= B) return ctc_refuse(err, DSMI_ERR_INVALID, "score: candidate " + std::to_string(n) + ": clip outside 0 .. B-1");
        int repeats = 0;
        if (int rc = ctc_check_row(kScoreRows, n, targets + (size_t)n * L_stride, target_lens[n], L_stride, C, blank, &repeats, err)) return rc;
        frames[n] = sz[b];
        tl[n] = ctc_feasible_len(target_lens[n], repeats, sz[b]);
        *L_max = std::max(*L_max, (int)tl[n]);
    }
    return DSMI_OK;
}

// ---- token confidence: where each candidate's stored trellises lie.  A feasible candidate with T > 0 frames and L tokens takes
// T * (2L + 1) elements from base[n], in the order of the candidates (every other candidate: base[n] = the running total, nothing
// taken).  tl [N] as the checks leave it.  Returns the total.
inline uint64_t alt_place(const int32_t* tl, const int32_t* frames, int N, int32_t* base) {
    uint64_t total = 0;
    for (int n = 0; n < N; ++n) {
        if (base) base[n] = (int32_t)std::min<uint64_t>(total, INT32_MAX);
        if (tl[n] >= 0) total += (uint64_t)frames[n] * (2 * (uint64_t)tl[n] + 1);
    }
    return total;
}
constexpr uint64_t kAltOutCap = (uint64_t)1 << 24;       // N * L_stride * n_labels: the results, on the handle and copied back
constexpr uint64_t kAltTrellisCap = (uint64_t)1 << 25;   // elements of one stored trellis over all candidates of a call

// What the two tools with a stored trellis per candidate check alike, behind their own checks of the numbers: the sizes, every
// candidate's clip and token row, the feasibility, and the stored trellises against their cap and in their places.
inline int ctc_check_stored(const CtcRows& r, const int32_t* sizes, int B, int To, const int32_t* cand_clip, const int32_t* targets,
                            const int32_t* target_lens, int N, int L_stride, int C, int blank, std::vector<int32_t>& sz,
                            std::vector<int32_t>& tl, std::vector<int32_t>& frames, std::vector<int32_t>& base, int* L_max,
                            uint64_t* trellis, std::string& err) {
    sz.assign((size_t)B, 0); tl.assign((size_t)N, 0); frames.assign((size_t)N, 0);
    if (int rc = ctc_check_sizes(r, sizes, B, To, sz.data(), err)) return rc;
    *L_max = 0;
    for (int n = 0; n < N; ++n) {
        const int b = cand_clip[n];
        if (b < 0 || b >= B) return ctc_refuse(err, DSMI_ERR_INVALID, std::string(r.tool) + ": candidate " + std::to_string(n) + ": clip outside 0 .. B-1");
        int repeats = 0;
        if (int rc = ctc_check_row(r, n, targets + (size_t)n * L_stride, target_lens[n], L_stride, C, blank, &repeats, err)) return rc;
        frames[n] = sz[b];
        tl[n] = ctc_feasible_len(target_lens[n], repeats, sz[b]);
        *L_max = std::max(*L_max, (int)tl[n]);
    }
    *trellis = alt_place(tl.data(), frames.data(), N, nullptr);
    if (*trellis > kAltTrellisCap)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, std::string(r.tool) + ": the stored trellises, the sum of frames * (2 * length + 1) over the candidates, exceed 2^25 elements (" + std::to_string(*trellis) + ")");
    base.assign((size_t)N, 0);
    alt_place(tl.data(), frames.data(), N, base.data());
    return DSMI_OK;
}

// sz [B], tl [N] (-1: infeasible), frames [N], base [N] (alt_place), *L_max = the longest feasible candidate, *trellis = alt_place's total
inline int alt_check(const int32_t* sizes, int B, int To, const int32_t* cand_clip, const int32_t* targets, const int32_t* target_lens,
                     int N, int L_stride, int C, int blank, std::vector<int32_t>& sz, std::vector<int32_t>& tl,
                     std::vector<int32_t>& frames, std::vector<int32_t>& base, int* L_max, uint64_t* trellis, std::string& err) {
    if (B <= 0 || To <= 0 || N <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "alternatives: B, T_out and N must be positive");
    if (L_stride < 0) return ctc_refuse(err, DSMI_ERR_INVALID, "alternatives: negative L_stride");
    if (int rc = ctc_check_stride(kAltRows, L_stride, err)) return rc;
    if ((uint64_t)N * (uint64_t)L_stride * (uint64_t)C > kAltOutCap)
        return ctc_refuse(err, DSMI_ERR_CAPACITY, "alternatives: N * L_stride * n_labels exceeds 2^24 (the results)");
    if ((uint64_t)N * (uint64_t)L_stride > kAltOutCap) return ctc_refuse(err, DSMI_ERR_CAPACITY, "alternatives: N * L_stride exceeds 2^24");
    return ctc_check_stored(kAltRows, sizes, B, To, cand_clip, targets, target_lens, N, L_stride, C, blank, sz, tl, frames, base, L_max, trellis, err);
}

// ---- occupancy: two stored trellises per feasible candidate, placed by alt_place and under alternatives' cap; the outputs are the
// caller's own device arrays.  The per-label sums need no grouping from the host: an output thread walks its candidate's tokens
// in order (occ.hip).
constexpr CtcRows kOccRows{"occupancy", "candidate", "target length", "target id", "DSMI_OCC_MAX_TOKENS", 0, DSMI_OCC_MAX_TOKENS};
constexpr uint64_t kOccUploadCap = (uint64_t)1 << 24;    // N * L_stride: the targets, uploaded to the handle

// sz [B], tl [N] (-1: infeasible), frames [N], base [N] (alt_place), *L_max = the longest feasible candidate, *trellis = alt_place's total
inline int occ_check(const int32_t* sizes, int B, int To, const int32_t* cand_clip, const int32_t* targets, const int32_t* target_lens,
                     int N, int L_stride, int C, int blank, std::vector<int32_t>& sz, std::vector<int32_t>& tl,
                     std::vector<int32_t>& frames, std::vector<int32_t>& base, int* L_max, uint64_t* trellis, std::string& err) {
    if (B <= 0 || To <= 0 || N <= 0) return ctc_refuse(err, DSMI_ERR_INVALID, "occupancy: B, T_out and N must be positive");
    if (L_stride < 0) return ctc_refuse(err, DSMI_ERR_INVALID, "occupancy: negative L_stride");
    if (int rc = ctc_check_stride(kOccRows, L_stride, err)) return rc;
    if ((uint64_t)N * (uint64_t)L_stride > kOccUploadCap) return ctc_refuse(err, DSMI_ERR_CAPACITY, "occupancy: N * L_stride exceeds 2^24 (the upload buffer)");
    return ctc_check_stored(kOccRows, sizes, B, To, cand_clip, targets, target_lens, N, L_stride, C, blank, sz, tl, frames, base, L_max, trellis, err);
}

}  // namespace dsmi
