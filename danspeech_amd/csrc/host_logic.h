// Host-only logic of libdsmi.so that touches no HIP call: kept in a header of its own so that `make -C danspeech_amd/csrc asan`
// can build it (with the language-model readers lm.cpp.inc / lm_klm.cpp.inc) for the CPU under AddressSanitizer and
// UndefinedBehaviorSanitizer (tools/asan/host_fuzz.cpp, tests/test_asan_host.py): GPU sanitizers are not available on the pool.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

namespace dsmi {

// order[k] = index of the k-th longest clip (stable): rank k % world takes it as its (k / world)-th clip
// (danspeech_amd/parallel.py plan_shards; pack_padded_sequence's order, reference model.py:117)
inline std::vector<int> length_order(const int64_t* n_samples, int n) {
    std::vector<int> order((size_t)std::max(n, 0));
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return n_samples[a] > n_samples[b]; });
    return order;
}

inline void plan_shards(const int64_t* n_samples, int n, int world, int32_t* rank_of, int32_t* slot_of) {
    const std::vector<int> order = length_order(n_samples, n);
    for (int k = 0; k < n; ++k) { rank_of[order[(size_t)k]] = k % world; slot_of[order[(size_t)k]] = k / world; }
}

// The energy gate of the reference's example_scripts/video_transcribe_simulation.py:84-143, one pass over the hop energies:
// phrases [seg_start, seg_end) in samples.  Returns how many phrases there are; at most max_segments are stored.
inline int segment_phrases(const double* e, int64_t nhops, int step, double energy_threshold, int pause_hops, int phrase_hops,
                           int64_t* seg_start, int64_t* seg_end, int max_segments) {
    bool is_speaking = false;
    int64_t frames_counter = 0, pause_count = 0, start_index = 0, iterator = 0;
    int found = 0;
    for (int64_t i = 0; i < nhops; ++i) {
        const double energy = e[i];
        if (energy > energy_threshold && !is_speaking) {
            is_speaking = true;
            start_index = iterator - 2 * (int64_t)step;
            if (start_index < 0) start_index = iterator;
        }
        iterator += step;
        if (is_speaking) {
            ++frames_counter;
            if (energy > energy_threshold) pause_count = 0;
            else ++pause_count;
        }
        if (pause_count > pause_hops && is_speaking) {
            if (frames_counter - pause_count > phrase_hops) {
                if (found < max_segments) { seg_start[found] = start_index; seg_end[found] = iterator; }
                ++found;
            }
            is_speaking = false;
            frames_counter = 0;
            pause_count = 0;
        }
    }
    return found;
}

// The live gate, Recognizer.listen_stream (Recognizer.py:218-324), restarted after every closed utterance as listen_in_background
// does (:356-377).  One session's state between runs of buffers:
struct GateState { int64_t phase = 0, kept = 0, phrase_count = 0, pause_count = 0; };      // phase: 0 waiting, 1 phrase
struct GateParams { double threshold; int64_t pause_n, phrase_n, keep_n; };

// ceil(seconds / (chunk / rate)) in float64, as :239-245 compute it
inline int64_t gate_buffer_count(double seconds, int chunk, int rate) {
    const double spb = (double)chunk / (double)rate;
    const double c = std::ceil(seconds / spb);
    return c < 0 ? 0 : (c > 4e15 ? (int64_t)4e15 : (int64_t)c);
}

// audioop.rms(buffer, 2): the sum of squares is an exact integer below 2^53, the quotient and the root are libm's
inline uint32_t gate_energy(uint64_t S, int64_t len) { return len > 0 ? (uint32_t)std::sqrt((double)S / (double)len) : 0u; }

// Events (first_buffer, n_buffers, last) of one run: an event joins the one before it when it continues it (the reference's
// one-buffer yields of a phrase become one run of buffers); a yield of no buffers survives only as a last mark.
struct GateEvents {
    int64_t* first; int64_t* count; int32_t* last; int64_t cap; int64_t n = 0;
    int64_t pf = 0, pc = 0; bool open = false;          // the newest event (kept here: it may lie past cap)
    void emit(int64_t f, int64_t c, bool l) {
        if (open && (c == 0 || pf + pc == f)) { pc += c; }
        else if (c == 0 && !l) return;
        else { ++n; pf = f; pc = c; }
        open = !l;
        if (n <= cap) { first[n - 1] = pf; count[n - 1] = pc; last[n - 1] = l ? 1 : 0; }
    }
};

// Advances one session over buffers 0 .. n - 1 of a run (sums S[i] of len[i] samples); end_of_stream is the empty read after them.
// Returns the utterances closed.
inline int64_t endpoint_gate(const GateParams& p, GateState& st, const uint64_t* S, const int64_t* len, int64_t n, bool end_of_stream,
                             GateEvents& ev, uint32_t* energies) {
    int64_t closed = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t e = gate_energy(S[i], len[i]);
        if (energies) energies[i] = e;
        const bool loud = (double)e > p.threshold;
        if (st.phase == 0) {
            st.kept = std::min(st.kept + 1, p.keep_n);          // appended, then trimmed, then tested (:263-272)
            if (loud) {
                ev.emit(i + 1 - st.kept, st.kept, false);
                st = GateState{1, 0, 0, 0};
            }
            continue;
        }
        ++st.phrase_count;
        st.pause_count = loud ? 0 : st.pause_count + 1;
        if (st.pause_count <= p.pause_n) { ev.emit(i, 1, false); continue; }
        // too short a phrase: the breaking buffer is dropped and the utterance goes on
        if (st.phrase_count - st.pause_count >= p.phrase_n) { ev.emit(i, 1, true); ++closed; }
        st = GateState{};
    }
    if (end_of_stream) {
        if (st.phase == 0) ev.emit(n - st.kept, st.kept, false);
        ev.emit(n, 0, true);
        ++closed;
        st = GateState{};
    }
    return closed;
}

}  // namespace dsmi
