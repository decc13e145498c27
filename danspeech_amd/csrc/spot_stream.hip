// Streaming phrase watch on the GPU (gfx950): dsmi_spot's trellis carried from chunk to chunk of N live sessions in one launch,
// with the online picking rule run beside it.  The recurrence, the tie rule and the rule are the contract of include/dsmi.h
// (dsmi_spot_stream_advance_many); tests/_spot_stream_ref.py implements the same in numpy.
//
// spot_stream_kernel: one workgroup per (group of phrases, session), one state per thread, the frame loop of spot_dp_kernel
// (spot.hip): lp a chunk of frames ahead in LDS (CtcFeeder over this call's frames), two score rows and two start rows in LDS
// behind their guards, one barrier per frame.  What is new:
//   - the entry restores the row of the session's last frame into the "previous" buffer (t0 = 0, a new utterance: -inf / -1,
//     and nothing of the state block is read), starts are written as t0 + f, and the exit stores the last row back;
//   - the owner of a phrase's last state keeps the picker's state (spot_pick.h) in registers, runs the rule on its own (score,
//     start) behind the frame's LDS writes -- the other lanes' chain from barrier to barrier is spot_dp_kernel's -- and writes a
//     fired event with plain stores to its own (session, phrase) slots: one thread owns one phrase, so nothing is shared;
//   - with 0 frames nothing of the trellis runs: the owners flush (when asked), zero their rows and leave.
// No communication between workgroups, no spinning, no atomics; the state block is read at the entry and written at the exit only.
#include "spot_stream.h"
#include "ctc_trellis.h"

namespace dsmi {

__global__ void __launch_bounds__(kSpotThreads) spot_stream_kernel(SpotStreamArgs a) {
    __shared__ float al[2][kSpotThreads + 2];
    __shared__ int sf[2][kSpotThreads + 2];
    using Feeder = CtcFeeder<float, kSpotThreads>;
    __shared__ float lpc[2][Feeder::kImage];      // chunk j in lpc[j & 1], [frame][label]
    constexpr int NT = kSpotThreads;
    const int g = blockIdx.x % a.n_groups, b = blockIdx.x / a.n_groups, tid = threadIdx.x;
    const SpotStreamDesc d = a.desc[b];
    const int T = d.T, C = a.C, t0 = d.t0, M = a.max_events;
    const int q = a.words[(size_t)g * NT + tid];
    const bool live = q & kSpotLive, first = q & kSpotFirst, skip = q & kSpotSkip, last = q & kSpotLast;
    const int lab = q & 255, k = q >> kSpotPhraseShift;      // (k: of a last state)
    const float* P = d.probs;
    const size_t bk = (size_t)b * a.K + (size_t)k;
    float* const Ek = a.E ? a.E + bk * a.F_stride : nullptr;
    int32_t* const Sk = a.E ? a.ST + bk * a.F_stride : nullptr;
    int32_t* const hit = a.hits + bk * M * 2;
    float* const hsc = a.scores + bk * M;
    int32_t* const hfi = a.fired + bk * M;

    // ---- the owner's picker: its state in registers, the events of this call counted in n_ev
    SpotPick pk = spot_pick_fresh();
    if (last && t0 > 0) pk = d.pick[k];
    int n_ev = 0;
    auto emit = [&](int s, int e, float v, int at) {
        if (n_ev < M) { hit[2 * n_ev] = s; hit[2 * n_ev + 1] = e + 1; hsc[n_ev] = v; hfi[n_ev] = at; }
        ++n_ev;
    };
    auto leave = [&] {      // (an owner) the flush, the rows past the count, the count, the picker's state
        if (d.flush) spot_pick_flush(pk, t0 + T, emit);
        for (int i = n_ev; i < M; ++i) { hit[2 * i] = 0; hit[2 * i + 1] = 0; hsc[i] = 0.f; hfi[i] = 0; }
        a.counts[bk] = n_ev;
        d.pick[k] = pk;
    };
    if (T == 0) {           // (the same for the whole workgroup) nothing of the trellis runs, the rows stay as they are
        if (last) leave();
        return;
    }

    // ---- the carried row of this thread's state: into the buffer frame 0 reads, row 1
    const size_t at = (size_t)g * NT + tid;
    float v = t0 > 0 ? d.score[at] : -INFINITY;
    int from = t0 > 0 ? d.start[at] : -1;
    al[0][tid + 2] = -INFINITY; al[1][tid + 2] = v;
    sf[0][tid + 2] = -1; sf[1][tid + 2] = from;
    if (tid < 2) {
        al[0][tid] = al[1][tid] = -INFINITY;
        sf[0][tid] = sf[1][tid] = -1;
    }
    Feeder feed(P, T, C, tid);
    feed.prologue(lpc);
    __syncthreads();

    // ---- frame f of this call = frame t0 + f of the utterance: row f & 1 from row (f + 1) & 1, as spot_dp_kernel
    for (int f = 0; f < T; ++f) {
        const float* pa = al[(f + 1) & 1] + tid;
        const int* ps = sf[(f + 1) & 1] + tid;
        const float* lpt = feed.frame(lpc, f);
        if (live) {
            const float a0 = pa[2], a1 = pa[1], a2 = pa[0];
            const int b0 = ps[2], b1 = ps[1], b2 = ps[0];
            const float l = lpt[lab];
            float best = a0;
            from = b0;
            if (a1 > best) { best = a1; from = b1; }
            if (skip && a2 > best) { best = a2; from = b2; }
            if (first) { best = 0.f; from = t0 + f; }
            v = best + l;                    // (-inf stays -inf, and its start is -1 already)
            al[f & 1][tid + 2] = v;
            sf[f & 1][tid + 2] = from;
            if (last) {                      // behind the LDS writes: registers only, a store when an event fires
                if (Ek) { Ek[f] = v; Sk[f] = from; }
                spot_pick_frame(pk, t0 + f, v, from, a.min_mean_logp, a.settle, emit);
            }
        }
        feed.end_of_frame(lpc, f);
        __syncthreads();
    }
    d.score[at] = v;
    d.start[at] = from;
    if (last) leave();
}

hipError_t launch_spot_stream(const SpotStreamArgs& a, int n, hipStream_t s) {
    hipLaunchKernelGGL(spot_stream_kernel, dim3(a.n_groups * n), dim3(kSpotThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dsmi
