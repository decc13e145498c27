// CTC phrase search on the GPU (gfx950): where in each clip is each of K phrases spoken?  The recurrence and the picking rule
// are the contract of include/dsmi.h (dsmi_spot); tests/_spot_ref.py implements the same in numpy.
//
// A phrase of L tokens has S = 2L - 1 states (token, blank, token, ..., token: no leading and no trailing blank).  Each state
// carries the score of the best path that ends in it and the frame at which that path began; state 0 restarts at every frame
// (a fresh start scores 0, every carried score is <= 0), so the trellis has a free start, and reading the last state at every
// frame gives it a free end.  No backpointer matrix: the start frame travels with the score.
//
// spot_dp_kernel: one state per thread, one workgroup per (group of phrases, clip).  The host packs the phrases into groups of
// at most 256 states (spot_plan, ctc_host.h); a per-state word holds the label, "may skip from s-2", "is a phrase's state 0"
// (which keeps s-1 / s-2 from reading the neighbouring phrase) and "is a phrase's last state".  All phrases of a group share one lp chunk
// per clip: the probabilities arrive as lp in LDS a chunk of frames ahead (CtcFeeder, ctc_trellis.h), so a frame's chain from
// barrier to barrier is LDS work only.  Two score rows and two start rows live in LDS, double-buffered:
// one barrier per frame.  The owner of a phrase's last state writes E[f] and ST[f] to the workspace [B][K][T_out].
//
// spot_pick_kernel: one workgroup per (phrase, clip).  Up to max_hits times: a workgroup-wide argmax over the frames that pass
// the threshold and whose window [ST[f], f] meets no hit taken so far (largest E, then lowest f).  The hits so far sit in LDS;
// nothing is marked in the tracks, so the caller may still read them.  It also fills the tracks past the clip's frames.
#include "spot.h"
#include "ctc_trellis.h"

namespace dsmi {

__global__ void __launch_bounds__(kSpotThreads) spot_dp_kernel(SpotArgs a) {
    // rows behind two guards, so that s-1 and s-2 are always readable (the guards' values are never chosen: thread 0 is always
    // a state 0, thread 1 a state 0 or a state 1, and a state 1 never skips)
    __shared__ float al[2][kSpotThreads + 2];
    __shared__ int sf[2][kSpotThreads + 2];
    using Feeder = CtcFeeder<float, kSpotThreads>;
    __shared__ float lpc[2][Feeder::kImage];      // chunk j in lpc[j & 1], [frame][label]
    constexpr int NT = kSpotThreads;
    const int g = blockIdx.x % a.n_groups, b = blockIdx.x / a.n_groups, tid = threadIdx.x;
    const int T = a.sizes[b], C = a.C;
    if (T == 0) return;                  // (spot_pick_kernel fills the tracks of the frames a clip does not have)
    const int q = a.words[(size_t)g * NT + tid];
    const bool live = q & kSpotLive, first = q & kSpotFirst, skip = q & kSpotSkip, last = q & kSpotLast;
    const int lab = q & 255;
    const float* P = a.probs + (size_t)b * a.T_out * C;
    const size_t track = ((size_t)b * a.K + (size_t)(q >> kSpotPhraseShift)) * a.T_out;      // (of a last state)
    float* const Ek = a.E + track;
    int32_t* const Sk = a.ST + track;

    al[0][tid + 2] = al[1][tid + 2] = -INFINITY;
    sf[0][tid + 2] = sf[1][tid + 2] = -1;
    if (tid < 2) {
        al[0][tid] = al[1][tid] = -INFINITY;
        sf[0][tid] = sf[1][tid] = -1;
    }
    Feeder feed(P, T, C, tid);
    feed.prologue(lpc);
    __syncthreads();

    // ---- frame f: scores and starts in row f & 1, from row (f + 1) & 1; lp of frame f in feed.frame(lpc, f)
    for (int f = 0; f < T; ++f) {
        const float* pa = al[(f + 1) & 1] + tid;
        const int* ps = sf[(f + 1) & 1] + tid;
        const float* lpt = feed.frame(lpc, f);
        if (live) {
            // every LDS read of the state at once, then no branch: predecessor s before s-1 before s-2, strict > to move
            const float a0 = pa[2], a1 = pa[1], a2 = pa[0];
            const int b0 = ps[2], b1 = ps[1], b2 = ps[0];
            const float l = lpt[lab];
            float best = a0;
            int from = b0;
            if (a1 > best) { best = a1; from = b1; }
            if (skip && a2 > best) { best = a2; from = b2; }
            if (first) { best = 0.f; from = f; }
            const float v = best + l;        // (-inf stays -inf, and its start is -1 already)
            al[f & 1][tid + 2] = v;
            sf[f & 1][tid + 2] = from;
            if (last) { Ek[f] = v; Sk[f] = from; }
        }
        feed.end_of_frame(lpc, f);
        __syncthreads();
    }
}

// (score, frame) a before b: the larger score, then the lower frame; "none" is (-inf, -1) and loses to every candidate
__device__ __forceinline__ bool spot_before(float va, int fa, float vb, int fb) { return va > vb || (va == vb && fa < fb); }

__global__ void __launch_bounds__(kSpotThreads) spot_pick_kernel(SpotArgs a) {
    __shared__ int hs[DSMI_SPOT_MAX_HITS], he[DSMI_SPOT_MAX_HITS];     // the hits taken so far: frames [hs, he], inclusive
    __shared__ float wv[kSpotThreads / kWave];
    __shared__ int wf[kSpotThreads / kWave];
    constexpr int NT = kSpotThreads;
    const int k = blockIdx.x % a.K, b = blockIdx.x / a.K, tid = threadIdx.x;
    const int T = a.sizes[b], M = a.max_hits;
    const size_t bk = (size_t)b * a.K + k;
    float* const E = a.E + bk * a.T_out;
    int32_t* const ST = a.ST + bk * a.T_out;
    for (int f = T + tid; f < a.T_out; f += NT) { E[f] = -INFINITY; ST[f] = -1; }
    int n = 0;
    for (; n < M; ++n) {
        float bv = -INFINITY;
        int bf = -1;
        for (int f = tid; f < T; f += NT) {          // (ascending f and a strict >: the lowest frame of equal scores)
            const float e = E[f];
            const int s = ST[f];
            if (!(e > -INFINITY) || !(e >= a.min_mean_logp * (float)(f - s + 1))) continue;
            bool free_ = true;
            for (int h = 0; h < n; ++h) free_ = free_ && !(s <= he[h] && hs[h] <= f);
            if (free_ && e > bv) { bv = e; bf = f; }
        }
        for (int d = kWave / 2; d >= 1; d >>= 1) {
            const float ov = __shfl_down(bv, d, kWave);
            const int of = __shfl_down(bf, d, kWave);
            if (spot_before(ov, of, bv, bf)) { bv = ov; bf = of; }
        }
        if ((tid & (kWave - 1)) == 0) { wv[tid / kWave] = bv; wf[tid / kWave] = bf; }
        __syncthreads();
        bv = wv[0]; bf = wf[0];
        for (int w = 1; w < NT / kWave; ++w)
            if (spot_before(wv[w], wf[w], bv, bf)) { bv = wv[w]; bf = wf[w]; }
        if (bf < 0) break;                           // (the same for every thread) no candidate is left
        const int s = ST[bf];
        if (tid == 0) {
            hs[n] = s; he[n] = bf;
            a.hits[(bk * M + n) * 2] = s;
            a.hits[(bk * M + n) * 2 + 1] = bf + 1;
            a.scores[bk * M + n] = bv;
        }
        __syncthreads();                             // the hit is in LDS, and wv / wf may be written again
    }
    for (int i = n + tid; i < M; i += NT) {          // rows past the count are 0
        a.hits[(bk * M + i) * 2] = 0;
        a.hits[(bk * M + i) * 2 + 1] = 0;
        a.scores[bk * M + i] = 0.f;
    }
    if (tid == 0) a.counts[bk] = n;
}

hipError_t launch_spot(const SpotArgs& a, int B, hipStream_t s) {
    hipLaunchKernelGGL(spot_dp_kernel, dim3(a.n_groups * B), dim3(kSpotThreads), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spot_pick_kernel, dim3(a.K * B), dim3(kSpotThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dsmi
