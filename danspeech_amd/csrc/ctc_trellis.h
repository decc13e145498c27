// The device half that the three CTC trellis kernels share (align.hip, spot.hip, score.hip): how a clip's probabilities reach a
// workgroup as log probabilities in LDS, and the state words of a blank-interleaved transcript.  What a kernel does with a frame
// -- max with backpointer, max with carried start, log-sum-exp -- stays in its own file.
#pragma once
#include "common.h"
#include "ctc_host.h"      // kCtcChunk, kCtcMaxLabels

#include <cfloat>
#include <cmath>
#include <type_traits>

namespace dsmi {

// The probabilities of one clip, P [T][C], travel in chunks of kCtcChunk frames.  Chunk j + 1 is loaded into registers at the
// last frame of chunk j - 1 and turned into lp = log(max(p, FLT_MIN)) in LDS at the last frame of chunk j, a whole chunk of
// frames later: no frame waits for a global load, and a frame's chain from barrier to barrier is LDS and ALU work only (loading
// frame t + 1 within frame t left a global round trip on every frame's chain: profiles/align_time.txt has the forms that were
// slower).  The image is the kernel's own `__shared__ LP lpc[2][CtcFeeder::kImage]`: chunk j in lpc[j & 1], [frame][label].
// LP = float takes logf, LP = double log of the float widened; NT = the workgroup's threads, each moves PER values of a chunk.
// The members are references to the kernel's own P, T, C and tid: with copies the compiler laid the kernels out anew and
// score_kernel's chain came out 2 us longer on 501 frames.
template <typename LP, int NT>
struct CtcFeeder {
    static constexpr int kImage = kCtcChunk * kCtcMaxLabels;
    static constexpr int PER = kImage / NT;
    static_assert(kImage % NT == 0, "every thread moves the same number of values");
    const float* const& P;
    const int &T, &C, &tid;
    const int CF;
    float pr[PER];

    __device__ __forceinline__ CtcFeeder(const float* const& clip_probs, const int& frames, const int& labels, const int& thread)
        : P(clip_probs), T(frames), C(labels), tid(thread), CF(kCtcChunk * labels) {}

    __device__ __forceinline__ void fetch(int chunk) {           // (frames past the clip's: p = 1, nothing is read)
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * NT, f = chunk * kCtcChunk + i / C;
            pr[j] = i < CF && f < T ? P[(size_t)chunk * CF + i] : 1.f;
        }
    }
    __device__ __forceinline__ void store(LP (*lpc)[kImage], int chunk) const {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * NT;
            if (i < CF) {
                if constexpr (std::is_same_v<LP, double>) lpc[chunk & 1][i] = log((double)fmaxf(pr[j], FLT_MIN));
                else lpc[chunk & 1][i] = logf(fmaxf(pr[j], FLT_MIN));
            }
        }
    }
    // before the first frame: chunk 0 in LDS (behind the caller's next barrier), chunk 1 on its way
    __device__ __forceinline__ void prologue(LP (*lpc)[kImage]) { fetch(0); store(lpc, 0); fetch(1); }
    // lp of frame t, [label]
    __device__ __forceinline__ const LP* frame(LP (*lpc)[kImage], int t) const { return lpc[(t / kCtcChunk) & 1] + (t % kCtcChunk) * C; }
    // behind frame t's work, before its barrier: at the last frame of a chunk the next chunk's lp, then the load of the one after it
    __device__ __forceinline__ void end_of_frame(LP (*lpc)[kImage], int t) {
        if ((t + 1) % kCtcChunk == 0) {
            const int next = (t + 1) / kCtcChunk;
            store(lpc, next);
            fetch(next + 1);
        }
    }
};

// The same feeder for a kernel that walks the frames from T - 1 down to 0 (the backward pass of alt.hip): the chunks travel in
// descending order, the last one first, and the chunk that is r chunks from the end sits in lpc[r & 1].  A struct of its own with
// its own copies of P, T, C and tid, so that CtcFeeder and the three kernels built on it stay as they are.
template <typename LP, int NT>
struct CtcFeederDown {
    static constexpr int kImage = kCtcChunk * kCtcMaxLabels;
    static constexpr int PER = kImage / NT;
    static_assert(kImage % NT == 0, "every thread moves the same number of values");
    const float* P;
    const int T, C, tid, CF, last;      // last = the chunk of frame T - 1
    float pr[PER];

    __device__ __forceinline__ CtcFeederDown(const float* clip_probs, int frames, int labels, int thread)
        : P(clip_probs), T(frames), C(labels), tid(thread), CF(kCtcChunk * labels), last((frames - 1) / kCtcChunk) {}

    __device__ __forceinline__ void fetch(int chunk) {           // (chunks before the first, frames past the clip's: p = 1, nothing is read)
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * NT, f = chunk * kCtcChunk + i / C;
            pr[j] = chunk >= 0 && i < CF && f < T ? P[(size_t)chunk * CF + i] : 1.f;
        }
    }
    __device__ __forceinline__ void store(LP (*lpc)[kImage], int chunk) const {
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int i = tid + j * NT;
            if (i < CF) {
                if constexpr (std::is_same_v<LP, double>) lpc[(last - chunk) & 1][i] = log((double)fmaxf(pr[j], FLT_MIN));
                else lpc[(last - chunk) & 1][i] = logf(fmaxf(pr[j], FLT_MIN));
            }
        }
    }
    // before frame T - 1: the last chunk in LDS (behind the caller's next barrier), the one before it on its way
    __device__ __forceinline__ void prologue(LP (*lpc)[kImage]) { fetch(last); store(lpc, last); fetch(last - 1); }
    // lp of frame t, [label]
    __device__ __forceinline__ const LP* frame(LP (*lpc)[kImage], int t) const { return lpc[(last - t / kCtcChunk) & 1] + (t % kCtcChunk) * C; }
    // behind frame t's work, before its barrier: at the first frame of a chunk the lp of the chunk below, then the load of the one below that
    __device__ __forceinline__ void end_of_frame(LP (*lpc)[kImage], int t) {
        if (t % kCtcChunk == 0 && t > 0) {
            const int next = t / kCtcChunk - 1;
            store(lpc, next);
            fetch(next - 1);
        }
    }
};

// The extended sequence of a transcript tg[0 .. L): S = 2L + 1 states, blank, t_1, blank, ..., blank.  lsk[s] = the state's label
// | (a token state whose label differs from the token before: s-2 competes) << 8, and the two -inf guards in front of each alpha
// row, so that s-1 and s-2 are always readable.  (tid by reference as in the feeder: by value the guards' code came out otherwise)
template <typename A, int NT>
__device__ __forceinline__ void ctc_blank_interleaved(const int32_t* tg, int S, int blank, const int& tid, int* lsk, A* al0, A* al1) {
    for (int s = tid; s < S; s += NT) {
        const int j = s >> 1;
        lsk[s] = (s & 1) ? tg[j] | (j >= 1 && tg[j - 1] != tg[j] ? 256 : 0) : blank;
    }
    if (tid < 2) al0[tid - 2] = al1[tid - 2] = -INFINITY;
}

}  // namespace dsmi
