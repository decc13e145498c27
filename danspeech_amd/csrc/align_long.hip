// Long-form CTC forced alignment on the GPU (gfx950): dsmi_align's recurrence, tie rule and outputs (align.hip, include/dsmi.h)
// for one recording of up to 2^22 frames and 2^20 tokens, with an optional free blank at either end.
//
// The trellis is cut into frame tiles of F = kAlongF frames and state tiles of W = kAlongW states.  HBM keeps one float32 alpha
// row per frame tile ("checkpoint": row j = alpha of frame min(j F, T - 1)) and no backpointers.  No launch signals between its
// workgroups:
//   along_first     row 0 from frame 0's probabilities.
//   along_forward   one launch per frame tile, one workgroup per state tile [s0, s1).  alpha_t(s) depends on alpha_{t-1}(s-2 .. s),
//                   so F frames on, [s0, s1) depends on [s0 - 2F, s1) of the checkpoint and on nothing else: the workgroup loads
//                   that window, runs the F frames in LDS as align_kernel does (two rows, one barrier per frame, CtcFeeder) and
//                   stores [s0, s1) of the last frame.  The 2F halo cells are recomputed by the tile to the left, never handed
//                   over; those of them whose inputs lie left of the window hold values of no meaning after a frame and are never
//                   stored.  A tile whose whole window lies right of state 2t + 1, the furthest any path has come at the
//                   checkpoint's frame t, stores -inf without running: that is what the recurrence gives there.
//   along_back      one workgroup, from the last frame tile to the first.  Going back r frames from state s at the tile's last
//                   frame the path stays inside [s - 2r, s], and alpha of such a cell n - r frames after the checkpoint depends on
//                   the checkpoint inside [s - 2n, s] only.  So the window [s - 2n, s], 2n + 1 <= 129 states, is enough: the
//                   workgroup reloads it, runs the tile's n frames again with one backpointer byte per cell in LDS, and one lane
//                   walks them and writes each token's start and end as it leaves the token's state.
//   along_means     per token the mean of p over its span, frames in order, as align_kernel's last loop.
// Every alpha cell that is stored or walked is computed from the same operands by the same operations as in align_kernel, so
// with both ends costly the results are dsmi_align's bit for bit, whatever W and F.
#include "align_long.h"
#include "ctc_trellis.h"

namespace dsmi {

namespace {

constexpr int NT = kAlongThreads;
constexpr int kFree = 1 << 9;           // state word: a free blank, lp = 0 (bits 0-7 label, bit 8 skip: ctc_blank_interleaved's)
using Feeder = CtcFeeder<float, NT>;

__device__ __forceinline__ int along_word(const AlongArgs& a, int s) {
    if (s & 1) {
        const int j = s >> 1;
        return a.targets[j] | (j >= 1 && a.targets[j - 1] != a.targets[j] ? 256 : 0);
    }
    return a.blank | ((s == 0 && a.lead_free) || (s == a.S - 1 && a.tail_free) ? kFree : 0);
}

// The frames t0 + 1 .. t0 + n of the states base .. base + nw - 1 (base may be negative: states below 0 stay -inf), from the
// checkpoint row `in` of frame t0.  al0 / al1: LDS rows of nw floats behind two guards each; lsk: nw state words; with BP one
// backpointer byte per cell in bp[r * PITCH + x], r = 0 for frame t0 + 1.  Returns the row of frame t0 + n, behind a barrier.
template <bool BP, int PITCH>
__device__ __forceinline__ const float* along_run(const AlongArgs& a, const int base, const int nw, const int t0, const int n, const float* in,
                                                  float* al0, float* al1, int* lsk, float (*lpc)[Feeder::kImage], unsigned char* bp,
                                                  const int tid) {
    const int x_lo = base < 0 ? -base : 0;
    for (int x = tid; x < nw; x += NT) {
        const int s = base + x;
        if (s >= 0) lsk[x] = along_word(a, s);
        al0[x] = s >= 0 ? in[s] : -INFINITY;
        al1[x] = -INFINITY;
    }
    if (tid < 2) al0[tid - 2] = al1[tid - 2] = -INFINITY;
    const float* P = a.probs + (size_t)(t0 + 1) * a.C;
    const int C = a.C;
    Feeder feed(P, n, C, tid);
    feed.prologue(lpc);
    __syncthreads();
    for (int r = 0; r < n; ++r) {
        const float* prev = (r & 1) ? al1 : al0;
        float* cur = (r & 1) ? al0 : al1;
        const float* lpt = feed.frame(lpc, r);
        for (int x = x_lo + tid; x < nw; x += NT) {
            const int q = lsk[x];
            const float a0 = prev[x], a1 = prev[x - 1], a2 = prev[x - 2];
            const float l = (q & kFree) ? 0.f : lpt[q & 255];
            float best = a0;
            int k = 0;
            if (a1 > best) { best = a1; k = 1; }
            if ((q & 256) && a2 > best) { best = a2; k = 2; }
            cur[x] = best + l;
            if constexpr (BP) bp[r * PITCH + x] = (unsigned char)k;
        }
        feed.end_of_frame(lpc, r);
        __syncthreads();
    }
    return (n & 1) ? al1 : al0;
}

__global__ void __launch_bounds__(NT) along_first(AlongArgs a) {
    const int s = blockIdx.x * NT + threadIdx.x;
    if (s >= a.S) return;
    float v = -INFINITY;
    if (s < 2) {
        const int q = along_word(a, s);
        v = (q & kFree) ? 0.f : logf(fmaxf(a.probs[q & 255], FLT_MIN));
    }
    a.rows[s] = v;
}

template <int W, int F>
__global__ void __launch_bounds__(NT) along_forward(AlongArgs a, int j) {
    __shared__ float al[2][W + 2 * F + 2];
    __shared__ int lsk[W + 2 * F];
    __shared__ float lpc[2][Feeder::kImage];
    const int tid = threadIdx.x;
    const int s0 = blockIdx.x * W, s1 = min(s0 + W, a.S), base = s0 - 2 * F;
    const int t0 = j * F, n = min(F, a.T - 1 - t0);
    float* out = a.rows + (size_t)(j + 1) * a.S;
    if (base > 2 * t0 + 1) {            // no path has reached the window at frame t0
        for (int s = s0 + tid; s < s1; s += NT) out[s] = -INFINITY;
        return;
    }
    const float* fin = along_run<false, 0>(a, base, s1 - base, t0, n, a.rows + (size_t)j * a.S, al[0] + 2, al[1] + 2, lsk, lpc, nullptr, tid);
    for (int s = s0 + tid; s < s1; s += NT) out[s] = fin[s - base];
}

template <int F>
__global__ void __launch_bounds__(NT) along_back(AlongArgs a) {
    constexpr int kBack = 2 * F + 1, kPitch = (kBack + 3) & ~3;      // the window's states; bytes of a backpointer row
    __shared__ float al[2][kBack + 3];
    __shared__ int lsk[kBack];
    __shared__ float lpc[2][Feeder::kImage];
    __shared__ unsigned char bp[F * kPitch];
    __shared__ int s_cur;
    const int tid = threadIdx.x;
    if (tid == 0) {                     // the end state: the trailing blank unless the last token is strictly better
        const float* fin = a.rows + (size_t)a.frame_tiles * a.S;
        int s = a.S - 1;
        float v = fin[a.S - 1];
        if (a.L > 0 && fin[a.S - 2] > v) { s = a.S - 2; v = fin[a.S - 2]; }
        a.path_logp[0] = v;
        s_cur = s;
    }
    __syncthreads();
    // (lane 0) `seen` = the state of the frame after the one being walked: a token's end is written on entering its state from
    // the right, its start on leaving it to the left
    int seen = -1;
    auto visit = [&](int s, int t) {
        if (s != seen) {
            if (seen >= 0 && (seen & 1)) a.spans[2 * (seen >> 1)] = t + 1;
            if (s & 1) a.spans[2 * (s >> 1) + 1] = t + 1;
        }
        seen = s;
    };
    for (int j = a.frame_tiles - 1; j >= 0; --j) {
        int s = s_cur;
        const int t0 = j * F, n = min(F, a.T - 1 - t0), base = s - 2 * n;
        along_run<true, kPitch>(a, base, 2 * n + 1, t0, n, a.rows + (size_t)j * a.S, al[0] + 2, al[1] + 2, lsk, lpc, bp, tid);
        if (tid == 0) {
            for (int r = n - 1; r >= 0; --r) {
                visit(s, t0 + 1 + r);
                s -= bp[r * kPitch + (s - base)];
            }
            s_cur = s;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int s = s_cur;
        visit(s, 0);
        if (s & 1) a.spans[2 * (s >> 1)] = 0;
    }
}

__global__ void __launch_bounds__(NT) along_means(AlongArgs a) {
    const int k = blockIdx.x * NT + threadIdx.x;
    if (k >= a.L) return;
    const int t0 = a.spans[2 * k], t1 = a.spans[2 * k + 1], lab = a.targets[k];
    float sum = 0.f;
    for (int t = t0; t < t1; ++t) sum += a.probs[(size_t)t * a.C + lab];
    a.token_probs[k] = sum / (float)(t1 - t0);
}

template <int W, int F>
hipError_t launch_form(const AlongArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(along_first, dim3((a.S + NT - 1) / NT), dim3(NT), 0, s, a);
    for (int j = 0; j < a.frame_tiles; ++j) hipLaunchKernelGGL((along_forward<W, F>), dim3(a.state_tiles), dim3(NT), 0, s, a, j);
    hipLaunchKernelGGL((along_back<F>), dim3(1), dim3(NT), 0, s, a);
    if (a.L > 0) hipLaunchKernelGGL(along_means, dim3((a.L + NT - 1) / NT), dim3(NT), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_align_long(const AlongArgs& a, hipStream_t s) {
#ifdef DSMI_EXPERIMENTS
    // the geometries that were measured and not adopted (ctc_tools.hip: DSMI_DEBUG_ALONG_FORM)
    if (a.W == 1792 && a.F == 128) return launch_form<1792, 128>(a, s);
    if (a.W == 896 && a.F == 64) return launch_form<896, 64>(a, s);
    if (a.W == 128 && a.F == 64) return launch_form<128, 64>(a, s);
#endif
    return launch_form<kAlongW, kAlongF>(a, s);
}

}  // namespace dsmi
