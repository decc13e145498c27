// CTC token confidence on the GPU (gfx950): for candidate transcript y of L tokens and every slot k, label c, the natural log of
// the probability that the CTC model emits exactly y with token k replaced by c (c = blank: token k deleted) -- what score.hip's
// recurrence gives for that variant, for all L * C variants out of one forward-backward pass, in float64 throughout (the contract:
// include/dsmi.h).
//
// With alpha_t(s) as in score.hip and beta_t(s) the log probability of finishing from state s at frame t, frame t's emission
// included, a path of the variant stays in the slot's own state for some frames, enters it from the states before token k and
// leaves it into the states behind token k, all of which the variant shares with y:
//     substitution:  u_t = logsumexp(u_{t-1}, alpha_{t-1}(2k), alpha_{t-1}(2k-1) [k >= 1, c != y_{k-1}]) + lp(t, c),  u_0 = lp(0, c) [k = 0]
//                    value = logsumexp over t of u_t + logsumexp(beta_{t+1}(2k+2), beta_{t+1}(2k+3) [k+1 < L, y_{k+1} != c])
//                    (k = L - 1: u_{T-1} joins, the path may end in the slot)
//     deletion:      value = logsumexp over t of logsumexp(alpha_t(2k), alpha_t(2k-1) [k >= 1, y_{k-1} != y_{k+1}]) + beta_{t+1}(2k+3)
//                    (k = 0: beta_0(3) joins; k = L - 1: logsumexp(alpha_{T-1}(2k), alpha_{T-1}(2k-1)) alone)
// Every path leaves the slot exactly once, so nothing is counted twice, and a variant that cannot fit the frames comes out -inf.
//
// Two launches.  alt_trellis_kernel: two workgroups per candidate in the order of score_plan, the even one the forward pass in
// the form of score_kernel, the odd one its mirror image from the last frame down (CtcFeederDown); both keep two rows in LDS, take
// one barrier per frame and write what the slots need to the workspace.  The pair sums come for nothing: a blank state has no
// skip, so the log-sum-exp inside alpha_{t+1}(2k) is logsumexp(alpha_t(2k), alpha_t(2k-1)), and the one inside beta_{t-1}(2k+2)
// is logsumexp(beta_t(2k+2), beta_t(2k+3)).  Neither pass cuts the states to those on a complete path as score_kernel does: the
// slots read states that lie on no path of y.  alt_slot_kernel: one thread per (k, c), 256 of them per workgroup; per frame a
// thread reads one stored entry value and one stored exit value (the lanes of one k read the same address), takes one
// log-sum-exp of two and adds one term to a running sum kept as (largest term, sum of exp(term - largest)): two exp and one
// log1p per frame.  The chains are independent; the only barrier is the feeder's, once per chunk of frames.
//
// Everything a candidate's workgroups compute depends on its own tokens and frames alone, so its results are the same bits
// whatever else is in the launch.
#include "alt.h"
#include "ctc_trellis.h"

namespace dsmi {

constexpr int kAltImage = kCtcChunk * kCtcMaxLabels;

__device__ __forceinline__ double alt_lse3(double a, double b, double c) {      // (score.hip's)
    const double m = fmax(a, fmax(b, c));
    const double u = a == m ? b : a;
    const double v = a == m ? c : (b == m ? c : b);
    const double r = m + log1p(exp(u - m) + exp(v - m));
    return m == -INFINITY ? m : r;       // (-inf - -inf is NaN: nothing of r is kept then)
}

__device__ __forceinline__ double alt_lse2(double a, double b) {
    const double m = fmax(a, b);
    const double r = m + log1p(exp(fmin(a, b) - m));
    return m == -INFINITY ? m : r;
}

// log of a sum of exp(x): the largest x so far and the sum of exp(x - largest); one exp per term
struct AltSum {
    double m = -INFINITY, sum = 0.0;
    __device__ __forceinline__ void add(double x) {
        if (x > -INFINITY) {
            const double d = x - m, e = exp(-fabs(d));          // (the first term: d = +inf, e = 0)
            if (d > 0) { sum = sum * e + 1.0; m = x; }
            else sum += e;
        }
    }
    __device__ __forceinline__ double value() const { return sum > 0.0 ? m + log(sum) : -INFINITY; }
};

// One pass of candidate n over its frames: rows [2][S_max + 4] in LDS, each between two -inf guards on either side, then per
// state its label | (may skip from s-2) << 8 [S_max].
template <bool Back>
__device__ __forceinline__ void alt_trellis_pass(const AltArgs& a, int n, double (*lpc)[kAltImage], double* carve) {
    constexpr int NT = kAltThreads;
    const int tid = threadIdx.x;
    const int L = a.tlen[n];
    if (L < 0) return;                   // infeasible: told by the host, nothing written
    const int b = a.cand_clip[n];
    const int T = a.sizes[b], S = 2 * L + 1, C = a.C;
    if (T == 0) {                        // (only an empty transcript is feasible without frames)
        if (!Back && tid == 0) a.logp[n] = 0.0;
        return;
    }
    const int R = a.S_max + 4;
    double* const r0 = carve + 2;
    double* const r1 = carve + R + 2;
    int* const lsk = reinterpret_cast<int*>(carve + 2 * R);
    const float* P = a.probs + (size_t)b * a.T_out * C;
    const int32_t* tg = a.targets + (size_t)n * a.L_stride;
    const size_t base = (size_t)a.base[n];
    ctc_blank_interleaved<double, NT>(tg, S, a.blank, tid, lsk, r0, r1);
    if (tid < 2) r0[S + tid] = r1[S + tid] = -INFINITY;

    if constexpr (!Back) {
        CtcFeeder<double, NT> feed(P, T, C, tid);
        feed.prologue(lpc);
        __syncthreads();
        double* const fw = a.fwd + base;                        // [t][k][2], k < L: state 2k is s, its pair sum s + 1
        for (int s = tid; s < S; s += NT) {
            const double v = s < 2 ? lpc[0][lsk[s] & 255] : -INFINITY;
            r0[s] = v;
            r1[s] = -INFINITY;
            if (!(s & 1) && s < S - 1) fw[s] = v;
        }
        __syncthreads();
        for (int t = 1; t < T; ++t) {
            const double* prev = (t & 1) ? r0 : r1;
            double* cur = (t & 1) ? r1 : r0;
            const double* lpt = feed.frame(lpc, t);
            double* const row = fw + (size_t)t * 2 * L;
            for (int s = tid; s < S; s += NT) {
                const int q = lsk[s];
                const double r = alt_lse3(prev[s], prev[s - 1], (q >> 8) ? prev[s - 2] : -INFINITY);
                const double v = r + lpt[q & 255];
                cur[s] = v;
                if (!(s & 1) && s < S - 1) {
                    row[s - 2 * L + 1] = r;                     // frame t - 1's pair sum
                    row[s] = v;
                }
            }
            feed.end_of_frame(lpc, t);
            __syncthreads();
        }
        const double* fin = ((T - 1) & 1) ? r1 : r0;
        for (int s = tid; s < S - 1; s += NT)
            if (!(s & 1)) fw[(size_t)(T - 1) * 2 * L + s + 1] = alt_lse3(fin[s], fin[s - 1], -INFINITY);
        if (tid == 0) a.logp[n] = alt_lse3(fin[S - 1], fin[S - 2], -INFINITY);
    } else {
        CtcFeederDown<double, NT> feed(P, T, C, tid);
        feed.prologue(lpc);
        __syncthreads();
        double* const bw = a.bwd + base;                        // [t][s]
        double* const bp = a.bwd_pair + base / 2;               // [t][k], k < L: the pair sum of states 2k + 2 and 2k + 3
        {
            double* top = ((T - 1) & 1) ? r1 : r0;
            double* other = ((T - 1) & 1) ? r0 : r1;
            const double* lpt = feed.frame(lpc, T - 1);
            for (int s = tid; s < S; s += NT) {
                const double v = s >= S - 2 ? lpt[lsk[s] & 255] : -INFINITY;
                top[s] = v;
                other[s] = -INFINITY;
                bw[(size_t)(T - 1) * S + s] = v;
            }
            feed.end_of_frame(lpc, T - 1);
            __syncthreads();
        }
        for (int t = T - 2; t >= 0; --t) {
            const double* prev = (t & 1) ? r0 : r1;             // frame t + 1's row
            double* cur = (t & 1) ? r1 : r0;
            const double* lpt = feed.frame(lpc, t);
            for (int s = tid; s < S; s += NT) {
                const int q = lsk[s];
                const bool skip = (s & 1) && s + 2 < S && (lsk[s + 2] >> 8);
                const double r = alt_lse3(prev[s], prev[s + 1], skip ? prev[s + 2] : -INFINITY);
                const double v = r + lpt[q & 255];
                cur[s] = v;
                bw[(size_t)t * S + s] = v;
                if (!(s & 1) && s >= 2) bp[(size_t)(t + 1) * L + (s - 2) / 2] = r;
            }
            feed.end_of_frame(lpc, t);
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(kAltThreads) alt_trellis_kernel(AltArgs a) {
    extern __shared__ double alt_carve[];
    __shared__ double lpc[2][kAltImage];           // chunk j in lpc[j & 1] (counted from the last chunk in the backward pass), [frame][label]
    const int n = a.order[blockIdx.x >> 1];
    if (blockIdx.x & 1) alt_trellis_pass<true>(a, n, lpc, alt_carve);
    else alt_trellis_pass<false>(a, n, lpc, alt_carve);
}

__global__ void __launch_bounds__(kAltThreads) alt_slot_kernel(AltArgs a) {
    __shared__ double lpc[2][kAltImage];
    constexpr int NT = kAltThreads;
    const int n = a.order[blockIdx.x / a.n_blocks], blk = blockIdx.x % a.n_blocks, tid = threadIdx.x;
    const int L = a.tlen[n], C = a.C;
    if (L <= 0 || blk * NT >= L * C) return;                    // (the whole workgroup)
    const int b = a.cand_clip[n];
    const int T = a.sizes[b], S = 2 * L + 1;                    // T >= 1: a feasible token has a frame
    const bool live = blk * NT + tid < L * C;                   // the others walk slot 0 along for the feeder and write nothing
    const int i = live ? blk * NT + tid : 0, k = i / C, c = i % C;
    const int32_t* tg = a.targets + (size_t)n * a.L_stride;
    const int before = k >= 1 ? tg[k - 1] : -1, after = k + 1 < L ? tg[k + 1] : -1;
    const bool del = c == a.blank, last = k == L - 1;
    const size_t base = (size_t)a.base[n];
    const float* P = a.probs + (size_t)b * a.T_out * C;

    // the entry value of frame t: alpha_t(2k), or the pair sum with alpha_t(2k-1) where the token before may hand over directly
    const bool wide = k >= 1 && (del ? last || before != after : c != before);
    const double* const en = a.fwd + base + 2 * k + (wide ? 1 : 0);
    const size_t en_stride = 2 * (size_t)L;
    const int en_lag = del ? 0 : 1;                             // a substitution's frame t enters from frame t - 1
    // the exit value of frame t: beta_t(2k+3) behind a deletion; beta_t(2k+2), or its pair sum with beta_t(2k+3)
    const double* ex;
    size_t ex_stride;
    if (del) { ex = a.bwd + base + (last ? 2 * k + 2 : 2 * k + 3); ex_stride = S; }      // (last: no exit is read for a value)
    else if (!last && after != c) { ex = a.bwd_pair + base / 2 + k; ex_stride = L; }
    else { ex = a.bwd + base + 2 * k + 2; ex_stride = S; }

    CtcFeeder<double, NT> feed(P, T, C, tid);
    feed.prologue(lpc);
    __syncthreads();
    AltSum acc;
    if (del && k == 0 && !last) acc.add(a.bwd[base + 3]);       // the deleted token's slot may be empty from frame 0 on
    double u = -INFINITY;
    double en_next = en[0], ex_next = ex[(size_t)min(1, T - 1) * ex_stride];       // loaded one frame ahead of their use
    for (int t = 0; t < T; ++t) {
        const double en_t = en_next, ex_t = ex_next;            // entry of frame t - en_lag, exit of frame t + 1
        en_next = en[(size_t)max(min(t + 1, T - 1) - en_lag, 0) * en_stride];
        ex_next = ex[(size_t)min(t + 2, T - 1) * ex_stride];
        const double* lpt = feed.frame(lpc, t);
        if (del) u = en_t;
        else u = t == 0 ? (k == 0 ? lpt[c] : -INFINITY) : alt_lse2(u, en_t) + lpt[c];
        if (t < T - 1) {
            if (!(del && last)) acc.add(u + ex_t);
        } else if (!del && last) {
            acc.add(u);
        }
        feed.end_of_frame(lpc, t);
        if ((t + 1) % kCtcChunk == 0) __syncthreads();          // the feeder's images change hands once per chunk
    }
    const double value = del && last ? en[(size_t)(T - 1) * en_stride] : acc.value();
    if (live) a.alt[((size_t)n * a.L_stride + k) * C + c] = value;
}

size_t alt_lds_bytes(int S_max) {
    return sizeof(double) * 2 * ((size_t)S_max + 4) + sizeof(int) * (size_t)S_max;
}

hipError_t launch_alt(const AltArgs& a, int N, hipStream_t s) {
    const size_t lds = alt_lds_bytes(a.S_max);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(alt_trellis_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(alt_trellis_kernel, dim3(2 * (unsigned)N), dim3(kAltThreads), lds, s, a);
    e = hipGetLastError();
    if (e != hipSuccess || a.n_blocks == 0) return e;
    hipLaunchKernelGGL(alt_slot_kernel, dim3((unsigned)N * (unsigned)a.n_blocks), dim3(kAltThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dsmi
