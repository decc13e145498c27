// CTC occupancy on the GPU (gfx950): for candidate transcript y of L tokens on T frames, the posterior that frame t is emitted
// by token k, tok[t][k], or carries label c, occ[t][c], given that the model emits y -- the product of score.hip's alpha and
// alt.hip's beta, in float64 throughout (the contract: include/dsmi.h).
//
// With alpha_t(s) as in score.hip, beta_t(s) the log probability of finishing from state s at frame t, frame t's emission
// included, and logp the transcript's log likelihood:
//     gamma_t(s) = exp(alpha_t(s) + beta_t(s) - lp(t, label(s)) - logp)         (0 where alpha or beta is -inf)
//     tok[t][k]  = gamma_t(2k + 1)
//     occ[t][c]  = the sum of gamma_t(s) over the states with label(s) == c
//
// Two launches, the second behind the first on the stream; no workgroup waits for another.
// occ_trellis_kernel: two workgroups per candidate in the order of score_plan, as alt_trellis_kernel has them: the even one the
// forward pass in the form of score_kernel (two rows in LDS, one barrier per frame, CtcFeeder), the odd one its mirror image from
// the last frame down (CtcFeederDown).  The forward pass writes every alpha_t(s) and logp, the backward pass every
// beta_t(s) - lp(t, label(s)), the log-sum-exp as it stands before the emission is added: the two stored trellises.  A pass
// stores and never loads, so its chain from barrier to barrier waits for no global memory; forming gamma in the backward pass
// from alpha loaded a frame ahead was measured and was slower.  No state is cut to those on a complete path: the
// other pass's trellis has them all, and -inf is what makes their gamma 0.
// occ_out_kernel: one thread per element of occ and of tok, over the caller's whole arrays, zeros included (rows past the clip's
// frames, columns past the transcript, infeasible candidates); it forms the gammas it needs, one exp each.  A label's sum runs
// over the candidate's own tokens in the order of k (the blank's over its L + 1 states in the order of s) in one thread: the
// order is fixed by the transcript alone, there is no atomic, and the reduction is off the frame chain.  At most
// L + 1 <= T + 1 terms of sum <= 1 add (L + 1) 2^-53, far inside the bound.
//
// Everything a candidate's workgroups and output threads compute depends on its own tokens and frames alone, so its results are
// the same bits whatever else is in the launch.
#include "occ.h"
#include "ctc_trellis.h"

namespace dsmi {

constexpr int kOccImage = kCtcChunk * kCtcMaxLabels;

__device__ __forceinline__ double occ_lse3(double a, double b, double c) {      // (score.hip's)
    const double m = fmax(a, fmax(b, c));
    const double u = a == m ? b : a;
    const double v = a == m ? c : (b == m ? c : b);
    const double r = m + log1p(exp(u - m) + exp(v - m));
    return m == -INFINITY ? m : r;       // (-inf - -inf is NaN: nothing of r is kept then)
}

// One pass of candidate n over its frames: rows [2][S_max + 4] in LDS, each between two -inf guards on either side, then per
// state its label | (may skip from s-2) << 8 [S_max].
template <bool Back>
__device__ __forceinline__ void occ_pass(const OccArgs& a, int n, double (*lpc)[kOccImage], double* carve) {
    constexpr int NT = kOccThreads;
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
    const size_t base = (size_t)a.base[n];
    ctc_blank_interleaved<double, NT>(a.targets + (size_t)n * a.L_stride, S, a.blank, tid, lsk, r0, r1);
    if (tid < 2) r0[S + tid] = r1[S + tid] = -INFINITY;

    if constexpr (!Back) {
        CtcFeeder<double, NT> feed(P, T, C, tid);
        feed.prologue(lpc);
        __syncthreads();
        double* const fw = a.fwd + base;                        // [t][s]: alpha_t(s)
        for (int s = tid; s < S; s += NT) {
            const double v = s < 2 ? lpc[0][lsk[s] & 255] : -INFINITY;
            r0[s] = v;
            r1[s] = -INFINITY;
            fw[s] = v;
        }
        __syncthreads();
        for (int t = 1; t < T; ++t) {
            const double* prev = (t & 1) ? r0 : r1;
            double* cur = (t & 1) ? r1 : r0;
            const double* lpt = feed.frame(lpc, t);
            double* const row = fw + (size_t)t * S;
            for (int s = tid; s < S; s += NT) {
                const int q = lsk[s];
                const double v = occ_lse3(prev[s], prev[s - 1], (q >> 8) ? prev[s - 2] : -INFINITY) + lpt[q & 255];
                cur[s] = v;
                row[s] = v;
            }
            feed.end_of_frame(lpc, t);
            __syncthreads();
        }
        if (tid == 0) {
            const double* fin = ((T - 1) & 1) ? r1 : r0;
            a.logp[n] = occ_lse3(fin[S - 1], fin[S - 2], -INFINITY);      // (the guard at -1 when there is no token)
        }
    } else {
        CtcFeederDown<double, NT> feed(P, T, C, tid);
        feed.prologue(lpc);
        __syncthreads();
        double* const bw = a.bwd + base;                        // [t][s]: beta_t(s) - lp(t, label(s))
        {
            double* top = ((T - 1) & 1) ? r1 : r0;
            double* other = ((T - 1) & 1) ? r0 : r1;
            const double* lpt = feed.frame(lpc, T - 1);
            for (int s = tid; s < S; s += NT) {
                const bool ends = s >= S - 2;                   // a path ends in the trailing blank or the last token
                top[s] = ends ? lpt[lsk[s] & 255] : -INFINITY;
                other[s] = -INFINITY;
                bw[(size_t)(T - 1) * S + s] = ends ? 0.0 : -INFINITY;
            }
            feed.end_of_frame(lpc, T - 1);
            __syncthreads();
        }
        for (int t = T - 2; t >= 0; --t) {
            const double* prev = (t & 1) ? r0 : r1;             // frame t + 1's row
            double* cur = (t & 1) ? r1 : r0;
            const double* lpt = feed.frame(lpc, t);
            double* const row = bw + (size_t)t * S;
            for (int s = tid; s < S; s += NT) {
                const int q = lsk[s];
                const bool skip = (s & 1) && s + 2 < S && (lsk[s + 2] >> 8);
                const double r = occ_lse3(prev[s], prev[s + 1], skip ? prev[s + 2] : -INFINITY);
                cur[s] = r + lpt[q & 255];
                row[s] = r;
            }
            feed.end_of_frame(lpc, t);
            __syncthreads();
        }
    }
}

// Workgroups 2i and 2i + 1: the forward and the backward pass of candidate order[i]; with no array asked for (a.both false)
// workgroup i is the forward pass of candidate order[i], for logp alone.
__global__ void __launch_bounds__(kOccThreads) occ_trellis_kernel(OccArgs a) {
    extern __shared__ double occ_carve[];
    __shared__ double lpc[2][kOccImage];           // chunk j in lpc[j & 1] (counted from the last chunk in the backward pass), [frame][label]
    const int n = a.order[a.both ? blockIdx.x >> 1 : blockIdx.x];
    if (a.both && (blockIdx.x & 1)) occ_pass<true>(a, n, lpc, occ_carve);
    else occ_pass<false>(a, n, lpc, occ_carve);
}

// gamma_t(s) of candidate n from the two stored trellises, i = its base + t * S + s
__device__ __forceinline__ double occ_gamma(const OccArgs& a, size_t i, double logp) {
    return exp(a.fwd[i] + a.bwd[i] - logp);        // (-inf where either is: exp gives 0; nothing here is +inf)
}

// The caller's arrays in full: element i of occ [N][T_out][C], then element i of tok [N][T_out][L_stride].
__global__ void __launch_bounds__(kOccThreads) occ_out_kernel(OccArgs a) {
    const size_t step = (size_t)gridDim.x * kOccThreads, first = (size_t)blockIdx.x * kOccThreads + threadIdx.x;
    if (a.occ) {
        const size_t C = (size_t)a.C, per = (size_t)a.T_out * C, total = (size_t)a.N * per;
        for (size_t i = first; i < total; i += step) {
            const int n = (int)(i / per), t = (int)(i % per / C), c = (int)(i % C);
            const int L = a.tlen[n];
            double v = 0.0;
            if (L >= 0 && t < a.sizes[a.cand_clip[n]]) {
                const size_t g = (size_t)a.base[n] + (size_t)t * (2 * L + 1);
                const double logp = a.logp[n];
                if (c == a.blank) {
                    for (int k = 0; k <= L; ++k) v += occ_gamma(a, g + 2 * k, logp);
                } else {
                    const int32_t* tg = a.targets + (size_t)n * a.L_stride;
                    for (int k = 0; k < L; ++k)
                        if (tg[k] == c) v += occ_gamma(a, g + 2 * k + 1, logp);
                }
            }
            a.occ[i] = v;
        }
    }
    if (a.tok && a.L_stride > 0) {
        const size_t Ls = (size_t)a.L_stride, per = (size_t)a.T_out * Ls, total = (size_t)a.N * per;
        for (size_t i = first; i < total; i += step) {
            const int n = (int)(i / per), t = (int)(i % per / Ls), k = (int)(i % Ls);
            const int L = a.tlen[n];
            double v = 0.0;
            if (k < L && t < a.sizes[a.cand_clip[n]]) v = occ_gamma(a, (size_t)a.base[n] + (size_t)t * (2 * L + 1) + 2 * k + 1, a.logp[n]);
            a.tok[i] = v;
        }
    }
}

size_t occ_lds_bytes(int S_max) {
    return sizeof(double) * 2 * ((size_t)S_max + 4) + sizeof(int) * (size_t)S_max;
}

hipError_t launch_occ(const OccArgs& a, hipStream_t s) {
    const size_t lds = occ_lds_bytes(a.S_max);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(occ_trellis_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(occ_trellis_kernel, dim3((a.both ? 2u : 1u) * (unsigned)a.N), dim3(kOccThreads), lds, s, a);
    e = hipGetLastError();
    if (e != hipSuccess || !a.both) return e;
    const size_t most = (size_t)a.N * a.T_out * (size_t)max(a.occ ? a.C : 0, a.tok ? a.L_stride : 0);
    const size_t blocks = std::min<size_t>((most + kOccThreads - 1) / kOccThreads, (size_t)1 << 20);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(occ_out_kernel, dim3((unsigned)blocks), dim3(kOccThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace dsmi
