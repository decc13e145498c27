// CTC transcript scoring on the GPU (gfx950): for each candidate transcript of a clip, the natural log of the probability that
// the CTC model emits exactly that label sequence, summed over every frame-level alignment -- the forward recurrence of
// align.hip with a log-sum-exp in place of the max and no backpointers, in float64 throughout (the contract: include/dsmi.h).
//
// The states are align.hip's: S = 2L + 1 (blank, t_1, blank, ..., blank), state 2k + 1 is token k, the same skip rule and the
// same alpha_0.  With lp(t, c) = log((double)fmaxf(p(t, c), FLT_MIN)):
//     alpha_t(s) = logsumexp(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2) [token state, label(s) != label(s-2)]) + lp(t, label(s))
//     logp       = logsumexp(alpha_{T-1}(S-1), alpha_{T-1}(S-2))
// The log-sum-exp takes the largest argument m out, so that its term is exactly 1: m + log1p(exp(u - m) + exp(v - m)) for the
// two others; all -inf gives -inf.
//
// One workgroup per candidate, in the order of score_plan (ctc_host.h).  The two alpha rows live in LDS, double-buffered, so a
// frame costs one barrier; each thread owns the states tid, tid + 256, ...  The probabilities arrive as float64 lp in LDS a
// chunk of frames ahead (CtcFeeder, ctc_trellis.h), so the chain from barrier to barrier is LDS and ALU work only.  States on
// no complete path are not computed: state s cannot be reached before frame (s - 1) / 2 (their alpha is still the -inf both
// rows start with), and a state below S - 2 - 2 (T - 1 - t) cannot reach the end in the frames left (no later state reads
// it).  Both bounds depend on the candidate's own S and T only, so a candidate's result is the same bits whatever else is in
// the launch.
#include "score.h"
#include "ctc_trellis.h"

namespace dsmi {

__device__ __forceinline__ double score_lse3(double a, double b, double c) {
    const double m = fmax(a, fmax(b, c));
    const double u = a == m ? b : a;
    const double v = a == m ? c : (b == m ? c : b);
    const double r = m + log1p(exp(u - m) + exp(v - m));
    return m == -INFINITY ? m : r;       // (-inf - -inf is NaN: nothing of r is kept then)
}

__global__ void __launch_bounds__(kScoreThreads) score_kernel(ScoreArgs a) {
    // alpha rows [2][S_max + 2], each behind two -inf guards so that s-1 and s-2 are always readable, then per state its
    // label | (may skip from s-2) << 8 [S_max]
    extern __shared__ double score_carve[];
    using Feeder = CtcFeeder<double, kScoreThreads>;
    __shared__ double lpc[2][Feeder::kImage];      // chunk j in lpc[j & 1], [frame][label]
    constexpr int NT = kScoreThreads;
    const int n = a.order[blockIdx.x], tid = threadIdx.x;
    const int L = a.tlen[n];
    if (L < 0) return;                   // infeasible: told by the host, nothing written
    const int b = a.cand_clip[n];
    const int T = a.sizes[b], S = 2 * L + 1, C = a.C;
    if (T == 0) {                        // (only an empty transcript is feasible without frames)
        if (tid == 0) a.logp[n] = 0.0;
        return;
    }
    const int R = a.S_max + 2;
    double* const al0 = score_carve + 2;
    double* const al1 = score_carve + R + 2;
    int* const lsk = reinterpret_cast<int*>(score_carve + 2 * R);
    const float* P = a.probs + (size_t)b * a.T_out * C;

    const int32_t* tg = a.targets + (size_t)n * a.L_stride;
    ctc_blank_interleaved<double, NT>(tg, S, a.blank, tid, lsk, al0, al1);
    Feeder feed(P, T, C, tid);
    feed.prologue(lpc);
    __syncthreads();
    for (int s = tid; s < S; s += NT) {
        al0[s] = s < 2 ? lpc[0][lsk[s] & 255] : -INFINITY;
        al1[s] = -INFINITY;
    }
    __syncthreads();

    // ---- forward: alpha_t in al[t & 1], lp of frame t in feed.frame(lpc, t)[label]
    for (int t = 1; t < T; ++t) {
        const double* prev = (t & 1) ? al0 : al1;
        double* cur = (t & 1) ? al1 : al0;
        const double* lpt = feed.frame(lpc, t);
        // the states on a complete path: reachable by frame t, and able to reach S - 2 in the frames left
        const int hi = min(S - 1, 2 * t + 1), lo = max(0, S - 2 - 2 * (T - 1 - t));
        for (int s = tid + (max(lo - tid, 0) + NT - 1) / NT * NT; s <= hi; s += NT) {
            const int q = lsk[s];
            const double a0 = prev[s], a1 = prev[s - 1], a2 = (q >> 8) ? prev[s - 2] : -INFINITY;
            const double l = lpt[q & 255];
            cur[s] = score_lse3(a0, a1, a2) + l;
        }
        feed.end_of_frame(lpc, t);
        __syncthreads();
    }

    // ---- the end: the trailing blank and the last token (the guard at -1 when there is no token)
    if (tid == 0) {
        const double* fin = ((T - 1) & 1) ? al1 : al0;
        a.logp[n] = score_lse3(fin[S - 1], fin[S - 2], -INFINITY);
    }
}

size_t score_lds_bytes(int S_max) {
    return sizeof(double) * 2 * ((size_t)S_max + 2) + sizeof(int) * (size_t)S_max;
}

hipError_t launch_score(const ScoreArgs& a, int N, hipStream_t s) {
    const size_t lds = score_lds_bytes(a.S_max);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(score_kernel, dim3(N), dim3(kScoreThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace dsmi
