// CTC forced alignment on the GPU (gfx950): for each clip, the most probable frame-level path through the CTC trellis of a
// transcript the caller already has, its per-token frame spans, per-token mean probabilities and its log probability.
//
// The extended sequence of a clip with L tokens t_1..t_L has S = 2L + 1 states: blank, t_1, blank, t_2, ..., blank (state
// 2k + 1 is token k).  With lp(t, c) = logf(fmaxf(p(t, c), FLT_MIN)), accumulated in fp32:
//     alpha_0(0) = lp(0, blank), alpha_0(1) = lp(0, t_1), every other state -inf
//     alpha_t(s) = max(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2) [token state, label(s) != label(s-2)]) + lp(t, label(s))
// Ties (include/dsmi.h, and tests/_align_ref.py implements the same rule): predecessor s before s-1 before s-2; at the end the
// trailing blank S-1 before the last token S-2.
//
// One workgroup per clip.  The two alpha rows live in LDS, double-buffered, so a frame costs one barrier; each thread owns the
// states tid, tid + 256, ... and reads a state's three predecessors and its packed label / skip word at once.  The
// probabilities arrive as lp in LDS a chunk of frames ahead (CtcFeeder, ctc_trellis.h), so the chain from barrier to barrier is
// LDS work only.  Each (t, s) leaves a one-byte backpointer (0, 1, 2: how far the state fell) in a device workspace
// [B][T_out][S_stride].  The backtrace stays on the GPU: going back 64 frames lowers the state by at most 126, so the workgroup
// stages the backpointers of frames t-63..t and states s-126..s (64 rows x 132 bytes) into LDS with one cooperative load and one
// lane walks the 64 steps from there -- one dependent global round trip per 64 frames, not per frame.
#include "align.h"
#include "ctc_trellis.h"

namespace dsmi {

__global__ void __launch_bounds__(kAlignThreads) align_kernel(AlignArgs a) {
    // alpha rows [2][S_max + 2], each behind two -inf guards so that s-1 and s-2 are always readable (later: spans start[L] /
    // end[L]), then per state its label | (may skip from s-2) << 8 [S_max]
    extern __shared__ float carve[];
    using Feeder = CtcFeeder<float, kAlignThreads>;
    __shared__ float lpc[2][Feeder::kImage];      // chunk j in lpc[j & 1], [frame][label]
    __shared__ uint32_t tile[kAlignTile * kAlignTileCols];
    __shared__ int s_cur;
    constexpr int NT = kAlignThreads;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = a.tlen[b];
    if (L < 0) return;                   // infeasible: told by the host, nothing written
    const int T = a.sizes[b], S = 2 * L + 1, C = a.C;
    if (T == 0) {                        // (only an empty transcript is feasible without frames)
        if (tid == 0) a.path_logp[b] = 0.f;
        return;
    }
    float* const al0 = carve + 2;
    float* const al1 = carve + a.S_max + 4;
    int* const lsk = reinterpret_cast<int*>(carve + 2 * a.S_max + 4);
    const float* P = a.probs + (size_t)b * a.T_out * C;
    unsigned char* BP = a.bp + (size_t)b * a.T_out * a.S_stride;

    const int32_t* tg = a.targets + (size_t)b * a.L_stride;
    ctc_blank_interleaved<float, NT>(tg, S, a.blank, tid, lsk, al0, al1);
    Feeder feed(P, T, C, tid);
    feed.prologue(lpc);
    __syncthreads();
    for (int s = tid; s < S; s += NT) al0[s] = s < 2 ? lpc[0][lsk[s] & 255] : -INFINITY;
    __syncthreads();

    // ---- forward: alpha_t in al[t & 1], lp of frame t in feed.frame(lpc, t)[label]
    for (int t = 1; t < T; ++t) {
        const float* prev = (t & 1) ? al0 : al1;
        float* cur = (t & 1) ? al1 : al0;
        const float* lpt = feed.frame(lpc, t);
        unsigned char* row = BP + (size_t)t * a.S_stride;
        for (int s = tid; s < S; s += NT) {
            // every LDS read of the state at once, then lp of its label: two round trips, no branch
            const int q = lsk[s];
            const float a0 = prev[s], a1 = prev[s - 1], a2 = prev[s - 2];
            const float l = lpt[q & 255];
            float best = a0;
            int k = 0;
            if (a1 > best) { best = a1; k = 1; }
            if ((q >> 8) && a2 > best) { best = a2; k = 2; }
            cur[s] = best + l;
            row[s] = (unsigned char)k;
        }
        feed.end_of_frame(lpc, t);
        __syncthreads();
    }

    // ---- end state: the trailing blank unless the last token is strictly better
    if (tid == 0) {
        const float* fin = ((T - 1) & 1) ? al1 : al0;
        int s = S - 1;
        float v = fin[S - 1];
        if (L > 0 && fin[S - 2] > v) { s = S - 2; v = fin[S - 2]; }
        a.path_logp[b] = v;
        s_cur = s;
    }
    __syncthreads();

    // ---- backtrace in 64-frame tiles; the alpha rows are free now and hold the spans
    int* const st = reinterpret_cast<int*>(carve);
    int* const en = st + a.S_max + 2;
    int s = s_cur;
    int seen = -1;                       // (lane 0) the state of the frame after the one being walked
    for (int t_hi = T - 1; t_hi >= 0; t_hi -= kAlignTile) {
        const int t_lo = max(0, t_hi - (kAlignTile - 1));
        const int c0 = max(0, s - 2 * (kAlignTile - 1)) & ~3;
        const int n = (t_hi - t_lo + 1) * kAlignTileCols;
        __syncthreads();                 // the previous tile's walk is over and every thread has read s_cur
        for (int i = tid; i < n; i += NT) {
            const int r = i / kAlignTileCols, c = i - r * kAlignTileCols;
            tile[i] = *reinterpret_cast<const uint32_t*>(BP + (size_t)(t_lo + r) * a.S_stride + c0 + 4 * c);
        }
        __syncthreads();
        if (tid == 0) {
            const unsigned char* tb = reinterpret_cast<const unsigned char*>(tile);
            for (int t = t_hi; t >= t_lo; --t) {
                if (s & 1) {
                    const int k = s >> 1;
                    if (s != seen) en[k] = t + 1;
                    st[k] = t;
                }
                seen = s;
                if (t > 0) s -= tb[(t - t_lo) * (4 * kAlignTileCols) + (s - c0)];
            }
            s_cur = s;
        }
        __syncthreads();
        s = s_cur;
    }

    // ---- per token: its span and the mean of p(label) over it (fp32, frames in order)
    for (int k = tid; k < L; k += NT) {
        const int t0 = st[k], t1 = en[k], lab = lsk[2 * k + 1] & 255;
        float sum = 0.f;
        for (int t = t0; t < t1; ++t) sum += P[(size_t)t * C + lab];
        const size_t q = (size_t)b * a.L_stride + k;
        a.token_probs[q] = sum / (float)(t1 - t0);
        a.spans[2 * q] = t0;
        a.spans[2 * q + 1] = t1;
    }
}

size_t align_lds_bytes(int S_max) {
    return sizeof(float) * (2 * (size_t)S_max + 4) + sizeof(int) * (size_t)S_max;
}

hipError_t launch_align(const AlignArgs& a, int B, hipStream_t s) {
    const size_t lds = align_lds_bytes(a.S_max);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(align_kernel, dim3(B), dim3(kAlignThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace dsmi
