// CTC grammar decoding on the GPU (gfx950): for each clip, the most probable frame-level CTC path of any sentence that a token
// graph accepts -- the node visits of the path, their frame spans, per-visit mean probabilities and the path's log probability.
// The contract (the recurrence and its tie rule) is in include/dsmi.h; tests/_grammar_ref.py states it in numpy.
//
// Node n carries tok(n) and blk(n), the blank behind it; `lead` is the blank before the first token.  Per frame
//     ent(n)  = max{ lead [start]; per predecessor p in list order: blk(p), then tok(p) [label(p) != label(n)] }
//     tok'(n) = max(tok(n), ent(n) + w(n)) + lp(t, label(n));   blk'(n) = max(blk(n), tok(n)) + lp(t, blank);   lead' = lead + lp(t, blank)
// a later candidate replacing an earlier one only when strictly greater.  A chain graph is dsmi_align's trellis, candidate for
// candidate and addition for addition, so its results are align_kernel's bits.
//
// One workgroup per clip.  The clip's graph goes into LDS once: per node a word (label, start, final), its weight and its arc
// offset, per arc a 16-bit word (the predecessor and whether its tok may enter; the host packs it).  tok and blk of a node lie
// side by side as one 8-byte pair, two rows of pairs double-buffered, so a frame costs one barrier and a predecessor one LDS read.
// Each thread owns the nodes tid, tid + 256, ... and walks their predecessor lists; lead is the same register in every thread.
// The probabilities arrive as lp in LDS a chunk of frames ahead (CtcFeeder, ctc_trellis.h).  Each (t, n) leaves a 16-bit
// backpointer in a device workspace [B][T_out][node_stride]: where tok(n) came from (stay, lead, blk or tok of node p) and one
// bit for blk(n) (stayed, or came from tok(n)).
// The backtrace stays on the GPU, in one wave.  The path jumps between nodes at will, so no tile of neighbouring columns holds it
// (align.hip's does); but most steps stay in their node, and while the path is in tok(n) or blk(n) every code it needs is in
// column n.  The wave loads that column's codes of 64 frames at once, a lane per frame, finds by a ballot the first frame whose
// code leaves the node, and loads again from there: one dependent global round trip per node visit or 64 frames, not per frame.
#include "grammar.h"
#include "ctc_trellis.h"

#include <climits>

namespace dsmi {

__global__ void __launch_bounds__(kGrammarThreads) grammar_kernel(GrammarArgs a) {
    // tok / blk pairs [2][NS], node words [NS], weights [NS], arc offsets [NS + 4] and arcs [arc_words] of 16 bits
    extern __shared__ __align__(16) unsigned char carve[];
    using Feeder = CtcFeeder<float, kGrammarThreads>;
    __shared__ float lpc[2][Feeder::kImage];      // chunk j in lpc[j & 1], [frame][label]
    __shared__ float red_v[kGrammarThreads];
    __shared__ int red_i[kGrammarThreads];
    __shared__ int s_m;
    constexpr int NT = kGrammarThreads;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int T = a.sizes[b], C = a.C, g = a.clip_graph[b], NS = a.node_stride;
    const int n0 = a.node_off[g], N = a.node_off[g + 1] - n0;
    const int arc0 = a.arc_off[n0], NA = a.arc_off[n0 + N] - arc0;
    const bool empty_ok = a.empty_ok[g] != 0;
    if (T == 0) {                        // without frames only the empty sentence
        if (tid == 0) {
            a.path_logp[b] = empty_ok ? 0.f : -INFINITY;
            a.status[b] = empty_ok ? 0 : 1;
        }
        return;
    }
    float2* const row0 = reinterpret_cast<float2*>(carve);
    float2* const row1 = row0 + NS;
    int* const nodew = reinterpret_cast<int*>(row1 + NS);
    float* const wt = reinterpret_cast<float*>(nodew + NS);
    uint16_t* const aoff = reinterpret_cast<uint16_t*>(wt + NS);
    uint16_t* const arcs = aoff + NS + 4;
    const float* P = a.probs + (size_t)b * a.T_out * C;
    uint16_t* BP = a.bp + (size_t)b * a.T_out * NS;

    for (int n = tid; n < N; n += NT) { nodew[n] = a.words[n0 + n]; wt[n] = a.weights[n0 + n]; }
    for (int n = tid; n <= N; n += NT) aoff[n] = (uint16_t)(a.arc_off[n0 + n] - arc0);
    for (int j = tid; j < NA; j += NT) arcs[j] = a.arc_words16[arc0 + j];
    Feeder feed(P, T, C, tid);
    feed.prologue(lpc);
    __syncthreads();
    float lead = lpc[0][a.blank];
    for (int n = tid; n < N; n += NT) {
        const int q = nodew[n];
        row0[n] = make_float2((q & kGrammarStart) ? lpc[0][q & 255] + wt[n] : -INFINITY, -INFINITY);
    }
    __syncthreads();

    // ---- forward: the pairs of frame t in row[t & 1], lp of frame t in feed.frame(lpc, t)[label]
    for (int t = 1; t < T; ++t) {
        const float2* prev = (t & 1) ? row0 : row1;
        float2* cur = (t & 1) ? row1 : row0;
        const float* lpt = feed.frame(lpc, t);
        const float lb = lpt[a.blank];
        uint16_t* brow = BP + (size_t)t * NS;
        for (int n = tid; n < N; n += NT) {
            const int q = nodew[n];
            const float2 me = prev[n];
            const float w = wt[n], l = lpt[q & 255];
            const int j0 = aoff[n], j1 = aoff[n + 1];
            float ent = -INFINITY;
            int ecode = 0;
            if (q & kGrammarStart) { ent = lead; ecode = kGrammarLead << kGrammarKindShift; }
            for (int j = j0; j < j1; ++j) {
                const int aw = arcs[j], p = aw & kGrammarArcNode;
                const float2 pv = prev[p];
                if (pv.y > ent) { ent = pv.y; ecode = (kGrammarFromBlk << kGrammarKindShift) | p; }
                if ((aw & kGrammarArcTok) && pv.x > ent) { ent = pv.x; ecode = (kGrammarFromTok << kGrammarKindShift) | p; }
            }
            float best = me.x;
            int code = kGrammarStay << kGrammarKindShift;
            const float cand = ent + w;
            if (cand > best) { best = cand; code = ecode; }
            float bb = me.y;
            if (me.x > bb) { bb = me.x; code |= kGrammarBlkFromTok; }
            cur[n] = make_float2(best + l, bb + lb);
            brow[n] = (uint16_t)code;
        }
        lead += lb;
        feed.end_of_frame(lpc, t);
        __syncthreads();
    }

    // ---- the end: lead (when the empty sentence is accepted), then the final nodes ascending, blk before tok; the first of the
    // greatest wins.  Candidate index: 0 lead, 1 + 2n blk(n), 2 + 2n tok(n); a thread's own are ascending, then greatest value, least index
    {
        const float2* fin = ((T - 1) & 1) ? row1 : row0;
        float bv = -INFINITY;
        int bi = INT_MAX;
        if (tid == 0 && empty_ok) { bv = lead; bi = 0; }
        for (int n = tid; n < N; n += NT) {
            if (!(nodew[n] & kGrammarFinal)) continue;
            const float2 v = fin[n];
            if (v.y > bv) { bv = v.y; bi = 1 + 2 * n; }
            if (v.x > bv) { bv = v.x; bi = 2 + 2 * n; }
        }
        red_v[tid] = bv;
        red_i[tid] = bi;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const float v2 = red_v[tid + s];
                const int i2 = red_i[tid + s];
                if (v2 > red_v[tid] || (v2 == red_v[tid] && i2 < red_i[tid])) { red_v[tid] = v2; red_i[tid] = i2; }
            }
            __syncthreads();
        }
    }
    const float end_v = red_v[0];
    const int end_i = red_i[0];
    if (end_v == -INFINITY) {            // lp is finite, so -inf means that no accepted sentence fits the frames, and nothing else
        if (tid == 0) { a.path_logp[b] = -INFINITY; a.status[b] = 1; }
        return;
    }

    // ---- backtrace, wave 0: kind 0 = in tok(n) at frame t, 1 = in blk(n), 2 = in lead (every earlier frame too: over).  Visits
    // come out last first.
    int32_t* const pn = a.path_nodes + (size_t)b * a.T_out;
    int32_t* const ps = a.path_spans + 2 * (size_t)b * a.T_out;
    if (tid < 64) {
        int kind = 2, n = 0, t = T - 1, vend = T, M = 0;
        if (end_i > 0) { n = (end_i - 1) >> 1; kind = (end_i & 1) ? 1 : 0; }
#ifdef DSMI_EXPERIMENTS
        if (a.trace_form == 2) kind = 2; // (timing only: the forward pass alone, no path comes out)
        if (a.trace_form == 1) {         // one lane, one dependent load per frame: measured and not adopted
            while (tid == 0 && kind != 2 && t >= 0) {
                const int c = t >= 1 ? BP[(size_t)t * NS + n] : 0;
                if (kind == 1) {
                    if (t < 1) break;
                    if (c & kGrammarBlkFromTok) { kind = 0; vend = t; }
                } else {
                    const int kd = (c >> kGrammarKindShift) & 3;
                    if (t < 1 || kd != kGrammarStay) {
                        pn[M] = n; ps[2 * M] = t; ps[2 * M + 1] = vend; ++M;
                        if (t < 1 || kd == kGrammarLead) break;
                        n = min(c & kGrammarArcNode, N - 1);
                        kind = kd == kGrammarFromBlk ? 1 : 0;
                        vend = t;
                    }
                }
                --t;
            }
            kind = 2;
        }
#endif
        while (kind != 2) {
            const int f = t - tid;       // this lane's frame
            const int c = f >= 1 ? BP[(size_t)f * NS + n] : 0;
            int i = 0;                   // the path is at frame t - i
            bool jump = false;
            while (i < 64 && !jump) {
                const unsigned long long from = ~0ull << i;
                if (kind == 1) {         // blk(n): to the first frame that came from tok(n); the column stays
                    const unsigned long long m = __ballot(f < 1 || (c & kGrammarBlkFromTok)) & from;
                    if (!m) { i = 64; continue; }
                    const int k = __ffsll(m) - 1;
                    if (t - k < 1) { kind = 2; jump = true; continue; }      // (blk is -inf at frame 0: never on a path)
                    kind = 0; vend = t - k; i = k + 1;
                } else {                 // tok(n): to the first frame that did not stay, the visit's start
                    const unsigned long long m = __ballot(f < 1 || ((c >> kGrammarKindShift) & 3) != kGrammarStay) & from;
                    if (!m) { i = 64; continue; }
                    const int k = __ffsll(m) - 1, fs = t - k;
                    if (tid == 0) { pn[M] = n; ps[2 * M] = fs; ps[2 * M + 1] = vend; }
                    ++M;
                    const int cc = __shfl(c, k), kd = (cc >> kGrammarKindShift) & 3;
                    if (fs < 1 || kd == kGrammarLead) { kind = 2; jump = true; continue; }
                    n = min(cc & kGrammarArcNode, N - 1);
                    kind = kd == kGrammarFromBlk ? 1 : 0;
                    vend = fs;
                    t = fs - 1;
                    jump = true;
                }
            }
            if (!jump) t -= 64;
        }
        if (tid == 0) s_m = M;
    }
    __syncthreads();

    // ---- the visits in frame order, and per visit the mean of p(label) over its span (fp32, frames in order)
    const int M = s_m;
    for (int k = tid; k < M / 2; k += NT) {
        const int o = M - 1 - k;
        const int32_t n1 = pn[k], s1 = ps[2 * k], e1 = ps[2 * k + 1];
        pn[k] = pn[o]; ps[2 * k] = ps[2 * o]; ps[2 * k + 1] = ps[2 * o + 1];
        pn[o] = n1; ps[2 * o] = s1; ps[2 * o + 1] = e1;
    }
    __syncthreads();
    for (int k = tid; k < M; k += NT) {
        const int t0 = ps[2 * k], t1 = ps[2 * k + 1], lab = nodew[pn[k]] & 255;
        float sum = 0.f;
        for (int t = t0; t < t1; ++t) sum += P[(size_t)t * C + lab];
        a.token_probs[(size_t)b * a.T_out + k] = sum / (float)(t1 - t0);
    }
    if (tid == 0) { a.path_lens[b] = M; a.path_logp[b] = end_v; a.status[b] = 0; }
}

hipError_t launch_grammar(const GrammarArgs& a, int B, hipStream_t s) {
    const size_t lds = (size_t)grammar_carve_bytes(a.node_stride, a.arc_words);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(grammar_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grammar_kernel, dim3(B), dim3(kGrammarThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace dsmi
