// Streaming grammar decoding on the GPU (gfx950): grammar_kernel's search (grammar.hip) carried from chunk to chunk of N live
// sessions in one launch.  The contract is equality with dsmi_grammar over the rows laid end to end (include/dsmi.h,
// dsmi_grammar_stream_advance_many): the recurrence, the candidates' order, the strictly-greater rule and every float32 addition
// are grammar_kernel's, restated here so that grammar.hip stays as it is.
//
// grammar_stream_kernel: one workgroup per stream.  The stream's graph goes into LDS as in grammar_kernel (the rows laid out with
// the net's widest stride, since one launch has one carve).  The pairs of utterance frame t live in row t & 1, so a call that
// begins at t0 > 0 restores the carried pairs into row (t0 - 1) & 1 and `lead` into its register; with t0 = 0 nothing of the block
// is read and the first frame initialises.  CtcFeeder runs over this call's rows; backpointer row t0 + f goes to the stream's own
// block, the rows themselves are copied into its history (the per-visit means need them), and at the exit the pairs, `lead` and the
// frame count go back.  With mode 1 or 2 the end rule, the wave backtrace from frame F - 1 and the means follow.  Backpointer rows
// at or past F, left over from an earlier utterance, are never read: the backtrace starts at F - 1 and only descends.
//
// Heavy nodes.  A node with more than kGrammarHeavyFan predecessors is not walked by its owner thread (grammar_kernel's 98 ns per
// arc and frame).  The host lists them; the four waves take the listed nodes in turn; the lanes stride the arc list, each keeping
// the first of the greatest of its own candidates (index = 2 x list position, + 1 for tok), and a butterfly takes the greater
// value and, among equal values, the lesser index.  "The first of the greatest in list order" is the lexicographic maximum of
// (value, -index) and a maximum rounds nothing, so ent and its backpointer are the sequential walk's bits.  The pass reads the
// previous row and writes only its own node of the current one: no barrier beyond the frame's.
// No communication between workgroups, no spinning, no atomics.
#include "grammar_stream.h"
#include "ctc_trellis.h"

#include <climits>

namespace dsmi {

__global__ void __launch_bounds__(kGrammarThreads) grammar_stream_kernel(GrammarStreamArgs a) {
    // tok / blk pairs [2][NS], node words [NS], weights [NS], arc offsets [NS + 4] and arcs [arc_words] of 16 bits
    extern __shared__ __align__(16) unsigned char carve[];
    using Feeder = CtcFeeder<float, kGrammarThreads>;
    __shared__ float lpc[2][Feeder::kImage];      // chunk j of this call in lpc[j & 1], [frame][label]
    __shared__ float red_v[kGrammarThreads];
    __shared__ int red_i[kGrammarThreads];
    __shared__ uint16_t heavy[256];
    __shared__ int s_m;
    constexpr int NT = kGrammarThreads;
    const int b = blockIdx.x, tid = threadIdx.x;
    const GrammarStreamDesc d = a.desc[b];
    const int T = d.T, t0 = d.t0, F = t0 + T, C = a.C, g = d.graph, NS = a.node_stride, BS = d.ns, mode = d.mode;
    if (T == 0 && mode == 0) return;     // (the same for the whole workgroup) nothing is due
    const bool empty_ok = a.empty_ok[g] != 0;
    if (F == 0) {                        // a result without frames: mode 2 is dsmi_grammar's zero-frame clip, mode 1 the empty path
        if (tid == 0) {
            const bool ok = mode == 1 || empty_ok;
            a.path_logp[b] = ok ? 0.f : -INFINITY;
            a.status[b] = ok ? 0 : 1;
            a.complete[b] = empty_ok ? 1 : 0;
        }
        return;
    }
    const int n0 = a.node_off[g], N = a.node_off[g + 1] - n0;
    const int arc0 = a.arc_off[n0], NA = a.arc_off[n0 + N] - arc0;
    const int h0 = a.heavy_off[g], NH = a.heavy_off[g + 1] - h0;
    float2* const row0 = reinterpret_cast<float2*>(carve);
    float2* const row1 = row0 + NS;
    int* const nodew = reinterpret_cast<int*>(row1 + NS);
    float* const wt = reinterpret_cast<float*>(nodew + NS);
    uint16_t* const aoff = reinterpret_cast<uint16_t*>(wt + NS);
    uint16_t* const arcs = aoff + NS + 4;
    const float* P = d.probs;
    uint16_t* const BP = d.bp;

    for (int n = tid; n < N; n += NT) { nodew[n] = a.words[n0 + n]; wt[n] = a.weights[n0 + n]; }
    for (int n = tid; n <= N; n += NT) aoff[n] = (uint16_t)(a.arc_off[n0 + n] - arc0);
    for (int j = tid; j < NA; j += NT) arcs[j] = a.arc_words16[arc0 + j];
    for (int h = tid; h < NH; h += NT) heavy[h] = a.heavy[h0 + h];
    float lead = 0.f;
    if (t0 > 0) {                        // the carried pairs: into the row that frame t0 reads
        float2* const prev = ((t0 - 1) & 1) ? row1 : row0;
        for (int n = tid; n < N; n += NT) prev[n] = d.pairs[n];
        lead = d.head->lead;
    }

    if (T > 0) {
        {                                // this call's rows into the history, behind the frames before
            float* const H = d.hist + (size_t)t0 * C;
            const size_t cells = (size_t)T * C;
            for (size_t i = tid; i < cells; i += NT) H[i] = P[i];
        }
        Feeder feed(P, T, C, tid);
        feed.prologue(lpc);
        __syncthreads();
        int f = 0;
        if (t0 == 0) {                   // the utterance's first frame
            lead = lpc[0][a.blank];
            for (int n = tid; n < N; n += NT) {
                const int q = nodew[n];
                row0[n] = make_float2((q & kGrammarStart) ? lpc[0][q & 255] + wt[n] : -INFINITY, -INFINITY);
            }
            __syncthreads();
            f = 1;
        }

        // ---- forward: call frame f = utterance frame t; the pairs of frame t in row[t & 1], lp in feed.frame(lpc, f)[label]
        for (; f < T; ++f) {
            const int t = t0 + f;
            const float2* prev = (t & 1) ? row0 : row1;
            float2* cur = (t & 1) ? row1 : row0;
            const float* lpt = feed.frame(lpc, f);
            const float lb = lpt[a.blank];
            uint16_t* brow = BP + (size_t)t * BS;
            // the rest of a node's frame once its best entry is known: grammar_kernel's, candidate for candidate
            auto finish = [&](int n, int q, float ent, int ecode) {
                const float2 me = prev[n];
                const float w = wt[n], l = lpt[q & 255];
                float best = me.x;
                int code = kGrammarStay << kGrammarKindShift;
                const float cand = ent + w;
                if (cand > best) { best = cand; code = ecode; }
                float bb = me.y;
                if (me.x > bb) { bb = me.x; code |= kGrammarBlkFromTok; }
                cur[n] = make_float2(best + l, bb + lb);
                brow[n] = (uint16_t)code;
            };
            for (int n = tid; n < N; n += NT) {
                const int q = nodew[n];
                if (q & kGrammarHeavy) continue;
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
                finish(n, q, ent, ecode);
            }
            for (int h = tid >> 6; h < NH; h += NT / 64) {      // (the same h for a whole wave)
                const int n = heavy[h], lane = tid & 63;
                const int j0 = aoff[n], j1 = aoff[n + 1];
                float bv = -INFINITY;
                int bi = INT_MAX;
                for (int j = j0 + lane; j < j1; j += 64) {
                    const int aw = arcs[j], idx = 2 * (j - j0);
                    const float2 pv = prev[aw & kGrammarArcNode];
                    if (pv.y > bv) { bv = pv.y; bi = idx; }
                    if ((aw & kGrammarArcTok) && pv.x > bv) { bv = pv.x; bi = idx + 1; }
                }
#pragma unroll
                for (int s = 32; s > 0; s >>= 1) {
                    const float v2 = __shfl_xor(bv, s);
                    const int i2 = __shfl_xor(bi, s);
                    if (v2 > bv || (v2 == bv && i2 < bi)) { bv = v2; bi = i2; }
                }
                if (lane == 0) {
                    const int q = nodew[n];
                    float ent = -INFINITY;
                    int ecode = 0;
                    if (q & kGrammarStart) { ent = lead; ecode = kGrammarLead << kGrammarKindShift; }
                    if (bv > ent) {      // (bv > -inf: bi is a candidate of the list)
                        ent = bv;
                        ecode = (((bi & 1) ? kGrammarFromTok : kGrammarFromBlk) << kGrammarKindShift) | (arcs[j0 + (bi >> 1)] & kGrammarArcNode);
                    }
                    finish(n, q, ent, ecode);
                }
            }
            lead += lb;
            feed.end_of_frame(lpc, f);
            __syncthreads();
        }

        // ---- the state goes back: the pairs of frame F - 1, lead, the frame count
        const float2* last = ((F - 1) & 1) ? row1 : row0;
        for (int n = tid; n < N; n += NT) d.pairs[n] = last[n];
        if (tid == 0) { d.head->lead = lead; d.head->frames = F; }
    }
    if (mode == 0) return;
    __syncthreads();                     // (T = 0: the restored row)

    // ---- the end: lead (when the empty sentence is accepted), then the final nodes ascending, blk before tok; the first of the
    // greatest wins.  Candidate index: 0 lead, 1 + 2n blk(n), 2 + 2n tok(n).  A partial result (mode 1) takes every state.
    const bool any_state = mode == 1;
    {
        const float2* fin = ((F - 1) & 1) ? row1 : row0;
        float bv = -INFINITY;
        int bi = INT_MAX;
        if (tid == 0 && (empty_ok || any_state)) { bv = lead; bi = 0; }
        for (int n = tid; n < N; n += NT) {
            if (!any_state && !(nodew[n] & kGrammarFinal)) continue;
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
    if (end_v == -INFINITY) {            // no accepted sentence fits the frames (mode 2 only: a partial always has lead)
        if (tid == 0) { a.path_logp[b] = -INFINITY; a.status[b] = 1; a.complete[b] = 0; }
        return;
    }

    // ---- backtrace, wave 0, as grammar_kernel's: kind 0 = in tok(n) at frame t, 1 = in blk(n), 2 = in lead (over).  Every round
    // either ends or lowers t, whatever the codes hold; a node id is clamped into the graph.
    int32_t* const pn = a.path_nodes + (size_t)b * a.P_stride;
    int32_t* const ps = a.path_spans + 2 * (size_t)b * a.P_stride;
    if (tid < 64) {
        int kind = 2, n = 0, t = F - 1, vend = F, M = 0;
        if (end_i > 0) { n = (end_i - 1) >> 1; kind = (end_i & 1) ? 1 : 0; }
        while (kind != 2) {
            const int fr = t - tid;      // this lane's frame
            const int c = fr >= 1 ? BP[(size_t)fr * BS + n] : 0;
            int i = 0;                   // the path is at frame t - i
            bool jump = false;
            while (i < 64 && !jump) {
                const unsigned long long from = ~0ull << i;
                if (kind == 1) {         // blk(n): to the first frame that came from tok(n); the column stays
                    const unsigned long long m = __ballot(fr < 1 || (c & kGrammarBlkFromTok)) & from;
                    if (!m) { i = 64; continue; }
                    const int k = __ffsll(m) - 1;
                    if (t - k < 1) { kind = 2; jump = true; continue; }      // (blk is -inf at frame 0: never on a path)
                    kind = 0; vend = t - k; i = k + 1;
                } else {                 // tok(n): to the first frame that did not stay, the visit's start
                    const unsigned long long m = __ballot(fr < 1 || ((c >> kGrammarKindShift) & 3) != kGrammarStay) & from;
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

    // ---- the visits in frame order, and per visit the mean of p(label) over its span (fp32, frames in order), from the history
    const int M = s_m;
    for (int k = tid; k < M / 2; k += NT) {
        const int o = M - 1 - k;
        const int32_t n1 = pn[k], s1 = ps[2 * k], e1 = ps[2 * k + 1];
        pn[k] = pn[o]; ps[2 * k] = ps[2 * o]; ps[2 * k + 1] = ps[2 * o + 1];
        pn[o] = n1; ps[2 * o] = s1; ps[2 * o + 1] = e1;
    }
    __syncthreads();
    for (int k = tid; k < M; k += NT) {
        const int v0 = ps[2 * k], v1 = ps[2 * k + 1], lab = nodew[pn[k]] & 255;
        float sum = 0.f;
        for (int t = v0; t < v1; ++t) sum += d.hist[(size_t)t * C + lab];
        a.token_probs[(size_t)b * a.P_stride + k] = sum / (float)(v1 - v0);
    }
    if (tid == 0) {
        a.path_lens[b] = M; a.path_logp[b] = end_v; a.status[b] = 0;
        a.complete[b] = end_i == 0 ? (empty_ok ? 1 : 0) : ((nodew[(end_i - 1) >> 1] & kGrammarFinal) ? 1 : 0);
    }
}

hipError_t launch_grammar_stream(const GrammarStreamArgs& a, int n, hipStream_t s) {
    const size_t lds = (size_t)grammar_carve_bytes(a.node_stride, a.arc_words);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(grammar_stream_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(grammar_stream_kernel, dim3(n), dim3(kGrammarThreads), lds, s, a);
    return hipGetLastError();
}

}  // namespace dsmi
