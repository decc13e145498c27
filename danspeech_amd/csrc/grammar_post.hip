// CTC grammar posterior on the GPU (gfx950): grammar.hip's recurrence in the log-sum-exp semiring, float64 throughout, forward
// and backward over the same token graph -- the summed probability of every path the graph accepts (logp), the posterior that
// frame t carries label c given the grammar (occ) and each node's expected number of entries (visits).  The contract is in
// include/dsmi.h; tests/_grammar_post_ref.py states it in numpy.
//
// Node n carries tok(n) and blk(n), the blank behind it; `lead` is the blank before the first token.  Forward, per frame
//     ent(n)  = LSE{ lead [start]; per predecessor p in list order: blk(p), then tok(p) [label(p) != label(n)] }
//     tok'(n) = LSE(tok(n), ent(n) + w(n)) + lp(t, label(n));   blk'(n) = LSE(blk(n), tok(n)) + lp(t, blank);   lead' = lead + lp(t, blank)
// and backward its mirror image over the successor lists (the transposed arcs, built by the host), with b(x) = beta_{t+1}(x),
// frame t + 1's emission included, and bh = beta_t less frame t's emission, which is what is stored (as occ.hip does):
//     bh(tok n) = LSE{ b(tok n), b(blk n); per successor s with label(s) != label(n): w(s) + b(tok s) }
//     bh(blk n) = LSE{ b(blk n); per successor s: w(s) + b(tok s) }
//     bh(lead)  = LSE{ b(lead); per start node s: w(s) + b(tok s) }
// A log-sum-exp over a list is the greatest term first, then the sum of exp(term - greatest) in list order, then one log: its
// order is fixed by the graph alone.
//
// Three launches, each behind the one before on the stream; no workgroup waits for another.
// gp_trellis_kernel: two workgroups per clip as occ_trellis_kernel has them, the even one the forward pass (CtcFeeder), the odd
// one the backward pass from the last frame down (CtcFeederDown).  A workgroup keeps its graph in LDS as grammar_kernel does --
// node words, weights, 16-bit arc offsets and arcs, the backward pass the successors in the predecessors' place -- and two
// double-buffered rows of float64 (tok, blk) pairs; each thread owns the nodes tid, tid + 256, ...; one barrier per frame.  lead
// is a register of every thread going forward; going backward it needs the start nodes' sum, which wave 0 forms from the row of
// the frame before (a lane per start node of the list in LDS, the greatest by a butterfly, then the sum by a butterfly: a fixed
// tree).  A node with more than 24 arcs in the pass's lists is reduced by a wave in the same way, lane l summing the arcs l,
// l + 64, ... in order (a word loop's shared space node has every word's last letter before it).  A pass stores every (t, n)
// pair and lead and never loads (occ.hip has the measurement behind that).  The forward pass ends with logp, a block reduction
// in a fixed tree, and the status: -inf means unreachable and nothing else.
// gp_occ_kernel: one thread per element of occ over the caller's whole array, zeros included; a label's sum runs over the
// graph's nodes of that label in ascending order (the host's buckets), the blank's over lead and every blk.
// gp_visits_kernel: one thread per node, over the frames in order: the entries at t are gamma_t(tok n) less those that stayed,
// exp(alpha_{t-1}(tok n) + lp(t, label n) + bh_t(tok n) - logp); both terms are the node's own.
//
// Everything a clip's workgroups and output threads compute depends on its own graph and frames alone (the node stride places
// the rows and is no part of any sum), so its results are the same bits whatever else is in the launch.
#include "grammar_post.h"
#include "ctc_trellis.h"

namespace dsmi {

constexpr int kGpImage = kCtcChunk * kCtcMaxLabels;

__device__ __forceinline__ double gp_lse2(double a, double b) {
    const double m = fmax(a, b), u = fmin(a, b);
    const double r = m + log1p(exp(u - m));
    return m == -INFINITY ? m : r;       // (-inf - -inf is NaN: nothing of r is kept then)
}

__device__ __forceinline__ double gp_lse3(double a, double b, double c) {      // (occ.hip's)
    const double m = fmax(a, fmax(b, c));
    const double u = a == m ? b : a;
    const double v = a == m ? c : (b == m ? c : b);
    const double r = m + log1p(exp(u - m) + exp(v - m));
    return m == -INFINITY ? m : r;
}

__device__ __forceinline__ double gp_wave_max(double v) {
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) v = fmax(v, __shfl_xor(v, k));
    return v;
}
__device__ __forceinline__ double gp_wave_sum(double v) {      // a butterfly: every lane the same tree, x + y == y + x
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) v += __shfl_xor(v, k);
    return v;
}

// One pass of clip b over its frames.  The carve: pairs [2][NS], node words [NS], weights [NS], arc offsets [NS + 4], start nodes
// [NS], arcs [arc_words].
template <bool Back>
__device__ __forceinline__ void gp_pass(const GrammarPostArgs& a, int b, double (*lpc)[kGpImage], double* red, uint16_t* heavy, int* heavy_n,
                                        unsigned char* carve) {
    constexpr int NT = kGrammarPostThreads;
    const int tid = threadIdx.x;
    const int T = a.sizes[b], C = a.C, g = a.clip_graph[b], NS = a.node_stride;
    const int n0 = a.node_off[g], N = a.node_off[g + 1] - n0;
    const bool empty_ok = a.empty_ok[g] != 0;
    if (T == 0) {                        // without frames only the empty sentence
        if (!Back && tid == 0) {
            a.logp[b] = empty_ok ? 0.0 : -INFINITY;
            a.status[b] = empty_ok ? 0 : 1;
        }
        return;
    }
    double2* const row0 = reinterpret_cast<double2*>(carve);
    double2* const row1 = row0 + NS;
    int* const nodew = reinterpret_cast<int*>(row1 + NS);
    float* const wt = reinterpret_cast<float*>(nodew + NS);
    uint16_t* const aoff = reinterpret_cast<uint16_t*>(wt + NS);
    uint16_t* const starts = aoff + NS + 4;
    uint16_t* const arcs = starts + NS;
    const float* P = a.probs + (size_t)b * a.T_out * C;
    const size_t clip = (size_t)b * a.T_out;
    const int32_t* const off = Back ? a.succ_off : a.arc_off;
    const uint16_t* const lists = Back ? a.succ16 : a.arc16;
    const int arc0 = off[n0], NA = off[n0 + N] - arc0;
    const int st0 = a.start_off[g], NSt = a.start_off[g + 1] - st0;

    for (int n = tid; n < N; n += NT) { nodew[n] = a.words[n0 + n]; wt[n] = a.weights[n0 + n]; }
    for (int n = tid; n <= N; n += NT) aoff[n] = (uint16_t)(off[n0 + n] - arc0);
    for (int j = tid; j < NA; j += NT) arcs[j] = lists[arc0 + j];
    if (Back)
        for (int i = tid; i < NSt; i += NT) starts[i] = a.start16[st0 + i];
    // the nodes with more than kGrammarPostHeavy arcs in this pass's lists, each reduced by a wave: which wave takes which is
    // the order the threads arrive in, what a wave computes for a node is not (an integer counter in LDS, no sum goes through it)
    if (tid == 0) *heavy_n = 0;
    __syncthreads();
    for (int n = tid; n < N; n += NT)
        if (off[n0 + n + 1] - off[n0 + n] > kGrammarPostHeavy) heavy[atomicAdd(heavy_n, 1)] = (uint16_t)n;
    __syncthreads();
    const int n_heavy = *heavy_n, wave = tid >> 6, lane = tid & 63;

    if constexpr (!Back) {
        CtcFeeder<double, NT> feed(P, T, C, tid);
        feed.prologue(lpc);
        __syncthreads();
        double2* const FW = a.fwd + clip * NS;
        double* const LF = a.lead_fwd + clip;
        double lead = lpc[0][a.blank];
        for (int n = tid; n < N; n += NT) {
            const int q = nodew[n];
            const double2 v = make_double2((q & kGrammarStart) ? lpc[0][q & 255] + (double)wt[n] : -INFINITY, -INFINITY);
            row0[n] = v;
            FW[n] = v;
        }
        if (tid == 0) LF[0] = lead;
        __syncthreads();
        for (int t = 1; t < T; ++t) {
            const double2* prev = (t & 1) ? row0 : row1;
            double2* cur = (t & 1) ? row1 : row0;
            const double* lpt = feed.frame(lpc, t);
            const double lb = lpt[a.blank];
            double2* const frow = FW + (size_t)t * NS;
            for (int n = tid; n < N; n += NT) {
                const int q = nodew[n];
                const double2 me = prev[n];
                const int j0 = aoff[n], j1 = aoff[n + 1];
                if (j1 - j0 > kGrammarPostHeavy) continue;      // (a wave's, below)
                const bool st = (q & kGrammarStart) != 0;
                double m = st ? lead : -INFINITY;
                for (int j = j0; j < j1; ++j) {
                    const int aw = arcs[j];
                    const double2 pv = prev[aw & kGrammarArcNode];
                    m = fmax(m, pv.y);
                    if (aw & kGrammarArcTok) m = fmax(m, pv.x);
                }
                double ent = -INFINITY;
                if (m != -INFINITY) {
                    double s = st ? exp(lead - m) : 0.0;
                    for (int j = j0; j < j1; ++j) {
                        const int aw = arcs[j];
                        const double2 pv = prev[aw & kGrammarArcNode];
                        s += exp(pv.y - m);
                        if (aw & kGrammarArcTok) s += exp(pv.x - m);
                    }
                    ent = m + log(s);
                }
                const double2 v = make_double2(gp_lse2(me.x, ent + (double)wt[n]) + lpt[q & 255], gp_lse2(me.y, me.x) + lb);
                cur[n] = v;
                frow[n] = v;
            }
            for (int h = wave; h < n_heavy; h += NT / 64) {      // a node of many predecessors: lane l the arcs l, l + 64, ...
                const int n = heavy[h], q = nodew[n];
                const double2 me = prev[n];
                const int j0 = aoff[n], j1 = aoff[n + 1];
                const bool st = (q & kGrammarStart) != 0;
                double m = st ? lead : -INFINITY;
                for (int j = j0 + lane; j < j1; j += 64) {
                    const int aw = arcs[j];
                    const double2 pv = prev[aw & kGrammarArcNode];
                    m = fmax(m, pv.y);
                    if (aw & kGrammarArcTok) m = fmax(m, pv.x);
                }
                m = gp_wave_max(m);
                double ent = -INFINITY;
                if (m != -INFINITY) {
                    double s = st && lane == 0 ? exp(lead - m) : 0.0;
                    for (int j = j0 + lane; j < j1; j += 64) {
                        const int aw = arcs[j];
                        const double2 pv = prev[aw & kGrammarArcNode];
                        s += exp(pv.y - m);
                        if (aw & kGrammarArcTok) s += exp(pv.x - m);
                    }
                    ent = m + log(gp_wave_sum(s));
                }
                const double2 v = make_double2(gp_lse2(me.x, ent + (double)wt[n]) + lpt[q & 255], gp_lse2(me.y, me.x) + lb);
                if (lane == 0) { cur[n] = v; frow[n] = v; }
            }
            lead += lb;
            if (tid == 0) LF[t] = lead;
            feed.end_of_frame(lpc, t);
            __syncthreads();
        }
        // ---- the end: lead (when the empty sentence is accepted), then the final nodes ascending, blk before tok: the greatest in
        // a tree, then each thread's sum in that order, then the sums in the same tree
        const double2* fin = ((T - 1) & 1) ? row1 : row0;
        double m = tid == 0 && empty_ok ? lead : -INFINITY;
        for (int n = tid; n < N; n += NT)
            if (nodew[n] & kGrammarFinal) m = fmax(m, fmax(fin[n].x, fin[n].y));
        red[tid] = m;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
            __syncthreads();
        }
        const double M = red[0];
        __syncthreads();
        if (M == -INFINITY) {            // lp is finite, so -inf means that no accepted sentence fits the frames, and nothing else
            if (tid == 0) { a.logp[b] = -INFINITY; a.status[b] = 1; }
            return;
        }
        double sum = tid == 0 && empty_ok ? exp(lead - M) : 0.0;
        for (int n = tid; n < N; n += NT)
            if (nodew[n] & kGrammarFinal) { sum += exp(fin[n].y - M); sum += exp(fin[n].x - M); }
        red[tid] = sum;
        __syncthreads();
        for (int s = NT / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        if (tid == 0) { a.logp[b] = M + log(red[0]); a.status[b] = 0; }
    } else {
        CtcFeederDown<double, NT> feed(P, T, C, tid);
        feed.prologue(lpc);
        __syncthreads();
        double2* const BW = a.bwd + clip * NS;
        double* const LB = a.lead_bwd + clip;
        double leadh = empty_ok ? 0.0 : -INFINITY;       // bh(lead) of the frame above, and that frame's lp(blank): wave 0's
        double lb_up;
        {
            double2* top = ((T - 1) & 1) ? row1 : row0;
            const double* lpt = feed.frame(lpc, T - 1);
            lb_up = lpt[a.blank];
            for (int n = tid; n < N; n += NT) {
                const int q = nodew[n];
                const double z = (q & kGrammarFinal) ? 0.0 : -INFINITY;      // a path ends in a final node's tok or blk
                top[n] = make_double2(z + lpt[q & 255], z + lb_up);
                BW[(size_t)(T - 1) * NS + n] = make_double2(z, z);
            }
            if (tid == 0) LB[T - 1] = leadh;
            feed.end_of_frame(lpc, T - 1);
            __syncthreads();
        }
        for (int t = T - 2; t >= 0; --t) {
            const double2* prev = (t & 1) ? row0 : row1;        // frame t + 1's row, its emission included
            double2* cur = (t & 1) ? row1 : row0;
            const double* lpt = feed.frame(lpc, t);
            const double lb = lpt[a.blank];
            double2* const brow = BW + (size_t)t * NS;
            for (int n = tid; n < N; n += NT) {
                const int q = nodew[n];
                const double2 me = prev[n];
                const int j0 = aoff[n], j1 = aoff[n + 1];
                if (j1 - j0 > kGrammarPostHeavy) continue;      // (a wave's, below)
                double m_all = -INFINITY, m_dif = -INFINITY;     // over every successor, and over those of another label
                for (int j = j0; j < j1; ++j) {
                    const int aw = arcs[j], s = aw & kGrammarArcNode;
                    const double v = (double)wt[s] + prev[s].x;
                    m_all = fmax(m_all, v);
                    if (aw & kGrammarArcTok) m_dif = fmax(m_dif, v);
                }
                double e_all = -INFINITY, e_dif = -INFINITY;
                if (m_all != -INFINITY) {
                    double sa = 0.0, sd = 0.0;
                    for (int j = j0; j < j1; ++j) {
                        const int aw = arcs[j], s = aw & kGrammarArcNode;
                        const double e = exp((double)wt[s] + prev[s].x - m_all);
                        sa += e;
                        if (aw & kGrammarArcTok) sd += e;
                    }
                    e_all = m_all + log(sa);
                    if (m_dif == m_all) {
                        e_dif = sd == sa ? e_all : m_all + log(sd);
                    } else if (m_dif != -INFINITY) {             // (a successor of the node's own label is the greatest: the others again)
                        sd = 0.0;
                        for (int j = j0; j < j1; ++j) {
                            const int aw = arcs[j], s = aw & kGrammarArcNode;
                            if (aw & kGrammarArcTok) sd += exp((double)wt[s] + prev[s].x - m_dif);
                        }
                        e_dif = m_dif + log(sd);
                    }
                }
                const double bt = gp_lse3(me.x, me.y, e_dif), bb = gp_lse2(me.y, e_all);
                brow[n] = make_double2(bt, bb);
                cur[n] = make_double2(bt + lpt[q & 255], bb + lb);
            }
            for (int h = wave; h < n_heavy; h += NT / 64) {      // a node of many successors: lane l the arcs l, l + 64, ...
                const int n = heavy[h], q = nodew[n];
                const double2 me = prev[n];
                const int j0 = aoff[n], j1 = aoff[n + 1];
                double m_all = -INFINITY, m_dif = -INFINITY;
                for (int j = j0 + lane; j < j1; j += 64) {
                    const int aw = arcs[j], s = aw & kGrammarArcNode;
                    const double v = (double)wt[s] + prev[s].x;
                    m_all = fmax(m_all, v);
                    if (aw & kGrammarArcTok) m_dif = fmax(m_dif, v);
                }
                m_all = gp_wave_max(m_all);
                m_dif = gp_wave_max(m_dif);
                double e_all = -INFINITY, e_dif = -INFINITY;
                if (m_all != -INFINITY) {
                    double sa = 0.0, sd = 0.0;
                    for (int j = j0 + lane; j < j1; j += 64) {
                        const int aw = arcs[j], s = aw & kGrammarArcNode;
                        const double e = exp((double)wt[s] + prev[s].x - m_all);
                        sa += e;
                        if (aw & kGrammarArcTok) sd += e;
                    }
                    sa = gp_wave_sum(sa);
                    sd = gp_wave_sum(sd);
                    e_all = m_all + log(sa);
                    if (m_dif == m_all) {
                        e_dif = sd == sa ? e_all : m_all + log(sd);
                    } else if (m_dif != -INFINITY) {
                        sd = 0.0;
                        for (int j = j0 + lane; j < j1; j += 64) {
                            const int aw = arcs[j], s = aw & kGrammarArcNode;
                            if (aw & kGrammarArcTok) sd += exp((double)wt[s] + prev[s].x - m_dif);
                        }
                        e_dif = m_dif + log(gp_wave_sum(sd));
                    }
                }
                const double bt = gp_lse3(me.x, me.y, e_dif), bb = gp_lse2(me.y, e_all);
                if (lane == 0) {
                    brow[n] = make_double2(bt, bb);
                    cur[n] = make_double2(bt + lpt[q & 255], bb + lb);
                }
            }
            if (tid < 64) {              // lead: the start nodes' sum from frame t + 1's row
                double m = -INFINITY;
                for (int i = tid; i < NSt; i += 64) {
                    const int s = starts[i];
                    m = fmax(m, (double)wt[s] + prev[s].x);
                }
                m = gp_wave_max(m);
                double S = -INFINITY;
                if (m != -INFINITY) {
                    double sum = 0.0;
                    for (int i = tid; i < NSt; i += 64) {
                        const int s = starts[i];
                        sum += exp((double)wt[s] + prev[s].x - m);
                    }
                    S = m + log(gp_wave_sum(sum));
                }
                leadh = gp_lse2(leadh + lb_up, S);
                lb_up = lb;
                if (tid == 0) LB[t] = leadh;
            }
            feed.end_of_frame(lpc, t);
            __syncthreads();
        }
    }
}

// Workgroups 2i and 2i + 1: the forward and the backward pass of clip i; with no array asked for (a.both false) workgroup i is
// the forward pass of clip i, for logp alone.
__global__ void __launch_bounds__(kGrammarPostThreads) gp_trellis_kernel(GrammarPostArgs a) {
    extern __shared__ __align__(16) unsigned char gp_carve[];
    __shared__ double lpc[2][kGpImage];            // chunk j in lpc[j & 1] (counted from the last chunk in the backward pass), [frame][label]
    __shared__ double red[kGrammarPostThreads];
    __shared__ uint16_t heavy[kGrammarPostMaxHeavy];
    __shared__ int heavy_n;
    const int b = a.both ? blockIdx.x >> 1 : blockIdx.x;
    if (a.both && (blockIdx.x & 1)) gp_pass<true>(a, b, lpc, red, heavy, &heavy_n, gp_carve);
    else gp_pass<false>(a, b, lpc, red, heavy, &heavy_n, gp_carve);
}

// The caller's occ [B][T_out][C] in full.
__global__ void __launch_bounds__(kGrammarPostThreads) gp_occ_kernel(GrammarPostArgs a) {
    const size_t step = (size_t)gridDim.x * kGrammarPostThreads, first = (size_t)blockIdx.x * kGrammarPostThreads + threadIdx.x;
    const size_t C = (size_t)a.C, per = (size_t)a.T_out * C, total = (size_t)a.B * per;
    for (size_t i = first; i < total; i += step) {
        const int b = (int)(i / per), t = (int)(i % per / C), c = (int)(i % C);
        double v = 0.0;
        if (t < a.sizes[b] && a.status[b] == 0) {
            const int g = a.clip_graph[b], n0 = a.node_off[g], N = a.node_off[g + 1] - n0;
            const double logp = a.logp[b];
            const size_t lead = (size_t)b * a.T_out + t, base = lead * a.node_stride;
            if (c == a.blank) {
                v = exp(a.lead_fwd[lead] + a.lead_bwd[lead] - logp);      // (-inf where either is: exp gives 0; nothing here is +inf)
                for (int n = 0; n < N; ++n) v += exp(a.fwd[base + n].y + a.bwd[base + n].y - logp);
            } else {
                const int32_t* bo = a.bucket_off + (size_t)g * (C + 1);
                for (int k = bo[c]; k < bo[c + 1]; ++k) {
                    const int n = a.bucket_nodes[n0 + k];
                    v += exp(a.fwd[base + n].x + a.bwd[base + n].x - logp);
                }
            }
        }
        a.occ[i] = v;
    }
}

// visits [B][N_stride] in full: columns past the graph's nodes and infeasible clips are 0.
__global__ void __launch_bounds__(kGrammarPostThreads) gp_visits_kernel(GrammarPostArgs a) {
    const size_t i = (size_t)blockIdx.x * kGrammarPostThreads + threadIdx.x;
    if (i >= (size_t)a.B * a.N_stride) return;
    const int b = (int)(i / a.N_stride), n = (int)(i % a.N_stride);
    const int g = a.clip_graph[b], n0 = a.node_off[g], N = a.node_off[g + 1] - n0, T = a.sizes[b];
    double v = 0.0;
    if (n < N && T > 0 && a.status[b] == 0) {
        const int lab = a.words[n0 + n] & 255;
        const double logp = a.logp[b];
        const float* P = a.probs + (size_t)b * a.T_out * a.C + lab;
        const size_t base = (size_t)b * a.T_out * a.node_stride + n;
        double up = -INFINITY;           // alpha_{t-1}(tok n)
        for (int t = 0; t < T; ++t) {
            const double f = a.fwd[base + (size_t)t * a.node_stride].x, h = a.bwd[base + (size_t)t * a.node_stride].x;
            v += exp(f + h - logp);
            if (t > 0) v -= exp(up + log((double)fmaxf(P[(size_t)t * a.C], FLT_MIN)) + h - logp);
            up = f;
        }
    }
    a.visits[i] = v;
}

hipError_t launch_grammar_post(const GrammarPostArgs& a, hipStream_t s) {
    const size_t lds = (size_t)grammar_post_carve_bytes(a.node_stride, a.arc_words);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gp_trellis_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gp_trellis_kernel, dim3((a.both ? 2u : 1u) * (unsigned)a.B), dim3(kGrammarPostThreads), lds, s, a);
    e = hipGetLastError();
    if (e != hipSuccess || !a.both) return e;
    if (a.occ) {
        const size_t most = (size_t)a.B * a.T_out * a.C;
        const size_t blocks = std::min<size_t>((most + kGrammarPostThreads - 1) / kGrammarPostThreads, (size_t)1 << 20);
        hipLaunchKernelGGL(gp_occ_kernel, dim3((unsigned)blocks), dim3(kGrammarPostThreads), 0, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (a.visits && a.N_stride > 0) {
        const size_t blocks = ((size_t)a.B * a.N_stride + kGrammarPostThreads - 1) / kGrammarPostThreads;
        hipLaunchKernelGGL(gp_visits_kernel, dim3((unsigned)blocks), dim3(kGrammarPostThreads), 0, s, a);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace dsmi
