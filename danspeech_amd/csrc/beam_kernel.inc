// CTC prefix beam search kernel (gfx950) and its on-chip layout: the device half of decoder.hip, kept in a file of its own
// so that tools/exp/beam_emu.cpp can compile the SAME source for the CPU (a small SIMT emulation: one host thread per
// GPU thread, real barriers) -- the frame loop's phase structure can then be debugged without a GPU.
// Needs: lm.h (LmView, lm_cond_log10), <cmath>, and DSMI_WAIT_STORES() = "every vector-memory store of this wave has landed".
namespace {

constexpr double BIN_SPAN = 64.0; // the selection histogram has one bin per thread, over the 64 nats below the frame's score bound
constexpr int LISTCAP = 256;      // members of the threshold bin that are ranked from a list (more: ranked against all keys)
constexpr int MAXCTX = kMaxOrder - 1;
constexpr int MAXC = 128;
constexpr int MEMO_UNSET = 0x7fc00001;   // a NaN pattern no float computation produces

// One record of the node pool (HBM).  Written at creation, tstep / lpc updated in place by get_path_trie's "better emission
// frame" rule; read only when a dormant prefix re-enters the beam (the walk in resolve()) and by the final path output.
struct __attribute__((aligned(32))) NodeRec { int parent, ch, tstep, depth; double lpc; double pad; };
static_assert(sizeof(NodeRec) == 32, "NodeRec is two 16-byte stores");

struct BeamArgs {
    const float* probs; const int32_t* sizes; int T, C, blank, space, beam, cutoff_top_n; float cutoff_prob;
    int has_lm, order; double alpha, beta;
    LmView lm; const int32_t* trie_next; const int32_t* trie_word; int unk, bos;
    int ncap;                    // per-utterance node pool capacity
    NodeRec* nodes;
    int32_t* dbg;                // optional [B][4]: dormant prefixes revived, walk hops, list rankings, full rankings
    unsigned long long* stamps;  // optional [64 frames][8]: 100 MHz timestamps of utterance 0's phase boundaries, from the middle of the clip
    // outputs
    int32_t *out_tok, *out_step, *out_len, *out_n; double* out_score;
    const struct BeamStreamDesc* desc;   // RESUME: [gridDim.x] one session each (the batch fields above are unused)
};

// One session of a resumable launch (beam_kernel<..., RESUME = true>): this chunk's rows, the search carried from the frames
// before it, the session's node pool, and where its best hypotheses go.
struct BeamStreamDesc {
    const float* probs;          // [T][C] this chunk's probabilities (T = 0 allowed)
    unsigned char* state;        // the carried search, laid out by stream_state()
    NodeRec* nodes;              // the session's node pool (capacity >= 2 + (t0 + T) * beam, kept by the host)
    int32_t *out_tok, *out_step; // [n_best][out_T] hypotheses over frames 0 .. t0 + T, best first
    int32_t *out_len, *out_n;    // [n_best], [1]: beams written (min(beams in the search, n_best))
    double* out_score;           // [n_best] totals with the trailing-word term, as the offline search reports them
    int T, t0, n_best, out_T;    // n_best = 0: advance only
};

// The carried search of one session in HBM: every value a frame reads that an earlier frame wrote.  That is the current buffer's
// entry arrays and child table, the beam size, the scorer's min_cutoff key, the score bound and the node count; everything else
// in the carve is written in the frame that reads it (the hist bins are cleared as they are read, the other buffer's child table
// in F2, the probability row one frame ahead -- the entry makes the chunk's first).
struct StreamHdr { int nb, nn; uint64_t kmin; double bound; double pad; };
struct StreamState { size_t hdr, bprev, nbprev, score, uplpc, ownlpc, node, ch, ds, depth, up, upch, upnode, memo, ctx, cell, bytes; };
__host__ __device__ inline StreamState stream_state(int BW, int C) {
    StreamState k; size_t o = 0;
    auto take = [&](size_t n, size_t sz) { const size_t at = o; o += ((n * sz + 15) & ~(size_t)15); return at; };
    k.hdr = take(1, sizeof(StreamHdr));
    k.bprev = take(BW, 8); k.nbprev = take(BW, 8); k.score = take(BW, 8); k.uplpc = take(BW, 8); k.ownlpc = take(BW, 8);
    k.node = take(BW, 4); k.ch = take(BW, 4); k.ds = take(BW, 4); k.depth = take(BW, 4); k.up = take(BW, 4);
    k.upch = take(BW, 4); k.upnode = take(BW, 4); k.memo = take(BW, 4); k.ctx = take((size_t)BW * MAXCTX, 4);
    k.cell = take(((size_t)BW * C + 1) & ~(size_t)1, 2);
    k.bytes = o;
    return k;
}

// On-chip layout of one utterance's search, shared by the kernel and the launcher's size check.
struct Carve {
    size_t lp, sd, bprev, nbprev, score, uplpc, ownlpc, bcur, nbcur, ckey, lkey, su, wkmin, fkey;   // 8-byte items
    size_t node, ch, ds, depth, up, upch, upnode, memo, ctx, newslot, use, lidx, hist, wtot, wsurv, wfresh, si, pfp, fidx, fmark, farc, ffr;   // 4-byte
    size_t cell;                                                                                // 2-byte
    size_t lmv;
    size_t bytes;
};
__host__ __device__ inline Carve carve(int BW, int C, int BT) {
    const int NBINS = BT, NWAVE = BT / 64;
    Carve k; size_t o = 0;
    const size_t NMAX = (size_t)BW * (C + 1);
    auto take = [&](size_t n, size_t sz) { const size_t at = o; o += ((n * sz + 15) & ~(size_t)15); return at; };
    k.lp = take(2 * MAXC, 8); k.sd = take(8, 8);
    k.bprev = take(2 * BW, 8); k.nbprev = take(2 * BW, 8); k.score = take(2 * BW, 8); k.uplpc = take(2 * BW, 8); k.ownlpc = take(2 * BW, 8);
    k.bcur = take(BW, 8); k.nbcur = take(BW, 8); k.ckey = take(NMAX, 8); k.lkey = take(LISTCAP, 8); k.su = take(4, 8); k.wkmin = take(NWAVE, 8); k.fkey = take(BW, 8);
    k.node = take(2 * BW, 4); k.ch = take(2 * BW, 4); k.ds = take(2 * BW, 4); k.depth = take(2 * BW, 4); k.up = take(2 * BW, 4);
    k.upch = take(2 * BW, 4); k.upnode = take(2 * BW, 4); k.memo = take(2 * BW, 4); k.ctx = take((size_t)2 * BW * MAXCTX, 4);
    k.newslot = take(BW, 4); k.use = take(2 * MAXC, 4); k.lidx = take(LISTCAP, 4); k.hist = take(NBINS, 4);
    k.wtot = take(NWAVE, 4); k.wsurv = take(NWAVE, 4); k.wfresh = take(NWAVE, 4); k.si = take(16, 4); k.pfp = take(2 * MAXC, 4);
    k.fidx = take(BW, 4); k.fmark = take(BW, 4); k.farc = take(BW, 4); k.ffr = take(BW, 4);
    k.cell = take((size_t)2 * (((size_t)BW * C + 1) & ~(size_t)1), 2);
    k.lmv = take(1, sizeof(LmView));
    k.bytes = o;
    return k;
}

__device__ __forceinline__ double lse2(double x, double y) {
    // log(exp(x - m) + exp(y - m)) + m with m = max: the larger term's exp is exactly 1
    if (x == -INFINITY) return y;
    if (y == -INFINITY) return x;
    const double m = fmax(x, y), d = fmin(x, y) - m;
    return log(1.0 + exp(d)) + m;
}

__device__ __forceinline__ uint64_t okey(double v) {   // order-preserving bits, > 0 for every double
    uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double unokey(uint64_t k) {
    const uint64_t u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}
template <int NBINS>
__device__ __forceinline__ int score_bin(double U, double s) {     // monotone: a better score never lands in a later bin
    const double q = (U - s) * (NBINS / BIN_SPAN);
    if (!(q < (double)(NBINS - 1))) return NBINS - 1;              // also NaN (U - s with both infinite)
    return q > 0.0 ? (int)q : 0;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// inclusive prefix sum over the 64 lanes of a wave: four shifts inside each row of 16 lanes, then the two row broadcasts
__device__ __forceinline__ unsigned wave_incl_scan(unsigned v) {
#ifdef SIMT_EMU
    for (int o = 1; o < 64; o <<= 1) { const unsigned u = __shfl_up(v, o, 64); if ((int)(threadIdx.x & 63) >= o) v += u; }
    return v;
#else
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);     // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);     // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);     // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);     // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);     // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);     // row_bcast:31 into rows 2 and 3
    return (unsigned)x;
#endif
}

struct Tup { int up, upch, upnode; double uplpc; };

// The scorer's n-gram look-ups stay out of line: three call sites, rarely taken, a long chain of dependent loads each.
__device__ __noinline__ float lm_word_log10(const LmView* v, const int32_t* ctx, int n, int32_t w, int32_t unk) {
    return lm_cond_log10(*v, ctx, n, w, unk);
}

// CTC prefix beam search of one utterance by one workgroup; the algorithm, array for array, is oracle/beam_flat.py
// (tests/test_oracle_beam_flat.py holds that formulation to ctcdecode's pointer trie as restated in oracle/beam.py).
// A frame is six barrier-separated phases, all on LDS; HBM sees fire-and-forget stores (new node records, timestep updates)
// and, one frame ahead, the load of the next probability row:
//   F1  every candidate in registers: thread idx < nb = beam entry idx (its blank / repeat terms, and -- pull form -- the
//       extension it receives from its parent when that is a beam entry), the others = (entry, character) pairs; keys go
//       into a 1024-bin histogram of (bound - score) at 1/16 nat;
//   F2  prefix sums of the histogram, wave level; the last wave turns the prefetched row into log-probabilities;
//   F3  the bin in which the beam_width-th best score lies, and how many of its members survive;
//   F4  members of that bin ranked exactly (score desc, character asc, index asc) when not all of them survive; survivors
//       numbered inside each wave;
//   F5  new slot numbers; what left the beam, which dormant prefixes came back;
//   F6  commit: the new beam entry by entry into the other buffer (edge tuples resolved through whatever left), node
//       records to HBM, the child table of the new beam.
// CBW / CC: beam width and label count as compile-time constants (0: read from the arguments).  With them every LDS array's
// offset is an immediate of its instruction instead of a register the frame loop keeps live: the generic build holds ~30 such
// bases and spills 60 dwords per lane at 1024 threads.
// RESUME: one workgroup per session of a.desc, resuming that session's carried search at frame t0 for its chunk's T frames,
// saving the search back, and -- n_best > 0 -- writing the best n_best hypotheses over all t0 + T frames (the final section on
// the saved copy: the carried scores never receive the trailing-word term).  Node timesteps are absolute (t0 + t).
template <int BT, int KMAX, int CBW = 0, int CC = 0, bool RESUME = false>
__global__ __launch_bounds__(BT) void beam_kernel(BeamArgs a) {
    constexpr int NWAVE = BT / 64, NBINS = BT, BPL = NBINS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int C = CC ? CC : a.C, BW = CBW ? CBW : a.beam;
    // thread roles: EW waves carry the beam entries; with a scorer the next SW waves carry the (entry, space) pairs -- the ones
    // that may have to look an n-gram up, a chain of dependent loads that then runs beside the entries' chain instead of inside
    // the other pairs' loop; the remaining PT threads carry all other pairs
    const int EW = (BW + 63) / 64, SW = a.has_lm ? EW : 0, PT = BT - 64 * (EW + SW);
    const Carve kv = carve(BW, C, BT);
    LmView* s_lm = reinterpret_cast<LmView*>(smem_raw + kv.lmv);
    double* lp = reinterpret_cast<double*>(smem_raw + kv.lp);            // [2][MAXC] by frame parity
    double* sd = reinterpret_cast<double*>(smem_raw + kv.sd);            // [0..1] ln p(blank), [2..3] max_c lp, [4] bound on the beam's scores
    double* e_bprev = reinterpret_cast<double*>(smem_raw + kv.bprev);    // entry arrays [2][BW]
    double* e_nbprev = reinterpret_cast<double*>(smem_raw + kv.nbprev);
    double* e_score = reinterpret_cast<double*>(smem_raw + kv.score);
    double* e_uplpc = reinterpret_cast<double*>(smem_raw + kv.uplpc);
    double* e_ownlpc = reinterpret_cast<double*>(smem_raw + kv.ownlpc);
    double* e_bcur = reinterpret_cast<double*>(smem_raw + kv.bcur);      // [BW]
    double* e_nbcur = reinterpret_cast<double*>(smem_raw + kv.nbcur);
    uint64_t* c_key = reinterpret_cast<uint64_t*>(smem_raw + kv.ckey);   // [NMAX] 0 = no candidate, else okey(score)
    uint64_t* l_key = reinterpret_cast<uint64_t*>(smem_raw + kv.lkey);   // [LISTCAP]
    uint64_t* su = reinterpret_cast<uint64_t*>(smem_raw + kv.su);        // [0] smallest key of the beam
    uint64_t* wkmin = reinterpret_cast<uint64_t*>(smem_raw + kv.wkmin);  // [NWAVE]
    int* e_node = reinterpret_cast<int*>(smem_raw + kv.node);
    int* e_ch = reinterpret_cast<int*>(smem_raw + kv.ch);
    int* e_ds = reinterpret_cast<int*>(smem_raw + kv.ds);
    int* e_depth = reinterpret_cast<int*>(smem_raw + kv.depth);
    int* e_up = reinterpret_cast<int*>(smem_raw + kv.up);
    int* e_upch = reinterpret_cast<int*>(smem_raw + kv.upch);
    int* e_upnode = reinterpret_cast<int*>(smem_raw + kv.upnode);
    int* e_memo = reinterpret_cast<int*>(smem_raw + kv.memo);
    int* e_ctx = reinterpret_cast<int*>(smem_raw + kv.ctx);              // [2][BW][MAXCTX]
    int* newslot = reinterpret_cast<int*>(smem_raw + kv.newslot);
    int* usev = reinterpret_cast<int*>(smem_raw + kv.use);               // [2][MAXC]
    int* l_idx = reinterpret_cast<int*>(smem_raw + kv.lidx);
    unsigned* hist = reinterpret_cast<unsigned*>(smem_raw + kv.hist);
    int* wsurv = reinterpret_cast<int*>(smem_raw + kv.wsurv);
    int* wfresh = reinterpret_cast<int*>(smem_raw + kv.wfresh);
    int* si = reinterpret_cast<int*>(smem_raw + kv.si);
    uint64_t* f_key = reinterpret_cast<uint64_t*>(smem_raw + kv.fkey);   // the next beam's candidates by slot: key, candidate index,
    int* f_idx = reinterpret_cast<int*>(smem_raw + kv.fidx);             // kind, dictionary arc, rank among the new nodes
    int* f_mark = reinterpret_cast<int*>(smem_raw + kv.fmark);
    int* f_arc = reinterpret_cast<int*>(smem_raw + kv.farc);
    int* f_fr = reinterpret_cast<int*>(smem_raw + kv.ffr);
    float* pfp = reinterpret_cast<float*>(smem_raw + kv.pfp);            // [MAXC] row being pruned, [MAXC] the same sorted
    short* cell = reinterpret_cast<short*>(smem_raw + kv.cell);          // [2][CELLS]: (entry, label) -> an entry of that edge
    const int CELLS = (BW * C + 1) & ~1;
#define s_nb si[0]
#define s_bstar si[1]
#define s_r si[2]
#define s_mb si[3]
#define s_nlist si[4]
#define s_nrev si[5]
#define s_kmin su[0]

    const BeamStreamDesc* sdsc = RESUME ? a.desc + b : nullptr;
    NodeRec* nodes = RESUME ? sdsc->nodes : a.nodes + (size_t)b * a.ncap;
    const int T = RESUME ? sdsc->T : a.sizes ? min(a.sizes[b], a.T) : a.T;
    const float* pb = RESUME ? sdsc->probs : a.probs + (size_t)b * a.T * C;
    const int t0 = RESUME ? sdsc->t0 : 0;
    const bool fresh = !RESUME || t0 == 0;
    const int NCTX = a.order - 1;
    const double betap = fmax(0.0, a.beta);
    const bool prune = a.cutoff_prob < 1.0f || a.cutoff_top_n < C;
    const unsigned long long lt_mask = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    int dbg_rev = 0, dbg_hops = 0, dbg_list = 0, dbg_full = 0;

    // The last wave turns row tt of the probabilities (held in p0, p1: labels lane and lane + 64; pbl = p(blank)) into the
    // log-probabilities, the vocabulary mask and the two scalars of frame tt (decoder_utils get_pruned_log_probs).
    auto make_row = [&](int tt, float p0, float p1, float pbl) {
        const int par = tt & 1;
        // ln p(blank) (no FLT_MIN, for the scorer's min_cutoff) rides in a lane the labels leave free
        double x0 = lane < C ? (double)p0 + 1.17549435e-38 : 1.0, x1 = lane + 64 < C ? (double)p1 + 1.17549435e-38 : 1.0;
        if (C < 64) { if (lane == 63) x0 = (double)pbl; }
        else if (C < 128) { if (lane == 63) x1 = (double)pbl; }
        const double l0 = log(x0);
        if (lane < C) { lp[par * MAXC + lane] = l0; usev[par * MAXC + lane] = 1; }
        if (C < 64) { if (lane == 63) sd[par] = l0; }
        else {
            const double l1 = log(x1);
            if (lane + 64 < C) { lp[par * MAXC + lane + 64] = l1; usev[par * MAXC + lane + 64] = 1; }
            if (C < 128) { if (lane == 63) sd[par] = l1; }
            else if (lane == 0) sd[par] = log((double)pbl);
        }
        if (prune) {
            // rank of every label by (probability desc, index asc); the cumulative sum runs in that order, in double, like the
            // reference's loop, so that `cum >= cutoff_prob` falls on the same label
            if (lane < C) pfp[lane] = p0;
            if (lane + 64 < C) pfp[lane + 64] = p1;
            __builtin_amdgcn_wave_barrier();
            int rk[2] = {0, 0};
            for (int h = 0; h < 2; ++h) {
                const int c = lane + 64 * h;
                if (c >= C) continue;
                const float pc = pfp[c];
                int r = 0;
                for (int o = 0; o < C; ++o) { const float po = pfp[o]; r += (po > pc) || (po == pc && o < c); }
                rk[h] = r;
                pfp[MAXC + r] = pc;
            }
            __builtin_amdgcn_wave_barrier();
            int len = C;
            if (a.cutoff_prob < 1.0f) {
                int mine = C;
                for (int h = 0; h < 2; ++h) {
                    const int c = lane + 64 * h;
                    if (c >= C) continue;
                    double cum = 0.0;
                    for (int k = 0; k <= rk[h]; ++k) cum += (double)pfp[MAXC + k];
                    if (cum >= (double)a.cutoff_prob || rk[h] + 1 >= a.cutoff_top_n) mine = min(mine, rk[h] + 1);
                }
                for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o, 64));
                len = mine;
            } else len = a.cutoff_top_n;
            for (int h = 0; h < 2; ++h) { const int c = lane + 64 * h; if (c < C) usev[par * MAXC + c] = rk[h] < len; }
        }
    };

    // ---- start: the root is the whole beam
    int nn0 = 1;
    for (int q = tid; q < NBINS; q += BT) hist[q] = 0;
    if (fresh) {
    for (int q = tid; q < CELLS; q += BT) reinterpret_cast<int*>(cell)[q] = -1;       // both buffers (2 * CELLS shorts)
    if (tid == 0) {
        NodeRec r; r.parent = -1; r.ch = -1; r.tstep = 0; r.depth = 0; r.lpc = -INFINITY; r.pad = 0.0;
        nodes[0] = r;
        e_node[0] = 0; e_ch[0] = -1; e_ds[0] = 0; e_depth[0] = 0; e_up[0] = -1; e_upch[0] = -1; e_upnode[0] = -1; e_memo[0] = MEMO_UNSET;
        e_bprev[0] = 0.0; e_nbprev[0] = -INFINITY; e_score[0] = 0.0; e_uplpc[0] = -INFINITY; e_ownlpc[0] = -INFINITY;
        for (int k = 0; k < MAXCTX; ++k) e_ctx[k] = a.bos;
        s_nb = 1; s_kmin = okey(0.0); sd[4] = 0.0; s_nlist = 0; s_nrev = 0;
        *s_lm = a.lm;
    }
    } else if constexpr (RESUME) {
        // ---- resume: the carried search into buffer 0 (buffer 1's child table is cleared in F2 before anything uses it)
        const StreamState ks = stream_state(BW, C);
        const unsigned char* st = sdsc->state;
        const StreamHdr h = *reinterpret_cast<const StreamHdr*>(st + ks.hdr);
        nn0 = h.nn;
        for (int j = tid; j < h.nb; j += BT) {
            e_bprev[j] = reinterpret_cast<const double*>(st + ks.bprev)[j]; e_nbprev[j] = reinterpret_cast<const double*>(st + ks.nbprev)[j];
            e_score[j] = reinterpret_cast<const double*>(st + ks.score)[j]; e_uplpc[j] = reinterpret_cast<const double*>(st + ks.uplpc)[j];
            e_ownlpc[j] = reinterpret_cast<const double*>(st + ks.ownlpc)[j];
            e_node[j] = reinterpret_cast<const int*>(st + ks.node)[j]; e_ch[j] = reinterpret_cast<const int*>(st + ks.ch)[j];
            e_ds[j] = reinterpret_cast<const int*>(st + ks.ds)[j]; e_depth[j] = reinterpret_cast<const int*>(st + ks.depth)[j];
            e_up[j] = reinterpret_cast<const int*>(st + ks.up)[j]; e_upch[j] = reinterpret_cast<const int*>(st + ks.upch)[j];
            e_upnode[j] = reinterpret_cast<const int*>(st + ks.upnode)[j]; e_memo[j] = reinterpret_cast<const int*>(st + ks.memo)[j];
            for (int k = 0; k < MAXCTX; ++k) e_ctx[(size_t)j * MAXCTX + k] = reinterpret_cast<const int*>(st + ks.ctx)[(size_t)j * MAXCTX + k];
        }
        for (int q = tid; q < CELLS / 2; q += BT) reinterpret_cast<int*>(cell)[q] = reinterpret_cast<const int*>(st + ks.cell)[q];
        if (tid == 0) { s_nb = h.nb; s_kmin = h.kmin; sd[4] = h.bound; s_nlist = 0; s_nrev = 0; *s_lm = a.lm; }
    }
    if (wid == NWAVE - 1 && T > 0)
        make_row(0, lane < C ? pb[lane] : 0.f, lane + 64 < C ? pb[lane + 64] : 0.f, pb[a.blank]);
    __syncthreads();
    int cur = 0, nn = nn0;
    const int stamp_t0 = T / 2;
    auto stamp = [&](int t, int phase) {
        if (a.stamps && b == 0 && tid == 0 && t >= stamp_t0 && t < stamp_t0 + 64) a.stamps[(t - stamp_t0) * 8 + phase] = wall_clock64();
    };

    for (int t = 0; t < T; ++t) {
        const int nxt = cur ^ 1, par = t & 1;
        stamp(t, 0);
        const int nb = s_nb;
        const double* lpv = lp + par * MAXC; const int* use = usev + par * MAXC;
        const double* bprev = e_bprev + cur * BW; const double* nbprev = e_nbprev + cur * BW; const double* score = e_score + cur * BW;
        double* uplpc = e_uplpc + cur * BW; const double* ownlpc = e_ownlpc + cur * BW;
        const int* node = e_node + cur * BW; const int* ech = e_ch + cur * BW; const int* eds = e_ds + cur * BW;
        const int* depth = e_depth + cur * BW; const int* up = e_up + cur * BW; const int* upch = e_upch + cur * BW;
        const int* upnode = e_upnode + cur * BW; int* memo = e_memo + cur * BW; const int* ctx = e_ctx + (size_t)cur * BW * MAXCTX;
        short* cellc = cell + (size_t)cur * CELLS; short* celln = cell + (size_t)nxt * CELLS;
        // next frame's row, on its way while this frame runs
        float pn0 = 0.f, pn1 = 0.f, pnb = 0.f;
        if (wid == NWAVE - 1 && t + 1 < T) {
            const float* pr = pb + (size_t)(t + 1) * C;
            if (lane < C) pn0 = pr[lane];
            if (lane + 64 < C) pn1 = pr[lane + 64];
            pnb = pr[a.blank];
        }
        const bool full = a.has_lm && nb == BW;
        const double mincut = a.has_lm ? unokey(s_kmin) + sd[par] - betap : -INFINITY;
        const double U = sd[4] + betap + 1.2;      // no score of this frame exceeds it (alpha >= 0; ln p <= 0; a log-sum of three)
        const int NP = nb * C, N = nb + NP;
        const float invC = 1.0f / (float)C;

        // the extension of prefix P by character c (not a repeat of its blank-terminated self): ctc_beam_search_decoder.cpp's
        // log_p, with the scorer's word score on the space character
        auto pair_logp = [&](int P, int c, int arcw) -> double {
            const double l = lpv[c];
            double logp = -INFINITY;
            if (c == ech[P]) { if (bprev[P] > -INFINITY) logp = l + bprev[P]; }
            else logp = l + score[P];
            if (a.has_lm && c == a.space) {
                double lm = kOovScore;
                if (arcw >= 0) {
                    float l10;
                    const int mm = memo[P];
                    if (mm != MEMO_UNSET) l10 = __int_as_float(mm);
                    else {
                        l10 = lm_word_log10(s_lm, ctx + (size_t)P * MAXCTX, NCTX, arcw, a.unk);
                        memo[P] = __float_as_int(l10);
                    }
                    lm = (double)l10 / (double)kLog10E;
                }
                logp += lm * a.alpha;
                logp += a.beta;
            }
            return logp;
        };

        // ---- F1: candidates.  The first EW waves carry the beam entries (one each: the long dependent chain of the frame, two
        // log-sum-exps in double), every other wave KMAX (entry, character) pairs per thread.
        uint64_t key[KMAX]; int mark[KMAX], arcv[KMAX], binv[KMAX], cidx[KMAX];   // mark: -1 none, 0 entry, 1 fresh child, 2 + rep: dormant top
#pragma unroll
        for (int k = 0; k < KMAX; ++k) { key[k] = 0; mark[k] = -1; arcv[k] = -1; binv[k] = NBINS; cidx[k] = -1; }
        if (wid < EW) {
            __builtin_amdgcn_s_setprio(3);              // the other waves' pair work fits beside it; this chain is what the frame waits for
            if (tid < nb) {
                const int j = tid;
                const double sc = score[j];
                double bl = -INFINITY, rp = -INFINITY, ex = -INFINITY;
                if (use[a.blank] && !(full && lpv[a.blank] + sc < mincut)) bl = lpv[a.blank] + sc;
                const int cj = ech[j];
                if (cj >= 0 && use[cj] && !(full && lpv[cj] + sc < mincut)) rp = lpv[cj] + nbprev[j];
                const int P = up[j];
                if (P >= 0) {
                    const int c = upch[j];
                    if (use[c] && !(full && lpv[c] + score[P] < mincut)) {
                        if (uplpc[j] < lpv[c]) {            // get_path_trie: a better emission frame for the edge's top node
                            uplpc[j] = lpv[c];
                            NodeRec* tn = nodes + upnode[j];
                            tn->lpc = lpv[c]; tn->tstep = t0 + t;
                        }
                        if (upnode[j] == node[j]) {
                            int arcw = -1;
                            if (a.has_lm && c == a.space) arcw = a.trie_word[eds[P]];
                            ex = pair_logp(P, c, arcw);
                        }
                    }
                }
                // nb_cur = lse(rp, ex), score = lse(bl, nb_cur), written so that the two exps and the two logs are independent of
                // each other (half the dependent chain of two nested log-sum-exps; same value to ~1e-16 relative)
                const double m2 = fmax(rp, ex);
                const double e1 = (rp > -INFINITY && ex > -INFINITY) ? exp(fmin(rp, ex) - m2) : 0.0;
                const double e2 = (bl > -INFINITY && m2 > -INFINITY) ? exp(-fabs(bl - m2)) : 0.0;
                const double sum2 = 1.0 + e1;
                const double x = bl >= m2 ? 1.0 + sum2 * e2 : e2 + sum2;
                const double nbc = m2 + log(sum2), s = fmax(bl, m2) + log(x);
                e_bcur[j] = bl; e_nbcur[j] = nbc;
                key[0] = okey(s); mark[0] = 0; cidx[0] = j;
            }
            __builtin_amdgcn_s_setprio(0);
        } else if (wid < EW + SW) {
            const int i = tid - 64 * EW, c = a.space;
            if (i < nb && use[c] && !(full && lpv[c] + score[i] < mincut)) {
                cidx[0] = nb + i * C + c;
                const int r = cellc[i * C + c];
                if (!(r >= 0 && upnode[r] == node[r])) {
                    const int arc = a.trie_word[eds[i]];
                    if (r >= 0 || arc >= 0) { mark[0] = r >= 0 ? 2 + r : 1; arcv[0] = arc; key[0] = okey(pair_logp(i, c, arc)); }
                }
            }
        } else {
            int cellv[KMAX];
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {          // pass 1: what each pair is, and its dictionary arc requested
                const int p = tid - 64 * (EW + SW) + k * PT;
                cellv[k] = -1;
                if (p >= NP) continue;
                const int i = min((int)(((float)p + 0.5f) * invC), nb - 1), c = p - i * C;
                if (c == a.blank || (SW && c == a.space)) continue;
                cidx[k] = nb + p;
                if (!use[c] || (full && lpv[c] + score[i] < mincut)) continue;
                const int r = cellc[i * C + c];
                if (r >= 0 && upnode[r] == node[r]) continue;          // the child is a beam entry: it pulls this term itself
                cellv[k] = r; mark[k] = r >= 0 ? 2 + r : 1;
                if (a.has_lm && r < 0) arcv[k] = a.trie_next[(size_t)eds[i] * C + c];
            }
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {          // pass 2: scores
                if (mark[k] < 0) continue;
                const int p = cidx[k] - nb;
                const int i = min((int)(((float)p + 0.5f) * invC), nb - 1), c = p - i * C;
                if (a.has_lm && cellv[k] < 0 && arcv[k] < 0) { mark[k] = -1; continue; }     // the dictionary has no such arc (space: no word ends here)
                key[k] = okey(pair_logp(i, c, arcv[k]));
            }
        }
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const bool valid = key[k] != 0;
            if (cidx[k] >= 0) c_key[cidx[k]] = key[k];
            int bin = NBINS;
            if (valid) bin = score_bin<NBINS>(U, unokey(key[k]));
            binv[k] = bin;
            const bool lastb = valid && bin == NBINS - 1;          // the hopeless ones pile up in the last bin: one add per wave
            const unsigned long long bl = __ballot(lastb);
            if (valid && !lastb) atomicAdd(&hist[bin], 1u);
            if (bl && lane == __builtin_ctzll(bl)) atomicAdd(&hist[NBINS - 1], (unsigned)__builtin_popcountll(bl));
        }
        stamp(t, 7);
        __syncthreads();
        stamp(t, 1);

        // ---- F2: wave 0 finds the bin in which the beam_width-th best score lies; the last wave makes the next row
        if (wid == 0) {
            unsigned cnt[BPL];
            unsigned mine = 0;
#pragma unroll
            for (int q = 0; q < BPL; ++q) { cnt[q] = hist[lane * BPL + q]; hist[lane * BPL + q] = 0; mine += cnt[q]; }
            const unsigned incl = wave_incl_scan(mine);
            const unsigned total = __shfl(incl, 63, 64), excl = incl - mine;
            const unsigned long long have = __ballot(mine != 0);
            if (have && lane == __builtin_ctzll(have)) {
                int q0 = 0;
#pragma unroll
                for (int q = BPL - 1; q >= 0; --q) if (cnt[q]) q0 = q;
                sd[4] = U - (double)(lane * BPL + q0) * (BIN_SPAN / NBINS);      // no score of this frame is above the best one's bin
            }
            if (total <= (unsigned)BW) { if (lane == 0) { s_bstar = NBINS; s_r = 0; s_mb = 0; } }
            else if (excl < (unsigned)BW && incl >= (unsigned)BW) {
                unsigned run = excl;
                int q = 0;
#pragma unroll
                for (int qq = 0; qq < BPL; ++qq) if (run + cnt[qq] < (unsigned)BW && qq == q) { run += cnt[qq]; ++q; }
                unsigned hit = 0;
#pragma unroll
                for (int qq = 0; qq < BPL; ++qq) if (qq == q) hit = cnt[qq];
                s_bstar = lane * BPL + q; s_r = (int)((unsigned)BW - run); s_mb = (int)hit;
            }
        } else {
            for (int q = tid - 64; q < CELLS / 2; q += BT - 64) reinterpret_cast<int*>(celln)[q] = -1;
            if (tid == 64) { s_nlist = 0; s_nrev = 0; }
            if (wid == NWAVE - 1 && t + 1 < T) make_row(t + 1, pn0, pn1, pnb);
        }
        __syncthreads();
        stamp(t, 2);
        stamp(t, 3);

        // ---- F4: exact ranking inside the threshold bin; survivors numbered per wave
        const int bstar = s_bstar, rr = s_r, mb = s_mb;
        bool surv[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) surv[k] = key[k] != 0 && (binv[k] < bstar || (binv[k] == bstar && rr == mb));
        if (bstar < NBINS && rr != mb) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (binv[k] == bstar) {
                    const int at = atomicAdd(&s_nlist, 1);
                    if (at < LISTCAP) { l_key[at] = key[k]; l_idx[at] = cidx[k]; }
                }
            __syncthreads();
            const int nl = s_nlist;
            auto label_of = [&](int idx) { if (idx < nb) return ech[idx]; const int p = idx - nb; const int i = min((int)(((float)p + 0.5f) * invC), nb - 1); return p - i * C; };
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                if (binv[k] != bstar) continue;
                const int idx = cidx[k], myc = label_of(idx);
                const uint64_t mk = key[k];
                int rank = 0;
                if (nl <= LISTCAP) {
                    for (int q = 0; q < nl; ++q) {
                        const uint64_t ok = l_key[q]; const int oi = l_idx[q];
                        if (oi == idx) continue;
                        if (ok > mk) { ++rank; continue; }
                        if (ok == mk) { const int oc = label_of(oi); rank += (oc < myc) || (oc == myc && oi < idx); }
                    }
                    ++dbg_list;
                } else {
                    for (int q = 0; q < N; ++q) {
                        const uint64_t ok = c_key[q];
                        if (ok == 0 || q == idx || score_bin<NBINS>(U, unokey(ok)) != bstar) continue;
                        if (ok > mk) { ++rank; continue; }
                        if (ok == mk) { const int oc = label_of(q); rank += (oc < myc) || (oc == myc && q < idx); }
                    }
                    ++dbg_full;
                }
                surv[k] = rank < rr;
            }
        }
        int within[KMAX], fwithin[KMAX];
        int wcount = 0, fcount = 0;
        uint64_t kmin = ~0ull;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const unsigned long long bs = __ballot(surv[k]), bf = __ballot(surv[k] && mark[k] == 1);
            within[k] = wcount + __builtin_popcountll(bs & lt_mask); wcount += __builtin_popcountll(bs);
            fwithin[k] = fcount + __builtin_popcountll(bf & lt_mask); fcount += __builtin_popcountll(bf);
            if (surv[k] && key[k] < kmin) kmin = key[k];
        }
        if (a.has_lm) {             // the scorer's min_cutoff needs the worst score of the next beam
            for (int o = 32; o > 0; o >>= 1) { const uint64_t v = __shfl_xor(kmin, o, 64); kmin = v < kmin ? v : kmin; }
            if (lane == 0) wkmin[wid] = kmin;
        }
        if (lane == 0) { wsurv[wid] = wcount; wfresh[wid] = fcount; }
        __syncthreads();
        stamp(t, 4);

        // ---- F5: slot numbers of the next beam
        int sbase = 0, fbase = 0, nnext = 0, nfresh = 0;
        for (int w = 0; w < NWAVE; ++w) { const int v = wsurv[w], f = wfresh[w]; nnext += v; nfresh += f; if (w < wid) { sbase += v; fbase += f; } }
        if (a.has_lm && tid == 0) {
            uint64_t m = ~0ull;
            for (int w = 0; w < NWAVE; ++w) m = wkmin[w] < m ? wkmin[w] : m;
            s_kmin = m;
        }
        if (wid < EW && tid < nb) newslot[tid] = surv[0] ? sbase + within[0] : -1;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (!surv[k]) continue;
            const int sl = sbase + within[k];                          // survivors are few and scattered: listed by slot, so that
            f_key[sl] = key[k]; f_idx[sl] = cidx[k]; f_mark[sl] = mark[k]; f_arc[sl] = arcv[k]; f_fr[sl] = fbase + fwithin[k];     // one thread per new entry commits
            if (mark[k] >= 2) {
                const int p = cidx[k] - nb; const int i = min((int)(((float)p + 0.5f) * invC), nb - 1), c = p - i * C;
                cellc[i * C + c] = (short)(-2 - sl);                   // this edge's dormant top is a beam entry again
                s_nrev = 1;
            }
        }
        __syncthreads();
        stamp(t, 5);

        // ---- F6: commit
        if (s_nrev) {     // the walk below reads node records other waves have stored: have every store land first
            DSMI_WAIT_STORES();
            __syncthreads();
        }
        // an entry's edge tuple in the new slot numbers: through ancestors that left the beam, under a top that came back
        auto resolve = [&](Tup tp, int node_j, int walk_from, int walk_depth, int ch_j, double own_j) -> Tup {
            while (tp.up >= 0) {
                const int m = cellc[tp.up * C + tp.upch];
                if (m <= -2 && tp.upnode != node_j) {
                    int n = walk_from;
                    const int hops = walk_depth - depth[tp.up] - 2;
                    for (int h = 0; h < hops; ++h) n = nodes[n].parent;
                    dbg_hops += hops > 0 ? hops : 0;
                    Tup r; r.up = -2 - m; r.upnode = n;
                    if (n == node_j) { r.upch = ch_j; r.uplpc = own_j; }
                    else { const NodeRec x = nodes[n]; r.upch = x.ch; r.uplpc = x.lpc; }
                    return r;
                }
                const int ns = newslot[tp.up];
                if (ns >= 0) { tp.up = ns; return tp; }
                const int P = tp.up;                         // P left the beam: it is part of this edge now
                tp.up = up[P]; tp.upch = upch[P]; tp.upnode = upnode[P]; tp.uplpc = uplpc[P];
            }
            return Tup{-1, -1, -1, -INFINITY};
        };
        if (tid < nnext) {
            const int sl = tid, idx = f_idx[sl], mk = f_mark[sl], arcw = f_arc[sl];
            const double lg = unokey(f_key[sl]);
            const size_t o = (size_t)nxt * BW + sl;
            int* nctxp = e_ctx + o * MAXCTX;
            if (mk == 0) {                                  // an entry that stays
                const int j = idx;
                const bool direct = upnode[j] == node[j];
                const double own = direct ? uplpc[j] : ownlpc[j];
                const Tup tp = resolve(Tup{up[j], upch[j], upnode[j], uplpc[j]}, node[j], node[j], depth[j], ech[j], own);
                e_node[o] = node[j]; e_ch[o] = ech[j]; e_ds[o] = eds[j]; e_depth[o] = depth[j]; e_memo[o] = memo[j];
                e_bprev[o] = e_bcur[j]; e_nbprev[o] = e_nbcur[j]; e_score[o] = lg; e_ownlpc[o] = own;
                e_up[o] = tp.up; e_upch[o] = tp.upch; e_upnode[o] = tp.upnode; e_uplpc[o] = tp.uplpc;
                for (int q = 0; q < MAXCTX; ++q) nctxp[q] = ctx[(size_t)j * MAXCTX + q];
                if (tp.up >= 0) celln[tp.up * C + tp.upch] = (short)sl;
            } else {
            const int p = idx - nb;
            const int i = min((int)(((float)p + 0.5f) * invC), nb - 1), c = p - i * C;
            const bool sp = a.has_lm && c == a.space;
            int id; double lpc;
            if (mk == 1) {                                  // a new node
                id = nn + f_fr[sl];
                lpc = lpv[c];
                NodeRec r; r.parent = node[i]; r.ch = c; r.tstep = t0 + t; r.depth = depth[i] + 1; r.lpc = lpc; r.pad = 0.0;
                nodes[id] = r;
            } else {                                             // a dormant prefix is back: same node, its log_prob_c kept
                const int rep = mk - 2;
                id = upnode[rep]; lpc = uplpc[rep];
                ++dbg_rev;
            }
            int nds = 0;
            if (a.has_lm && !sp) nds = mk == 1 ? arcw : a.trie_next[(size_t)eds[i] * C + c];
            const int* pctx = ctx + (size_t)i * MAXCTX;
            for (int q = 0; q < MAXCTX; ++q) {
                int v = pctx[q];
                if (sp) v = q + 1 < NCTX ? pctx[q + 1] : (q + 1 == NCTX ? arcw : a.bos);
                nctxp[q] = v;
            }
            Tup tp{newslot[i], c, id, lpc};
            if (tp.up < 0) tp = resolve(Tup{up[i], upch[i], upnode[i], uplpc[i]}, id, node[i], depth[i], c, lpc);
#ifdef SIMT_EMU
            if (tp.up >= BW || tp.up < -1) std::fprintf(stderr, "t=%d tid=%d idx=%d mark=%d i=%d c=%d sl=%d nb=%d newslot[i]=%d up[i]=%d tp.up=%d\n", t, tid, idx, mk, i, c, sl, nb, newslot[i], up[i], tp.up);
#endif
            e_node[o] = id; e_ch[o] = c; e_ds[o] = nds; e_depth[o] = depth[i] + 1; e_memo[o] = MEMO_UNSET;
            e_bprev[o] = -INFINITY; e_nbprev[o] = lg; e_score[o] = lg; e_ownlpc[o] = lpc;
            e_up[o] = tp.up; e_upch[o] = tp.upch; e_upnode[o] = tp.upnode; e_uplpc[o] = tp.uplpc;
            if (tp.up >= 0) celln[tp.up * C + tp.upch] = (short)sl;
            }
        }
        nn += nfresh;
        if (tid == 0) s_nb = nnext;
        __syncthreads();
        stamp(t, 6);
        cur = nxt;
    }

    // ---- final: trailing partial word, order, write out
    DSMI_WAIT_STORES();
    __syncthreads();
    if constexpr (RESUME) {
        // ---- save the carried search (the final section below then works on the LDS copy)
        const StreamState ks = stream_state(BW, C);
        unsigned char* st = sdsc->state;
        const int nb = s_nb;
        const size_t o = (size_t)cur * BW;
        for (int j = tid; j < nb; j += BT) {
            reinterpret_cast<double*>(st + ks.bprev)[j] = e_bprev[o + j]; reinterpret_cast<double*>(st + ks.nbprev)[j] = e_nbprev[o + j];
            reinterpret_cast<double*>(st + ks.score)[j] = e_score[o + j]; reinterpret_cast<double*>(st + ks.uplpc)[j] = e_uplpc[o + j];
            reinterpret_cast<double*>(st + ks.ownlpc)[j] = e_ownlpc[o + j];
            reinterpret_cast<int*>(st + ks.node)[j] = e_node[o + j]; reinterpret_cast<int*>(st + ks.ch)[j] = e_ch[o + j];
            reinterpret_cast<int*>(st + ks.ds)[j] = e_ds[o + j]; reinterpret_cast<int*>(st + ks.depth)[j] = e_depth[o + j];
            reinterpret_cast<int*>(st + ks.up)[j] = e_up[o + j]; reinterpret_cast<int*>(st + ks.upch)[j] = e_upch[o + j];
            reinterpret_cast<int*>(st + ks.upnode)[j] = e_upnode[o + j]; reinterpret_cast<int*>(st + ks.memo)[j] = e_memo[o + j];
            for (int k = 0; k < MAXCTX; ++k) reinterpret_cast<int*>(st + ks.ctx)[(size_t)j * MAXCTX + k] = e_ctx[(o + j) * MAXCTX + k];
        }
        const int* cellv = reinterpret_cast<const int*>(cell + (size_t)cur * CELLS);
        for (int q = tid; q < CELLS / 2; q += BT) reinterpret_cast<int*>(st + ks.cell)[q] = cellv[q];
        if (tid == 0) { StreamHdr h; h.nb = nb; h.nn = nn; h.kmin = s_kmin; h.bound = sd[4]; h.pad = 0.0; *reinterpret_cast<StreamHdr*>(st + ks.hdr) = h; }
        __syncthreads();
    }
    if (!RESUME || sdsc->n_best > 0) {
        const int nb = s_nb;
        double* score = e_score + cur * BW; const int* node = e_node + cur * BW; const int* ech = e_ch + cur * BW;
        const int* eds = e_ds + cur * BW; const int* depth = e_depth + cur * BW; const int* ctx = e_ctx + (size_t)cur * BW * MAXCTX;
        if (a.has_lm) {
            for (int i = tid; i < nb; i += BT) {
                if (node[i] != 0 && ech[i] != a.space) {
                    const int w = a.trie_word[eds[i]];
                    double lm = kOovScore;
                    if (w >= 0) lm = (double)lm_word_log10(s_lm, ctx + (size_t)i * MAXCTX, NCTX, w, a.unk) / (double)kLog10E;
                    double s = lm * a.alpha;
                    s += a.beta;
                    score[i] += s;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < nb; i += BT) {
            int rank = 0;
            for (int j = 0; j < nb; ++j) {
                if (j == i) continue;
                rank += score[j] > score[i] || (score[j] == score[i] && (ech[j] < ech[i] || (ech[j] == ech[i] && j < i)));
            }
            const int len = depth[i];
            if constexpr (RESUME) {
                if (rank >= sdsc->n_best) continue;
                const size_t o = (size_t)rank * sdsc->out_T;
                int n = node[i];
                for (int k = len - 1; k >= 0; --k) { const NodeRec r = nodes[n]; sdsc->out_tok[o + k] = r.ch; sdsc->out_step[o + k] = r.tstep; n = r.parent; }
                sdsc->out_len[rank] = len;
                sdsc->out_score[rank] = score[i];
                continue;
            }
            const size_t o = ((size_t)b * BW + rank) * a.T;
            int n = node[i];
            for (int k = len - 1; k >= 0; --k) { const NodeRec r = nodes[n]; a.out_tok[o + k] = r.ch; a.out_step[o + k] = r.tstep; n = r.parent; }
            a.out_len[(size_t)b * BW + rank] = len;
            a.out_score[(size_t)b * BW + rank] = score[i];
        }
        if (tid == 0) { if constexpr (RESUME) *sdsc->out_n = min(nb, sdsc->n_best); else a.out_n[b] = nb; }
    }
    if (a.dbg) {
        dbg_rev = wave_sum(dbg_rev); dbg_hops = wave_sum(dbg_hops); dbg_list = wave_sum(dbg_list); dbg_full = wave_sum(dbg_full);
        if (lane == 0) { atomicAdd(a.dbg + 4 * b, dbg_rev); atomicAdd(a.dbg + 4 * b + 1, dbg_hops); atomicAdd(a.dbg + 4 * b + 2, dbg_list); atomicAdd(a.dbg + 4 * b + 3, dbg_full); }
    }
#undef s_nb
#undef s_bstar
#undef s_r
#undef s_mb
#undef s_nlist
#undef s_nrev
#undef s_kmin
}

}  // namespace
