// First conv layer -- Conv2d(1 -> 32, k = 41 x 11, stride 2 x 2, pad 20 x 5) + bias + BatchNorm2d(eval) + Hardtanh(0, 20) +
// MaskConv (reference danspeech/deepspeech/model.py:65-81, 358-371) -- on the fp16 MFMA with two-term split operands
// (x = hi + lo * 2^-11, three products, two fp32 accumulators: gemm.hip / conv_split.hip), instead of the fp32 MFMA of
// conv.hip, which runs at 1/16 of the fp16 rate (conv.hip stays as the plain fp32 statement and the fallback).
//
// One input channel gives the MFMA's K nothing to contract, so K is the kernel's TIME axis: one v_mfma_f32_32x32x16_f16
// contracts the 11 taps of one kernel row kf (padded to 16 with zero weights): A = weights [32 output channels][16 taps],
// B = input patch [16 taps][32 output steps].  A lane's B fragment is 8 consecutive input samples of row 2 f + kf - 20
// starting at 2 t - 5 + 8 hk: the time stride of 2 makes the start of neighbouring output steps 4 bytes apart, so
//   * the two column tiles of a wave take the EVEN and the ODD output steps (t = t0 + 2 li, t0 + 2 li + 1), and
//   * the staged rows exist twice in LDS, the second copy shifted by two samples,
// which makes every fragment two aligned 8-byte LDS reads at consecutive 8-byte addresses across the lanes (no bank
// conflicts).  The window of a workgroup (8 output rows x 64 output steps: 55 input rows x 137 samples) is split into its
// two fp16 terms once while it is staged.  Weight fragments come from L2 (82 KB for all 41 kernel rows), one row ahead.
#include "common.h"
#include <algorithm>

namespace dsmi {

namespace {

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
constexpr float kLoScale = 2048.f, kLoInv = 1.f / 2048.f;

constexpr int KF = 41, KT = 11, SF = 2, ST = 2, PF = 20, PT = 5, CO = 32;
constexpr int C1NF = 8;                        // output rows per workgroup (one per wave: 8 waves)
constexpr int C1NT = C1NF * 64;                // threads per workgroup
constexpr int C1TT = 64;                       // output steps per workgroup: an even and an odd column tile of 32
constexpr int ROWS = SF * (C1NF - 1) + KF;     // staged input rows: 55 (the 41-row halo is shared by 8 output rows)
constexpr int WIN = ST * (C1TT - 1) + KT + 5;  // samples a fragment may touch: 2 * 63 + 16 = 142
constexpr int PITCH = 144;                     // halfs per staged row (288 B: rows start 8-byte aligned)
constexpr int COPY = ROWS * PITCH;             // halfs per (plane, copy)
constexpr size_t C1_LDS = (size_t)2 * 2 * COPY * 2;   // planes x copies x halfs x 2 B = 63 360 B: two workgroups per CU

struct Conv1Args {
    const float* x; const uint16_t* wp; const float* bias; const float* bn_a; const float* bn_b; const int32_t* out_lens;
    float* y; uint16_t* y_sp;
    int B, fi, fo, ti, to, xs, ys;
    unsigned* tile_cnt;     // tiles by demand (conv_rows.h, dense_tiles.h): kDenseCntWords words, zero between launches; null: one workgroup per tile
};

// Kernel rows that read only the frequency padding are neither staged nor multiplied (conv_rows.h: a wave walks its own row's range;
// the rows no live wave reads stay unwritten).  BY_DEMAND: the workgroups of a by-demand launch take tile after tile (TileTaker,
// dense_tiles.h; a label's share is whole groups of f-neighbours, conv_rows.h); here: the ticket's word, the barriers around it, and
// what is derived per tile so that it does not live through the kernel rows.
// (Two workgroups per CU are sixteen waves: 128 registers each.  The static form takes 94; the by-demand form takes 128 / 126, exactly the
// limit -- any addition to its tile loop can spill: check -Rpass-analysis=kernel-resource-usage after a change.  How the compiler
// orders the kernel-row loop of the by-demand form also moves with the locals declared behind it: profiles/tile_taker.txt.)
template <bool SPLIT_OUT, bool BY_DEMAND = false>
__global__ __launch_bounds__(C1NT, 4) void conv1_f16x3_kernel(Conv1Args p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char c1sm[];
    _Float16* Xs = reinterpret_cast<_Float16*>(c1sm);      // [plane 2][copy 2][ROWS][PITCH]; copy 1 holds the row shifted by 2 samples
    const int tid0 = threadIdx.x;
    const int wv = __builtin_amdgcn_readfirstlane(tid0 >> 6);
    const ConvGrid grid{(p.to + C1TT - 1) / C1TT, (p.fo + C1NF - 1) / C1NF, p.B};
    const int total = conv_total(grid), label = blockIdx.x & 7;
    // the linear index of the workgroup's tile (-1: none left); lane 0 writes it, everybody reads it behind a barrier
    volatile int* const tk_lds = reinterpret_cast<volatile int*>(c1sm + C1_LDS);
    const TileCounters cnt{p.tile_cnt};
    unsigned dead = 0;      // lane 0's: the labels this workgroup has found used up (every tile's TileTaker works on it)
    if (BY_DEMAND) {
        if (tid0 == 0) tk_lds[0] = TileTaker(total, label, grid.nf, dead).first(cnt);
        __syncthreads();
    }
  // Every barrier below is reached by all eight waves of the workgroup, tile after tile: f < p.fo guards multiplications and stores
  // only, and a masked tile is uniform over the workgroup.
  for (;;) {
    // (by demand: what a tile derives from the lane is derived per tile -- hoisted out of the tile loop it would stay in registers
    // through the kernel rows)
    int tid = tid0;
    if (BY_DEMAND) asm volatile("" : "+v"(tid));
    const int lane = tid & 63, li = lane & 31, hk = lane >> 5;
    ConvTile tile;
    if (BY_DEMAND) {
        const int idx = __builtin_amdgcn_readfirstlane(tk_lds[0]);
        if (idx < 0) break;
        tile = conv_tile_at(grid, idx);
    } else {
        tile = ConvTile{(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z};
    }
    const int t0 = tile.tt * C1TT, f0 = tile.ft * C1NF, b = tile.z;
    const int f = f0 + wv;
    const int olen = p.out_lens[b];
    // (by demand: the epilogue's per-channel constants are loaded per tile -- hoisted out of the tile loop they would stay in registers
    // through the kernel rows)
    const float *bias = p.bias, *bn_a = p.bn_a, *bn_b = p.bn_b;
    if (BY_DEMAND) asm volatile("" : "+s"(bias), "+s"(bn_a), "+s"(bn_b));
    // the next tile's ticket goes out in front of this tile's stores and is redeemed behind them
    TileTaker taker(total, label, grid.nf, dead);
    auto ask = [&] { if (BY_DEMAND && tid == 0) taker.ask(cnt); };

    if (t0 >= olen) {     // fully masked tile: zeros in the consumer's format
        ask();
        if (SPLIT_OUT) {
            for (int idx = tid; idx < C1NF * 2 * C1TT * 4; idx += C1NT) {
                const int part = idx & 3, tl = (idx >> 2) % C1TT, pl = (idx / (4 * C1TT)) % 2, ff = idx / (4 * C1TT * 2);
                if (f0 + ff < p.fo && t0 + tl < p.to)
                    *reinterpret_cast<u32x4*>(reinterpret_cast<_Float16*>(p.y_sp) + ((((size_t)b * p.fo + f0 + ff) * 2 + pl) * p.to + t0 + tl) * 32 + part * 8) = u32x4{0, 0, 0, 0};
            }
        } else {
            for (int idx = tid; idx < CO * C1NF * C1TT; idx += C1NT) {
                const int tl = idx % C1TT, ff = (idx / C1TT) % C1NF, co = idx / (C1TT * C1NF);
                if (f0 + ff < p.fo && t0 + tl < p.to) p.y[(((size_t)b * CO + co) * p.fo + f0 + ff) * p.ys + t0 + tl] = 0.f;
            }
        }
        if (BY_DEMAND) __syncthreads();      // everybody has read this tile's ticket before lane 0 writes the next one
    } else {
    // ---- stage the window, split into (hi, lo * 2^11), twice: thread -> (row, pair of adjacent samples).  Wave w at kernel row kf
    // reads staged row SF w + kf = input row fin0 + SF w + kf, and only where that is a real row (its range below): the staged rows
    // anybody reads are the real input rows up to the last live wave's last one, and only those are written.
    const int fin0 = SF * f0 - PF, tin0 = ST * t0 - PT;        // input row / column of staged (0, 0)
    const int nlive = min(C1NF, p.fo - f0);
    const int row_lo = max(0, -fin0), row_hi = min(SF * (nlive - 1) + KF - 1, p.fi - 1 - fin0);
    for (int idx = tid + row_lo * (PITCH / 2); idx < (row_hi + 1) * (PITCH / 2); idx += C1NT) {
        const int row = idx / (PITCH / 2), q = 2 * (idx - row * (PITCH / 2));
        const int fin = fin0 + row;
        float v[2] = {0.f, 0.f};
        {
            const float* src = p.x + ((size_t)b * p.fi + fin) * p.xs;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int tin = tin0 + q + e;
                if (tin >= 0 && tin < p.ti && q + e < WIN) v[e] = src[tin];
            }
        }
        f16x2 h, l;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const _Float16 hi = (_Float16)v[e];
            h[e] = hi; l[e] = (_Float16)((v[e] - (float)hi) * kLoScale);
        }
        _Float16* r0 = Xs + row * PITCH + q;
        *reinterpret_cast<f16x2*>(r0) = h;                                   // plane 0, copy 0
        *reinterpret_cast<f16x2*>(r0 + 2 * COPY) = l;                        // plane 1, copy 0
        if (q >= 2) {
            *reinterpret_cast<f16x2*>(r0 + COPY - 2) = h;                    // plane 0, copy 1: sample q at index q - 2
            *reinterpret_cast<f16x2*>(r0 + 3 * COPY - 2) = l;                // plane 1, copy 1
        }
    }
    __syncthreads();
    if (f < p.fo) {
    const ConvRows myr = conv_rows_of(f, p.fi, KF, PF, SF);

    f32x16 acc[2], acl[2];      // [column tile: even / odd steps]  hi.hi ; (hi.lo + lo.hi) * 2^11
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[tt][r] = 0.f; acl[tt][r] = 0.f; }

    // B fragment of column tile tt, plane pl, kernel row kf: samples 2 (2 li + tt) + 8 hk .. + 7 of staged row 2 wv + kf
    //   tt = 0: copy 0 at index 4 li + 8 hk;   tt = 1: copy 1 at index (4 li + 2 + 8 hk) - 2 = 4 li + 8 hk
    const _Float16* xb = Xs + (SF * wv) * PITCH + 4 * li + 8 * hk;
    const u32x4* wq = reinterpret_cast<const u32x4*>(p.wp) + lane;          // [kf][plane][lane] 16-byte fragments
    const int kfirst = min(myr.lo, KF - 1);                                   // (an empty range multiplies nothing)
    u32x4 wn[2] = {wq[(size_t)kfirst * 128], wq[(size_t)kfirst * 128 + 64]};
#pragma unroll 1
    for (int kf = myr.lo; kf <= myr.hi; ++kf) {
        const f16x8 wh = __builtin_bit_cast(f16x8, wn[0]), wl = __builtin_bit_cast(f16x8, wn[1]);
        if (kf + 1 < KF) { wn[0] = wq[(size_t)(kf + 1) * 128]; wn[1] = wq[(size_t)(kf + 1) * 128 + 64]; }     // next row's weights, from L2
        const _Float16* xr = xb + kf * PITCH;
        f16x8 xh[2], xl[2];
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const f16x4 a0 = *reinterpret_cast<const f16x4*>(xr + tt * COPY), a1 = *reinterpret_cast<const f16x4*>(xr + tt * COPY + 4);
            const f16x4 b0 = *reinterpret_cast<const f16x4*>(xr + (2 + tt) * COPY), b1 = *reinterpret_cast<const f16x4*>(xr + (2 + tt) * COPY + 4);
            xh[tt] = f16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            xl[tt] = f16x8{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) acl[tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl, xh[tt], acl[tt], 0, 0, 0);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) acc[tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xh[tt], acc[tt], 0, 0, 0);
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) acl[tt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, xl[tt], acl[tt], 0, 0, 0);
    }

    ask();
    // ---- epilogue: D[i = output channel][j = li]: output step t0 + 2 li + tt
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
        const int t = t0 + 2 * li + tt;
        if (t >= p.to) continue;
        if (SPLIT_OUT) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f16x4 h, l;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = q + 8 * g + 4 * hk;
                    float v = (acc[tt][4 * g + q] + acl[tt][4 * g + q] * kLoInv + bias[co]) * bn_a[co] + bn_b[co];
                    v = fminf(fmaxf(v, 0.f), 20.f);
                    v = t < olen ? v : 0.f;
                    const _Float16 a = (_Float16)v;
                    h[q] = a; l[q] = (_Float16)(v - (float)a);        // UNSCALED lo term: the operand format of conv_split.hip
                }
                _Float16* base = reinterpret_cast<_Float16*>(p.y_sp) + ((((size_t)b * p.fo + f) * 2) * (size_t)p.to + t) * 32 + 8 * g + 4 * hk;
                *reinterpret_cast<f16x4*>(base) = h;
                *reinterpret_cast<f16x4*>(base + (size_t)p.to * 32) = l;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = (r & 3) + 8 * (r >> 2) + 4 * hk;
                float v = (acc[tt][r] + acl[tt][r] * kLoInv + bias[co]) * bn_a[co] + bn_b[co];
                v = fminf(fmaxf(v, 0.f), 20.f);
                p.y[(((size_t)b * CO + co) * p.fo + f) * p.ys + t] = t < olen ? v : 0.f;
            }
        }
    }
    }      // f < p.fo
    }      // not a masked tile
    if (!BY_DEMAND) break;
    if (tid == 0) tk_lds[0] = taker.next(cnt);
    // Every live wave is past its last read of the window (its kernel-row loop has ended: the fragments are in registers before the
    // MFMAs that take them) and everybody past this tile's ticket (the barrier behind the staging, or the masked tile's own): behind
    // this one the next tile's staging may overwrite the window.
    __syncthreads();
  }
    if (BY_DEMAND && tid0 == 0) tiles_leave(cnt);
}

}  // namespace

// w [32][1][41][11] fp32 -> [kf][plane][lane 64][8] fp16 terms (hi, lo * 2^11): lane (co = lane & 31, hk = lane >> 5) element e
// holds tap kt = 8 hk + e of kernel row kf (0 for kt >= 11).
std::vector<uint16_t> pack_conv1_w_split(const float* w) {
    std::vector<uint16_t> out((size_t)KF * 2 * 64 * 8, 0);
    for (int kf = 0; kf < KF; ++kf)
        for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 8; ++e) {
                const int co = lane & 31, kt = 8 * (lane >> 5) + e;
                if (kt >= KT) continue;
                const F16Pair x = f16_split_bits(w[((size_t)co * KF + kf) * KT + kt], kLoScale);
                const size_t base = (((size_t)kf * 2) * 64 + lane) * 8 + e;
                out[base] = x.hi; out[base + 512] = x.lo;
            }
    return out;
}

namespace {
// the kernel's 62 KB of LDS (+ the ticket's word, in every form) are above the default limit
template <bool SPLIT_OUT, bool BY_DEMAND>
void launch_conv1_form(const Conv1Args& a, dim3 grid, size_t lds, EvPair ev, hipStream_t s) {
    lds_once<conv1_f16x3_kernel<SPLIT_OUT, BY_DEMAND>>((int)C1_LDS + kTileTicketLds);
    DSMI_LAUNCH((conv1_f16x3_kernel<SPLIT_OUT, BY_DEMAND>), grid, dim3(C1NT), lds, s, ev, a);
}
}  // namespace

int launch_conv1_split(const ConvLaunch& c, const uint16_t* wp_sp, hipStream_t s) {
    Conv1Args a{c.x, wp_sp, c.bias, c.bn_a, c.bn_b, c.out_lens_dev, c.y, c.y_sp, c.B, c.fi, c.fo, c.ti, c.to, c.xs, c.ys,
                c.n_cus > 0 ? c.tile_cnt : nullptr};
    const ConvGrid g{ceil_div(c.to, C1TT), ceil_div(c.fo, C1NF), c.B};
    if (a.tile_cnt) {      // tiles by demand
        const dim3 gridd(tiles_workgroups(conv_total(g), c.n_cus));
        if (c.y_sp) launch_conv1_form<true, true>(a, gridd, C1_LDS + kTileTicketLds, c.ev, s);
        else launch_conv1_form<false, true>(a, gridd, C1_LDS + kTileTicketLds, c.ev, s);
        return (int)gridd.x;
    }
    const dim3 grid(g.nt, g.nf, g.nz);
    if (c.y_sp) launch_conv1_form<true, false>(a, grid, C1_LDS, c.ev, s);
    else launch_conv1_form<false, false>(a, grid, C1_LDS, c.ev, s);
    return g.nt * g.nf * g.nz;
}

}  // namespace dsmi
