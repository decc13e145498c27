// Persistent recurrent layer, ring variant on the whole register file: one workgroup of FOUR waves (one per SIMD, up to 512
// registers each) owns 32 hidden units of one direction and walks every batch tile of its window round-robin, with the tiles'
// packed states staged through a two-slot ring in LDS -- and every wave does the cell of the previous item in the shadows of
// the current item's MFMAs.
//
// Same arithmetic, packed weights, x-projection order, state layout and hand-off protocol as rnn_persist16.hip /
// rnn_persist_duo.hip (split-fp16 products on v_mfma_f32_16x16x32_f16, sc1 stores / sc1 loads, sharded agent-scope counter per
// (chain, step), bounded spins); replaces reference danspeech/deepspeech/model.py:114-122 (the nn.GRU / nn.LSTM / nn.RNN call
// inside BatchRNN.forward on a packed batch).  Beside the eight-wave form (rnn_persist_ring.hip: two halves taking turns on the
// matrix pipe, each with a cell slot of its own -- a slot as long as a GRU cell's dependent chain in ONE wave per SIMD, 0.90 us, of
// which the partner's 63 MFMAs needed 0.58): 6.4 against 7.2 us per step of a four-tile window of cfgA alone on the chip.  The
// eight-wave form stays for windows of one or two tiles (this form's phase has no branch: it multiplies phantom tiles like real
// ones): rnn_plan.h picks.  Every form measured on the way, and what bounds this one: profiles/r05_ring_experiments.txt, DESIGN.md 4.
//
//   * Wave (mh, kh): the 16-unit group mh of the workgroup's two ADJACENT groups (virtual workgroups 2 w and 2 w + 1 of the
//     16-unit geometry) and the half kh of the k-blocks.  Its W_hh -- up to 14 k-blocks x G gates x 2 planes x 4 registers = 336
//     -- stays in registers for the whole layer: the first 256 / (8 G) k-blocks in AccVGPRs, read by the MFMAs as their A
//     operands directly (the file is compiled with -mllvm -amdgpu-mfma-vgpr-form=1: results in VGPRs, no v_accvgpr copies),
//     the rest in VGPRs.  One wave per SIMD is what makes the file 512 registers deep.
//   * One phase per item q = (step s, tile j) = NT s + j, one workgroup barrier per phase:
//
//        P_q:  signal item q - 2  |  MFMAs of item q (B operands from ring slot q & 1, read two k-blocks ahead) with the cell of
//              item q - 1 (K-split reduction, cell, publish, output row), the state requests of item q + 1 and the poll's first
//              read for item q + 2 between them  |  drain: vmcnt(0)  |  x-projection requests for item q + 1  |  partial tiles
//              -> LDS  |  poll answered  |  barrier
//
//     so the matrix pipe of every SIMD works in every phase, and a chain's hand-off (cell -> store drain -> signal -> everybody's
//     signal visible -> state DMA -> MFMAs) lies under the other tiles' phases: NT - 1 of them.
//   * No vector-memory LOAD in the loop is visible to the compiler (state, x-projection and polls all arrive by LDS-DMA issued
//     from assembly): the compiler's wait for a load it knows of is vmcnt(0) wherever the value is used, and would wait for
//     everything in flight.  The kernel waits ONCE per phase, at the drain.  Stores and loads do not complete in order against
//     each other (loads do among themselves), so a counted wait cannot leave a load in flight past a store that must be drained.
//   * The K-split reduction is two-way (the eight-wave form: four-way): a lane writes its 4 units x 1 clip of a gate as one
//     16-byte store, the cell's thread -- (clip, two adjacent units) -- reads 8 bytes per gate and K-half.  Reduce buffers and the
//     x-projection's landing zone are double-buffered by the item's parity, which is what lets ONE barrier per phase order them.
//   * The x-projection of an item comes by LDS-DMA, 16 bytes per lane, 1 KiB per instruction ([16 clips][16 units] of one gate
//     and group).  It comes from HBM: the slowest request -- so it goes out BEHIND the phase's one drain (vmcnt(0): publish stores
//     drained, state requests landed, poll back), is the only thing in flight across the barrier and has the whole next phase to
//     land: three landing zones in rotation (requested at the end of P_q, landed by the drain of P_q+1, read in P_q+2).
//   * Publish: the four lanes of a (clip, 8-unit k-group) exchange their (hi | lo << 16) words by DPP quad broadcasts; the first
//     of them stores the 16 bytes of the hi plane, the second those of the lo plane, in ONE sc1 store instruction.  Stores carry no
//     branch: a lane with nothing to store has an offset beyond the buffer's range.
//   * The body of a phase is ONE basic block (no branch between the first MFMA and the last): requests that do not apply are
//     clamped onto valid, harmless ones instead of being skipped, step 0 (h = 0: no MFMAs, no state) is a prologue of its own.
#include "rnn_launch.h"
#include "rnn_cell.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace dsmi {

namespace {

constexpr int XNT = 256;               // 4 waves: (group mh = v & 1, K half kh = v >> 1)
constexpr int XU = kTileUnits;         // hidden units per group
constexpr int XB = kTileClips;         // clips per batch tile
constexpr int XMAXT = kRing4MaxTiles;  // tiles a window walks at most

using u32x4 = __attribute__((ext_vector_type(4))) unsigned int;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned int;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
constexpr float kLoScale = 2048.f, kLoInv = 1.f / 2048.f;

struct Ring4Args {
    const uint16_t* whh[2];    // pack_whh16 per direction
    const float* bhh[2]; const float* xp; float* out[2];
    const int32_t* lens; uint16_t* hpack; unsigned* cnt; unsigned* err;
    int B, T, H, Hs, Np, nwg16, nkb;
    int ntiles, D;             // 16-clip tiles of the whole batch (state and counter layout), directions
    int tile0, ntw, tile_end;  // window z (blockIdx.z) walks tiles tile0 + z * ntw .. + ntw - 1, below tile_end
    unsigned spin_limit;
    int drop_wg, drop_step;
    unsigned* tickets;         // [windows][2 directions] zeroed before the launch (null: a workgroup is (blockIdx.x, blockIdx.y)): see the prologue
    unsigned long long* dbg;   // diagnostics build only: per wave, 100 MHz ticks: [0] phase work (to the end of the partial tiles),
                               // [1] (unused), [2] poll spin (wave 0), [3] barrier; [4] shader cycles of the phase work; [5] polls whose first read was too early, [6] re-reads; [7] phases
};

// A wave-uniform pointer as an "s" operand of inline assembly: under scalar-register pressure the compiler computes such addresses
// on the vector unit and hands the assembly a VGPR pair for an "s" constraint (rejected by the assembler at best); through
// readfirstlane the operand is scalar whatever its history.
template <class T>
__device__ __forceinline__ const T* uni_ptr(const T* q) {
    const unsigned long long a = reinterpret_cast<unsigned long long>(q);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return reinterpret_cast<const T*>(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ void ring4_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }




// SKIP (timing experiments only, DSMI_DEBUG_RING_SKIP; results are garbage): 1 no state DMA, 2 no MFMAs, 4 polls taken as answered,
// 8 no x-projection requests, 16 no output / publish stores, 32 no cell
template <int KIND, int NKW, int NT, bool STAMP = false, int SKIP = 0>
__global__ __launch_bounds__(XNT) void rnn_persist_ring4_kernel(Ring4Args p) {
    constexpr int NG = KIND == DSMI_RNN_GRU ? 3 : (KIND == DSMI_RNN_LSTM ? 4 : 1);
    constexpr int NKA = NKW * NG * 8 <= 256 ? NKW : 256 / (NG * 8);      // k-blocks of W_hh held in AccVGPRs
    constexpr int NKD = (NKW + 1) / 2;                                    // k-blocks of an item's state one wave brings
    constexpr int XJ = (2 * NG + 3) / 4;                                  // x-projection requests per wave and item
    static_assert(NT >= 4 && NT <= XMAXT && (NT & 1) == 0, "the ring has two slots: an even number of tiles");
    extern __shared__ __attribute__((aligned(16))) unsigned char xlds[];
    const int sbytes = p.nkb * 2048;
    unsigned char* sbuf = xlds;                                                   // [2 ring slots][nkb][2 planes][1024]
    // reduce buffers: rows of 16 words (a clip's 16 units of one gate), a row's four 4-word blocks stored at block ^ ((clip >> 2) & 3):
    // conflict-free for the 16-byte stores (lane -> clip l & 15, block l >> 4) and the 8-byte reads (8 lanes per clip) alike
    constexpr int RED_G = 256;                                                    // words of one (buffer, group, K half, gate)
    constexpr int RED_BUF = 2 * 2 * NG * RED_G;
    constexpr int XGB = 2 * NG * 1024;                                            // bytes of one x-projection landing zone
    float* red_all = reinterpret_cast<float*>(xlds + 2 * sbytes);                 // [2 buffers][2 groups][2 K halves][NG][16 clips][16]
    float* xgl = red_all + 2 * RED_BUF;                                           // [3 zones][2 groups][NG][16 clips][16 units]
    int* sync = reinterpret_cast<int*>(xgl + 3 * 2 * NG * 256);                   // [0] dead flag (a hand-off wait timed out: stop waiting)
    unsigned long long* tacc = reinterpret_cast<unsigned long long*>(sync + 32) + (STAMP ? (threadIdx.x >> 6) * 8 : 0);
    const int tid = threadIdx.x, lane = tid & 63;
    const int v = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mh = v & 1, kh = v >> 1;
    const int ln = lane & 15, lg = lane >> 4;
    // Which (direction, unit group) this workgroup is.  A tile's packed state is read by every workgroup of its direction every
    // step, and every XCD's L2 that holds one of them fetches it from the fabric: the launch's workgroups land on the eight XCDs
    // round-robin, so with (blockIdx.x, blockIdx.y) a direction's workgroups sit on all eight.  With tickets, the workgroups that
    // find themselves on XCDs 0-3 (HW_REG_XCC_ID) take direction 0's unit groups in the order they arrive, those on 4-7 direction
    // 1's; whoever finds its direction full takes the other (speed only: any bijection is correct).  Four L2s fetch a tile's state
    // per step instead of eight.
    int w32 = blockIdx.x, d = blockIdx.y;
    if (p.tickets && p.D == 2) {
        const int nw = (p.nwg16 + 1) >> 1;
        if (tid == 0) {
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            unsigned* tk = p.tickets + 2 * blockIdx.z;
            unsigned want = (xcc >> 2) & 1u;
            unsigned t = atomicAdd(&tk[want], 1u);
            if (t >= (unsigned)nw) { want ^= 1u; t = atomicAdd(&tk[want], 1u); }
            sync[30] = (int)want; sync[31] = (int)t;
        }
        ring4_barrier();
        d = __builtin_amdgcn_readfirstlane(sync[30]);
        w32 = __builtin_amdgcn_readfirstlane(sync[31]);
        ring4_barrier();         // (sync[] is zeroed below)
    }
    const int tile0 = p.tile0 + (int)blockIdx.z * p.ntw;
    const int nt = min(min(p.ntw, p.tile_end - tile0), NT);
    const int w16 = 2 * w32 + mh;
    const bool half_ok = w16 < p.nwg16;
    const int nwg32 = (p.nwg16 + 1) >> 1;
    constexpr int GU = NG * XU;
    {   // ring slots (step 0 multiplies nothing, but a phantom k-block is read), reduce buffers (the prologue's cells read zeros)
        u32x4* z = reinterpret_cast<u32x4*>(xlds);
        const int n16 = (2 * sbytes + (2 * RED_BUF + 3 * 2 * NG * 256) * 4) / 16;
        for (int i = tid; i < n16; i += XNT) z[i] = u32x4{0u, 0u, 0u, 0u};
    }
    if (tid < 32) sync[tid] = 0;
    if (STAMP && lane < 8) tacc[lane] = 0;

    // ---- resident operand: this wave's k-blocks [kb0, kb1) of its group's split W_hh, all gates; a wave of the second half may own
    // one block fewer than NKW: its phantom block is zero and multiplies the wave's last real block of state
    const int kb0 = kh ? (p.nkb + 1) / 2 : 0, kb1 = kh ? p.nkb : (p.nkb + 1) / 2;
    f16x8 wv[NKW][NG][2];
    {
        const u32x4* wp = reinterpret_cast<const u32x4*>(p.whh[d]) + ((size_t)(half_ok ? w16 : 0) * p.nkb) * (NG * 2 * 64) + lane;
#pragma unroll
        for (int i = 0; i < NKW; ++i) {
            const bool real = half_ok && kb0 + i < kb1;
            const int kb = min(kb0 + i, p.nkb - 1);
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
                    u32x4 w = wp[(((size_t)kb * NG + g) * 2 + pl) * 64];
                    if (!real) w = u32x4{0u, 0u, 0u, 0u};
                    wv[i][g][pl] = __builtin_bit_cast(f16x8, w);
                    if (i < NKA) asm volatile("" : "+a"(wv[i][g][pl]));       // into its AccVGPRs as it arrives
                }
        }
    }
    const unsigned hp_par = (unsigned)((size_t)p.D * p.ntiles * p.nkb * 2048);     // bytes per parity
    const __amdgpu_buffer_rsrc_t hrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.hpack, 0, (int)(2 * hp_par), 0x00020000);
    float* outd = p.out[d];
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc((void*)outd, 0, (int)((size_t)p.T * p.B * p.Hs * 4), 0x00020000);
    const unsigned lds_sbuf = (unsigned)(size_t)sbuf;
    const unsigned lane16 = (unsigned)lane * 16u;
    const unsigned char* sbr = sbuf + lane16 + kb0 * 2048;       // this lane's fragment of its wave's first k-block, ring slot 0
    const int klast_off = (min(kb0 + NKW - 1, p.nkb - 1) - kb0) * 2048;     // the last (possibly phantom) block's offset from sbr

    // ---- per tile (uniform): chain, counters, row blocks; a phantom tile (J >= nt) is computed like a real one on the LAST real
    // tile's addresses with every store out of range
    const int chain0 = d * p.ntiles + tile0;
    const unsigned hchs = (unsigned)(p.nkb * 2048);                                   // state bytes of a chain
    const unsigned cnts = (unsigned)p.T * kPersist16CntWords;                          // counter words of a chain
    const unsigned orows = (unsigned)(XB * p.Hs), xrows = (unsigned)(XB * p.Np);      // elements of a tile inside a step's block
#define TOK(J) ((J) < nt)
#define TJ(J) ((unsigned)min((J), nt - 1))

    // ---- cell role: thread -> (clip cj, units u0, u0 + 1 of the wave's group)
    const int e4 = lane & 3, kg = (lane >> 2) & 1, cj = 8 * kh + (lane >> 3);
    const int u0 = 8 * kg + 2 * e4;
    const int cunit = w16 * XU + u0;
    float bh[NG][2];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        bh[g][0] = half_ok ? p.bhh[d][g * p.H + cunit] : 0.f;
        bh[g][1] = half_ok ? p.bhh[d][g * p.H + cunit + 1] : 0.f;
    }
    const int nb_last = p.B - (tile0 + nt - 1) * XB;                                   // clips of the window's last real tile (may exceed 16)
    unsigned actbits = 0;                                                              // bit j: this thread's (units, clip) exist in tile j
    int mylen[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const bool a = half_ok && j < nt && (j < nt - 1 || cj < nb_last);
        actbits |= (unsigned)a << j;
        mylen[j] = a ? p.lens[(tile0 + j) * XB + cj] : 0;
    }
    constexpr unsigned OOR = 0x80000000u;
    const unsigned o_by = (unsigned)(cj * p.Hs + (half_ok ? cunit : 0)) * 4u;          // byte offset inside an out row block [16 clips][Hs]
    // publish: lane e4 == 0 of a (clip, k-group) stores the hi plane's 16 bytes, lane e4 == 1 the lo plane's (+ 1024)
    const unsigned pub_off = (e4 < 2 && half_ok) ? (unsigned)(w16 >> 1) * 2048u + (unsigned)(2 * (w16 & 1) + kg) * 256u + (unsigned)cj * 16u + (unsigned)e4 * 1024u : OOR;
    const unsigned pub_sel = e4 == 1 ? 0x07060302u : 0x05040100u;                     // v_perm selector: the high (lo plane) or low (hi plane) halves
    const unsigned shard = (unsigned)(w32 & (kPersist16Shards - 1)) * 64u;
    const unsigned need = (unsigned)((nwg32 + kPersist16Shards - 1 - (lane & (kPersist16Shards - 1))) / kPersist16Shards);
    // reduce buffers: where this lane's MFMA results go (clip ln, units 4 lg ..), where this thread's cell reads from
    float* red_w = red_all + ((mh * 2 + kh) * NG) * RED_G + ln * 16 + 4 * (lg ^ ((ln >> 2) & 3));
    const float* red_r = red_all + ((mh * 2) * NG) * RED_G + cj * 16 + 4 * ((u0 >> 2) ^ ((cj >> 2) & 3)) + (u0 & 3);
    const float* xg_r = xgl + (mh * NG) * 256 + cj * 16 + u0;
    // x-projection requests of this wave: instruction k brings (group xm, gate xg_) = j / NG, j % NG of j = min(v + 4 k, 2 NG - 1):
    // lane l -> clip l >> 2, units 4 (l & 3) .. + 3
    unsigned xq_lds[XJ], xq_col[XJ];
#pragma unroll
    for (int k = 0; k < XJ; ++k) {
        const int j = min(v + 4 * k, 2 * NG - 1), xm = j / NG, xgate = j % NG;
        xq_lds[k] = (unsigned)(size_t)xgl + (unsigned)((xm * NG + xgate) * 1024);
        xq_col[k] = (unsigned)((d * p.nwg16 + min(2 * w32 + xm, p.nwg16 - 1)) * GU + xgate * XU) * 4u;
    }
    const unsigned xl_by = ((unsigned)(lane >> 2) * p.Np + 4u * (lane & 3)) * 4u;
    const unsigned xl_by_last = ((unsigned)min(lane >> 2, nb_last - 1) * p.Np + 4u * (lane & 3)) * 4u;
    // state DMA: this wave brings k-blocks dk0 .. dk0 + NKD - 1 of the item (clamped into the chain: what lies beyond the wave's
    // share is brought twice, to the same place)
    const int dk0 = (v * p.nkb) / 4;

    float hprev[NT][2], cprev[NT][2];
#pragma unroll
    for (int j = 0; j < NT; ++j) { hprev[j][0] = hprev[j][1] = 0.f; cprev[j][0] = cprev[j][1] = 0.f; }

    unsigned long long tm0 = 0, tm1 = 0, tc0 = 0;
#define XT_BEGIN() do { if (STAMP) { __builtin_amdgcn_sched_barrier(0); tm0 = __builtin_amdgcn_s_memrealtime(); tc0 = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } } while (0)
#define XT_CLOCK() do { if (STAMP) { __builtin_amdgcn_sched_barrier(0); if ((threadIdx.x & 63) == 0) tacc[4] += __builtin_amdgcn_s_memtime() - tc0; __builtin_amdgcn_sched_barrier(0); } } while (0)
#define XT_MARK(k) do { if (STAMP) { __builtin_amdgcn_sched_barrier(0); tm1 = __builtin_amdgcn_s_memrealtime(); if ((threadIdx.x & 63) == 0) tacc[k] += tm1 - tm0; tm0 = tm1; __builtin_amdgcn_sched_barrier(0); } } while (0)

    const size_t xstride = (size_t)p.B * p.Np;
    const unsigned ostride_by = (unsigned)((size_t)p.B * p.Hs * 4);

    // x-projection of item (time index tt, tile jt): this wave's XJ requests, into landing zone `zone`
    auto xg_request = [&](int tt, unsigned jt, bool last_tile, unsigned zone) {
        const float* xrow = uni_ptr(p.xp + (size_t)tt * xstride + (size_t)((unsigned)tile0 + jt) * xrows);
        const unsigned by = last_tile ? xl_by_last : xl_by;
#pragma unroll
        for (int k = 0; k < XJ; ++k) {
            const unsigned ldst = __builtin_amdgcn_readfirstlane(xq_lds[k] + zone * (unsigned)XGB), vo = by + xq_col[k];
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(ldst), "v"(vo), "s"(xrow) : "memory");
        }
    };
    unsigned xz = 0;                // landing zone of the phase's MFMA item q: q % 3 (its cell reads it in the next phase)

    // One phase.  J: tile of the MFMA item (s, J).  DO_M: multiply (false: step 0, whose state is zero, and the epilogue).  DO_C: the cell
    // of the previous item, (s, J - 1) or (s - 1, NT - 1).  DUTY: signal / poll / requests for the neighbouring items.
    auto phase = [&](auto jc, auto domc, auto docc, auto dutyc, int s) {
        constexpr int J = decltype(jc)::value;
        constexpr bool DO_M = decltype(domc)::value, DO_C = decltype(docc)::value, DUTY = decltype(dutyc)::value;
        constexpr int JP = (J + NT - 1) % NT, JN = (J + 1) % NT, JQ = (J + 2) % NT, JS = (J + NT - 2) % NT;
        const bool more = s + 1 < p.T;
        const int t = d == 0 ? s : p.T - 1 - s;
        const unsigned parw = (unsigned)(s & 1) * hp_par;            // parity offset step s's cells write h_s at
        const unsigned parr = hp_par - parw;                          // ... and its MFMAs read h_(s-1) from
        const unsigned xz_c = xz == 0 ? 2u : xz - 1u;                 // zone of the cell's item q - 1
        const unsigned xz_n = xz == 2 ? 0u : xz + 1u;                 // zone of item q + 1, requested at the end of this phase
        // item q + 2 = (s, J + 2) needs its chain's step s - 1 [s >= 1]; or (s + 1, J + 2 - NT): its chain's step s [more]
        const bool pon = DUTY && (J + 2 < NT ? s >= 1 : more) && TOK(JQ) && v == 0;
        const int psp = J + 2 < NT ? s - 1 : s;
        const unsigned* pollp = p.cnt + ((unsigned)(chain0 + JQ) * cnts + (unsigned)psp * kPersist16CntWords + (lane & (kPersist16Shards - 1)) * 64);
        // Polls land in LDS (LDS-DMA, 4 bytes per lane: shard l -> sync[8 + l]): no vector-memory load in this loop is visible to the
        // compiler, so it places no vmcnt wait of its own -- any such wait is vmcnt(0) and would also wait for the x-projection
        // requests that are meant to stay in flight (a load into a register by assembly is no way out: the compiler may copy the
        // register before the data has arrived)
        const unsigned poll_lds = (unsigned)(size_t)(sync + 8);
        auto poll_request = [&]() {
            if (lane < kPersist16Shards) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off sc1" :: "s"(poll_lds), "v"(pollp) : "memory");
        };
        XT_BEGIN();
        if (DUTY) {
            // item q - 2, whose stores every wave drained before the barrier that opened this phase: (s, J - 2), or (s - 1, J + NT - 2)
            const int ss = J >= 2 ? s : s - 1;
            if (v == 0 && ss >= 0 && TOK(JS)) {
                const bool drop = d == 0 && tile0 + JS == 0 && w32 == p.drop_wg && ss == p.drop_step;
                if (lane == 0 && !drop)
                    __hip_atomic_fetch_add(p.cnt + ((unsigned)(chain0 + JS) * cnts + (unsigned)ss * kPersist16CntWords + shard), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // the poll's first read, answered at the end of the phase.  With four tiles the signals it asks for go out at the start of
            // this very phase: the read goes out in the middle of the MFMA stream instead (below)
            if (pon && NT > 4) poll_request();
        }
        __builtin_amdgcn_sched_barrier(0);
        // ================= the body: one basic block
        // ---- the cell's operands: K-split partial sums of both halves, x-projection, all gates; two adjacent units of one clip
        f32x2 rv[NG][2], xg[NG];
        if (DO_C) {
            const float* xgz = xg_r + xz_c * (unsigned)(XGB / 4);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                rv[g][0] = *reinterpret_cast<const f32x2*>(red_r + (JP & 1) * RED_BUF + g * RED_G);
                rv[g][1] = *reinterpret_cast<const f32x2*>(red_r + (JP & 1) * RED_BUF + (NG + g) * RED_G);
                xg[g] = *reinterpret_cast<const f32x2*>(xgz + g * 256);
            }
        }
        // ---- MFMAs of item (s, J), B operands from ring slot J & 1; between them the state requests of item q + 1 and the cell
        f32x4 acc[NG], acl[NG];        // hi.hi ; (hi.lo + lo.hi) * 2^11
#pragma unroll
        for (int g = 0; g < NG; ++g) { acc[g] = f32x4{0.f, 0.f, 0.f, 0.f}; acl[g] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        const unsigned char* sb = sbr + (J & 1) * sbytes;
        // B operands: read TWO k-blocks ahead of their MFMAs (one block ahead = 9 MFMAs = 144 cycles, about the latency of a
        // 16-byte LDS read beside the DMA's writes: the matrix pipe then waits for its operands in every block)
        f16x8 bq[3][2];
        auto b_off = [&](int i) { return i < NKW - 1 ? i * 2048 : klast_off; };
        if (DO_M) {
#pragma unroll
            for (int i = 0; i < 2 && i < NKW; ++i) {
                bq[i][0] = *reinterpret_cast<const f16x8*>(sb + b_off(i));
                bq[i][1] = *reinterpret_cast<const f16x8*>(sb + b_off(i) + 1024);
            }
        }
        // item q + 1 = (s, J + 1) reads h_(s-1), or (s + 1, 0) reads h_s; (past the layer's end: a request nobody reads)
        constexpr bool DMA_ON = DUTY && (DO_M || J == NT - 1) && !(SKIP & 1);
        const unsigned dpar = J + 1 < NT ? parr : parw;
        const unsigned char* dsrc = reinterpret_cast<const unsigned char*>(p.hpack) + (dpar + ((unsigned)chain0 + TJ(JN)) * hchs);
        const unsigned dlds = lds_sbuf + (unsigned)((JN & 1) * sbytes);
        const unsigned l16 = lane16;           // (local copies: an asm operand inside a generic lambda does not capture by itself)
        const int dk0_ = dk0, nkb_ = p.nkb;
        // State requests: k-blocks dk0 + i of the item, i < NKD, two 1-KiB planes each, in pairs of blocks on ONE base (the
        // instruction offset applies to the global AND the LDS address: M0 and the scalar address serve four pieces).  Half h of
        // pair G = block 2 G + h; the second half reuses the M0 its first half set (nothing else in this kernel writes M0: checked
        // in the build's assembly, danspeech_amd/csrc/Makefile).
        auto dma_half = [&](int G, int h) {
            if (!DMA_ON || 2 * G + h >= NKD) return;
            const bool two = 2 * G + 1 < NKD;
            const unsigned kb = (unsigned)max(min(dk0_ + 2 * G, nkb_ - (two ? 2 : 1)), 0) * 2048u;
            const unsigned char* src = uni_ptr(dsrc + kb);
            if (h == 0)
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 sc1\n\tglobal_load_lds_dwordx4 %1, %2 offset:1024 sc1"
                             :: "s"(__builtin_amdgcn_readfirstlane(dlds + kb)), "v"(l16), "s"(src) : "memory");
            else
                asm volatile("global_load_lds_dwordx4 %0, %1 offset:2048 sc1\n\tglobal_load_lds_dwordx4 %0, %1 offset:3072 sc1"
                             :: "v"(l16), "s"(src) : "memory");
        };
        // the cell, cut into pieces that are placed between the k-blocks' MFMAs
        f32x2 hg[NG];
        float hn[2] = {0.f, 0.f};
        unsigned pk[2] = {0u, 0u};
        u32x4 pub = {0u, 0u, 0u, 0u};
        constexpr int CT = DO_C ? (J >= 1 ? 0 : 1) : 0;     // the cell's item lies a step back when J == 0
        const int tc = CT ? (d == 0 ? t - 1 : t + 1) : t;
        const unsigned osoff_c = (unsigned)tc * ostride_by;
        const unsigned parw_c = CT ? parr : parw;
        const bool act = (actbits >> JP) & 1u;
        auto cell_piece = [&](int piece) {
            if (!DO_C || (SKIP & 32)) return;
            if (piece == 0) {
#pragma unroll
                for (int g = 0; g < NG; ++g) { hg[g][0] = rv[g][0][0] + rv[g][1][0] + bh[g][0]; hg[g][1] = rv[g][0][1] + rv[g][1][1] + bh[g][1]; }
            } else if (piece == 1 || piece == 2) {
                const int u = piece - 1;
                float xgu[NG], hgu[NG];
#pragma unroll
                for (int g = 0; g < NG; ++g) { xgu[g] = xg[g][u]; hgu[g] = hg[g][u]; }
                float c = cprev[JP][u];
                float h = rnn_cell<KIND, true>(xgu, hgu, hprev[JP][u], c, tc < mylen[JP]);
                h = act ? h : 0.f;
                hn[u] = h; hprev[JP][u] = h;
                if (KIND == DSMI_RNN_LSTM) cprev[JP][u] = c;
                const _Float16 h1 = (_Float16)h;
                const _Float16 h2 = (_Float16)((h - (float)h1) * kLoScale);
                pk[u] = (unsigned)__builtin_bit_cast(unsigned short, h1) | ((unsigned)__builtin_bit_cast(unsigned short, h2) << 16);
            } else if (piece == 3) {
                // every lane of a quad (one clip, one 8-unit k-group) gets the quad's eight words: quad_perm [k, k, k, k] = 0x55 k
                unsigned u[8];
                u[0] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pk[0], 0x00, 0xF, 0xF, false);
                u[1] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pk[1], 0x00, 0xF, 0xF, false);
                u[2] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pk[0], 0x55, 0xF, 0xF, false);
                u[3] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pk[1], 0x55, 0xF, 0xF, false);
                u[4] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pk[0], 0xAA, 0xF, 0xF, false);
                u[5] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pk[1], 0xAA, 0xF, 0xF, false);
                u[6] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pk[0], 0xFF, 0xF, 0xF, false);
                u[7] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)pk[1], 0xFF, 0xF, 0xF, false);
#pragma unroll
                for (int m = 0; m < 4; ++m) pub[m] = __builtin_amdgcn_perm(u[2 * m + 1], u[2 * m], pub_sel);      // units 2m, 2m + 1 of this lane's plane
            } else if (piece == 4 && !(SKIP & 16)) {
                const unsigned hoff = parw_c + ((unsigned)chain0 + TJ(JP)) * hchs;
                __builtin_amdgcn_raw_buffer_store_b128(pub, hrs, TOK(JP) ? pub_off : OOR, hoff, 16);
                u32x2 ov = {__builtin_bit_cast(unsigned, hn[0]), __builtin_bit_cast(unsigned, hn[1])};
                __builtin_amdgcn_raw_buffer_store_b64(ov, ors, act ? o_by : OOR, osoff_c + ((unsigned)tile0 + TJ(JP)) * orows * 4u, 0);
            }
        };
        // ---- the x-projection of item q + 1 = (s, J + 1) or (s + 1, 0): the phase's LAST requests (they stay in flight), placed in
        // front of the last k-block's MFMAs rather than behind the partial tiles (where the matrix pipe would stand meanwhile)
        auto xg_next = [&]() {
            if (DUTY && !(SKIP & 8)) {
                const int tn = J + 1 < NT ? t : (more ? (d == 0 ? t + 1 : t - 1) : t);
                xg_request(tn, TJ(JN), JN >= nt - 1, xz_n);
            }
        };
        // ---- ONE drain per phase, then the x-projection requests of item q + 1.  Vector-memory LOADS (state requests, polls,
        // x-projection: all LDS-DMA) complete in issue order, stores and atomics among themselves, but not against loads: a counted
        // wait that is to leave the x-projection in flight cannot tell an outstanding store from it.  So the phase ends with
        // vmcnt(0) -- publish stores drained (the next phase signals them), state requests landed, poll back -- and the requests for
        // item q + 1's x-projection go out BEHIND it: they are the only operations in flight across the barrier and have the whole
        // next phase to arrive from HBM.  (In front of the partial tiles: the wait lies under the last k-block's MFMAs.)
        auto drain_then_xg = [&]() {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            xg_next();
        };
        constexpr int NP = 5;
        if (!DO_M) {
            if (DUTY && NT == 4 && pon) poll_request();
#pragma unroll
            for (int i = 0; i < NKD; ++i) dma_half(i >> 1, i & 1);
#pragma unroll
            for (int k = 0; k < NP; ++k) cell_piece(k);
            drain_then_xg();
        } else {
#pragma unroll
            for (int i = 0; i < NKW; ++i) {
                if (i + 2 < NKW) {
                    bq[(i + 2) % 3][0] = *reinterpret_cast<const f16x8*>(sb + b_off(i + 2));
                    bq[(i + 2) % 3][1] = *reinterpret_cast<const f16x8*>(sb + b_off(i + 2) + 1024);
                }
                // (pinned: left to itself the scheduler sinks every read to its first use, to save registers it does not lack)
                __builtin_amdgcn_sched_barrier(0);
                const f16x8 b0 = bq[i % 3][0], b1 = bq[i % 3][1];
                dma_half(i >> 1, i & 1);          // block i of the wave's share behind k-block i's operand reads
                // (not in front of the state requests' last block: a request pair's second block reuses the M0 of its first, the
                // poll writes M0;  SKIP >> 8: timing experiments)
                constexpr int POLL_I = (SKIP >> 8) ? (SKIP >> 8) : ((NKW * 9) / 16 > NKD - 1 ? (NKW * 9) / 16 : NKD - 1);
                if (DUTY && NT == 4 && i == POLL_I && pon) poll_request();
                if (i == NKW - 1) {
#pragma unroll
                    for (int k = NKW; k < NKD; ++k) dma_half(k >> 1, k & 1);
                }
                if (!(SKIP & 2)) {
#pragma unroll
                    for (int g = 0; g < NG; ++g) acl[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[i][g][1], b0, acl[g], 0, 0, 0);
#pragma unroll
                    for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[i][g][0], b0, acc[g], 0, 0, 0);
#pragma unroll
                    for (int g = 0; g < NG; ++g) acl[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wv[i][g][0], b1, acl[g], 0, 0, 0);
                }
                // the cell's pieces spread over the k-blocks (NKW >= NP: one piece per block from the first; fewer blocks: the rest behind the last)
                if (i < NP) cell_piece(i);
                if (i == NKW - 1) {
#pragma unroll
                    for (int k = NKW; k < NP; ++k) cell_piece(k);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            drain_then_xg();
            // partial tiles -> reduce buffer J & 1
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = acc[g][r] + acl[g][r] * kLoInv;
                *reinterpret_cast<f32x4*>(red_w + (J & 1) * RED_BUF + g * RED_G) = o;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ================= end of the body
        XT_CLOCK();           // [4]: shader-clock cycles of the body (with [0], its 100 MHz ticks: the clock the body ran at)
        XT_MARK(0);
        XT_MARK(1);
        if (pon && !sync[0] && !(SKIP & 4)) {
            // (LDS reads by assembly: a volatile read through a generic pointer becomes a flat load -- and a vmcnt(0) wait)
            auto lds_word = [&](unsigned addr) { unsigned r; asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(addr) : "memory"); return r; };
            const unsigned pl = poll_lds + (unsigned)(lane & (kPersist16Shards - 1)) * 4u;
            unsigned spins = 0;
            unsigned got = lane < kPersist16Shards ? lds_word(pl) : need;
            if (STAMP && lane == 0 && __builtin_amdgcn_ballot_w64(got < need) != 0) tacc[5] += 1;      // polls whose first read was too early
            while (__builtin_amdgcn_ballot_w64(got < need) != 0) {
                __builtin_amdgcn_s_sleep(1);
                ++spins;
                if (STAMP && lane == 0) tacc[6] += 1;
                if (spins > p.spin_limit) { __hip_atomic_store(p.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); sync[0] = 1; break; }
                if ((spins & 1023u) == 0) {           // somebody else gave up: stop waiting too
                    if (lane == 0) asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, off sc1" :: "s"(poll_lds + 32u), "v"(p.err) : "memory");
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    if (lds_word(poll_lds + 32u) != 0) { sync[0] = 1; break; }
                }
                poll_request();
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                got = lane < kPersist16Shards ? lds_word(pl) : need;
            }
        }
        XT_MARK(2);
        ring4_barrier();
        XT_MARK(3);
        if (STAMP && lane == 0) tacc[7] += 1;
        xz = xz_n;
    };

    // item 0's x-projection into zone 0; then: the prologue's loads (W_hh, biases, lengths) and that request have arrived, the zeroed
    // LDS is visible (the zeroing stores are ordered before the DMA's landing by the barrier in between)
    __builtin_amdgcn_s_waitcnt(0x0F70);
    ring4_barrier();
    if (!(SKIP & 8)) xg_request(d == 0 ? 0 : p.T - 1, 0u, nt <= 1, 0u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ring4_barrier();

    using std::integral_constant;
    constexpr std::true_type Y; constexpr std::false_type N;
    auto for_tiles = [&](auto f) {
        f(integral_constant<int, 0>{}); f(integral_constant<int, 1>{}); f(integral_constant<int, 2>{}); f(integral_constant<int, 3>{});
        if constexpr (NT > 4) { f(integral_constant<int, 4>{}); f(integral_constant<int, 5>{}); }
        if constexpr (NT > 6) { f(integral_constant<int, 6>{}); f(integral_constant<int, 7>{}); }
    };
    // step 0: h = 0 -- no state, no MFMAs; the cells of its items read the zeroed reduce buffers
    for_tiles([&](auto jc) {
        constexpr int J = decltype(jc)::value;
        if constexpr (J == 0) phase(jc, N, N, Y, 0); else phase(jc, N, Y, Y, 0);
    });
    for (int s = 1; s < p.T; ++s) {
        // W_hh's first NKA k-blocks live in AccVGPRs: the MFMAs take them from there
#pragma unroll
        for (int i = 0; i < NKA; ++i)
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) asm volatile("" : "+a"(wv[i][g][pl]));
        for_tiles([&](auto jc) { phase(jc, Y, Y, Y, s); });
    }
    // the cell of the last item, (T - 1, NT - 1)
    phase(integral_constant<int, 0>{}, N, Y, N, p.T);
#undef TOK
#undef TJ
#undef XT_BEGIN
#undef XT_MARK
#undef XT_CLOCK
    if (STAMP && lane == 0) {
        unsigned long long* o = p.dbg + ((size_t)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4 + v) * 8;
        for (int k = 0; k < 8; ++k) o[k] = tacc[k];
    }
}

// (dynamic LDS of a workgroup: ring4_lds_bytes, rnn_plan.h -- the same formula rnn_persist_ring4_tiles holds against the CU's LDS)
template <int KIND, int NT>
bool launch_ring4_nt(const Ring4Args& a, hipStream_t s, const EvPair& ev) {
    const int nkw = rnn_persist_ring4_form(KIND, a.nkb, a.ntw, a.dbg != nullptr);
    const size_t lds = ring4_lds_bytes(KIND, a.nkb);
    const dim3 grid((a.nwg16 + 1) / 2, a.D, ceil_div(a.tile_end - a.tile0, a.ntw)), block(XNT);
#define CASE(N, ...) case N: launch_lds(rnn_persist_ring4_kernel<KIND, N, NT, __VA_ARGS__>, grid, block, lds, s, ev, a); return true;
    if (a.dbg) {
        if constexpr (KIND == DSMI_RNN_GRU) switch (nkw) { CASE(13, true) }
        return false;
    }
#ifdef DSMI_EXPERIMENTS
    static const int skip = exp_env("DSMI_DEBUG_RING_SKIP") ? std::atoi(exp_env("DSMI_DEBUG_RING_SKIP")) : 0;
    if (skip) {           // timing experiments: cfgA's shape only, a fixed list of masks
        if constexpr (KIND == DSMI_RNN_GRU && NT == 4) {
            if (nkw != 13) return false;
#define SKIP_CASE(M) case M: launch_lds(rnn_persist_ring4_kernel<KIND, 13, NT, false, M>, grid, block, lds, s, ev, a); return true;
            switch (skip) {
                SKIP_CASE(1) SKIP_CASE(2) SKIP_CASE(4) SKIP_CASE(8) SKIP_CASE(16) SKIP_CASE(32) SKIP_CASE(9) SKIP_CASE(13) SKIP_CASE(29) SKIP_CASE(31) SKIP_CASE(61) SKIP_CASE(63)
                SKIP_CASE(0x600) SKIP_CASE(0x700) SKIP_CASE(0x900) SKIP_CASE(0xA00) SKIP_CASE(0xB00)          // the complete kernel with the poll's first read at k-block 6 .. 11
            }
#undef SKIP_CASE
        }
        return false;
    }
#endif
    switch (nkw) { CASE(1, false) CASE(2, false) CASE(3, false) CASE(4, false) CASE(5, false) CASE(6, false) CASE(7, false) CASE(8, false) }
    if constexpr (KIND != DSMI_RNN_LSTM) switch (nkw) { CASE(9, false) CASE(10, false) CASE(11, false) CASE(12, false) CASE(13, false) }
    if constexpr (KIND != DSMI_RNN_LSTM && NT <= 4) switch (nkw) { CASE(14, false) }      // (the eight-tile schedule: see rnn_persist_ring4_form)
#undef CASE
    return false;
}

}  // namespace

bool launch_rnn_persist_ring4(const RnnPersist16Launch& p, hipStream_t s) {
    Ring4Args a;
    fill_shared(a, p);
    a.nwg16 = p.g.nwg; a.tickets = p.tickets;
    a.tile0 = p.tile0; a.ntw = p.ntw > 0 ? p.ntw : a.ntiles - p.tile0;
    a.tile_end = std::min(a.ntiles, a.tile0 + a.ntw * std::max(p.nwin, 1));
    if (a.ntw < 1 || a.ntw > XMAXT || a.tile_end <= a.tile0 || !rnn_ring_rows_fit(p.g, p.B, p.T)) return false;
    if (a.ntw > 4) {          // more than four tiles per window: the eight-tile schedule (six: two phantom tiles); measured, no gain
#ifndef DSMI_EXPERIMENTS
        return false;         // (DSMI_RING_TILES=6|8 exists in the experiments build only: rnn_persist_ring4_tiles never says more than four)
#else
        return by_kind(p.g.kind, [&](auto k) { return launch_ring4_nt<decltype(k)::value, 8>(a, s, p.ev); });
#endif
    }
    return by_kind(p.g.kind, [&](auto k) { return launch_ring4_nt<decltype(k)::value, 4>(a, s, p.ev); });
}

}  // namespace dsmi
