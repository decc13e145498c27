// The host prelude of the five persistent recurrent kernel files (rnn_persist*.hip): set a kernel's dynamic LDS and launch it, the
// cell type as a template argument, the fields the four 16-unit argument blocks share.  Which instantiation a launcher's switch
// reaches is rnn_plan.h's answer (rnn_*_form): a launcher holds one `case` per instantiation and nothing that picks.
#pragma once
#include <type_traits>

#include "common.h"

namespace dsmi {

// Raise the kernel's dynamic-LDS limit to what this launch asks for, then launch it (ev set: with the dispatch's own timestamps).
template <class Args>
inline void launch_lds(void (*kernel)(Args), dim3 grid, dim3 block, size_t lds, hipStream_t s, const EvPair& ev, const Args& a) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    DSMI_LAUNCH(kernel, grid, block, lds, s, ev, a);
}

// f(std::integral_constant<int, KIND>) for the layer's cell type
template <class F>
inline bool by_kind(int kind, F&& f) {
    switch (kind) {
        case DSMI_RNN_GRU: return f(std::integral_constant<int, DSMI_RNN_GRU>{});
        case DSMI_RNN_LSTM: return f(std::integral_constant<int, DSMI_RNN_LSTM>{});
        default: return f(std::integral_constant<int, DSMI_RNN_TANH>{});
    }
}

// What P16Args, DuoArgs, RingArgs and Ring4Args take from the launch description under the same name and meaning; the window of
// the layer a launch carries, and the workgroup count (nwg / nwg16), are the launcher's own.
template <class Args>
inline void fill_shared(Args& a, const RnnPersist16Launch& p) {
    for (int d = 0; d < 2; ++d) { a.whh[d] = p.whh16[d]; a.bhh[d] = p.bhh[d]; a.out[d] = p.out[d]; }
    a.xp = p.xp; a.lens = p.lens_dev; a.hpack = p.hpack16; a.cnt = p.counters; a.err = p.err;
    a.B = p.B; a.T = p.T; a.H = p.g.H; a.Hs = p.g.Kp; a.Np = p.g.Np; a.nkb = ceil_div(p.g.H, 32);
    a.ntiles = ceil_div(p.B, kTileClips); a.D = p.g.D;
    a.spin_limit = p.spin_limit; a.drop_wg = p.drop_wg; a.drop_step = p.drop_step; a.dbg = p.dbg;
}

}  // namespace dsmi
