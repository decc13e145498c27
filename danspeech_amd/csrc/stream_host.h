// The host half of a streaming pass (dsmi_stream_forward, dsmi_stream_forward_many: stream.hip): what one chunk means for one session
// -- the chunk arithmetic of the reference's MaskConvStream (model.py:171-201) and LookaheadStream (:256-283), what is refused, and
// the flags a pass leaves on the handle -- stated once; both entry points call stream_pass_plan and stream_pass_commit and nothing
// else for it.  No HIP: tools/asan/host_fuzz.cpp (streampass) runs it under ASan + UBSan and tests/test_stream_pass_host.py holds it
// to the reference's frame counts.
#pragma once
#include <algorithm>

#include "../../include/dsmi.h"

namespace dsmi {

inline int conv_t1(int tin) { return (tin + 2 * 5 - 11) / 2 + 1; }     // conv1: k_t 11, stride 2, pad 5 (model.py:455)

// Rows LookaheadStream keeps of a chunk of Tc rows: x[-(context-1):] (model.py:263).  With context 1 that slice is x[-0:], the
// WHOLE chunk, which the next pass then yields a second time: the reference's behaviour, kept.
inline int la_keep(int Tc, int ctx) { return ctx == 1 ? Tc : std::min(Tc, ctx - 1); }

// What a session carries between calls on the host: which of the handle's device buffers hold something.
struct StreamFlags {
    bool has_left = false;       // left[]: the last 10 input frames of each conv layer
    bool has_hidden = false;     // hcarry / ccarry / hpack: h (and c) of every layer
    bool la_init = false;        // the lookahead has buffered a chunk, ...
    int la_rows = 0;             // ... la_buf holds this many rows
};

// What one chunk of T >= 1 feature frames means for one session.
struct StreamPass {
    int padl, padr, ctxl;        // per conv layer: zero frames in front of / behind the chunk, glued context frames
    int tin[2], to[2];           // frames into / out of each conv layer; to[1] = Tc, the recurrent steps
    bool buffering;              // the lookahead only stores the chunk: no output
    int ncat, nout, keep;        // buffered + new rows; frames yielded; rows the lookahead keeps of a chunk it emits from
};

// Plans the pass or refuses it: DSMI_OK and *pass, or a DSMI_ERR_* code and the reason in *why (*pass is not written; nothing here
// changes the flags).  have_probs / T_out_cap: the caller's output slot, which only a pass that yields frames needs.
inline int stream_pass_plan(const StreamFlags& f, int T, bool is_first, bool is_last, int context, bool have_probs, int T_out_cap,
                            StreamPass* pass, const char** why) {
    auto refuse = [&](int code, const char* msg) { *why = msg; return code; };
    if (!is_first && !f.has_left)
        return refuse(DSMI_ERR_INVALID, "the first chunk of an utterance must be passed with is_first (MaskConvStream has no left context)");
    StreamPass p;
    // MaskConvStream: is_first pads in front, otherwise is_last pads behind; unless is_first the ten kept frames are glued in front
    p.padl = is_first ? 5 : 0; p.padr = (!is_first && is_last) ? 5 : 0; p.ctxl = is_first ? 0 : 10;
    p.tin[0] = p.ctxl + p.padl + T + p.padr; p.to[0] = conv_t1(p.tin[0]);
    p.tin[1] = p.ctxl + p.padl + p.to[0] + p.padr; p.to[1] = p.tin[1];
    if ((!is_last && (p.tin[0] < 10 || p.tin[1] < 10)) || p.to[0] < 1) return refuse(DSMI_ERR_INVALID, "chunk too short for the conv context");
    // LookaheadStream: the first pass, or is_first, buffers the whole chunk; later passes yield all rows but the last context - 1
    p.buffering = !f.la_init || is_first;
    p.ncat = f.la_rows + p.to[1];
    p.nout = p.buffering ? 0 : (is_last ? p.ncat : p.ncat - (context - 1));
    p.keep = la_keep(p.to[1], context);
    if (!p.buffering && p.nout < 1) return refuse(DSMI_ERR_INVALID, "lookahead: fewer buffered frames than the context (torch raises here too)");
    if (!p.buffering && (!have_probs || T_out_cap < p.nout)) return refuse(DSMI_ERR_CAPACITY, "probs slot smaller than the frames this pass yields");
    *pass = p;
    return DSMI_OK;
}

// What a completed pass leaves behind: the flags, and pbase [L], each layer's parity offset of the packed state.  is_last clears
// the conv context and h / c (model.py:234-236; MaskConvStream simply stops storing) and, in a pass that emits, the lookahead (:279-281).
inline void stream_pass_commit(StreamFlags& f, int* pbase, int L, const StreamPass& p, bool is_last) {
    f.has_left = f.has_hidden = !is_last;
    for (int l = 0; l < L; ++l) pbase[l] = is_last ? 0 : (p.to[1] + pbase[l]) & 1;
    f.la_init = p.buffering || !is_last;
    f.la_rows = p.buffering ? p.to[1] : (is_last ? 0 : p.keep);
}

}  // namespace dsmi
