// The resumable beam search (beam_kernel<..., RESUME = true> of danspeech_amd/csrc/beam_kernel.inc) on the CPU SIMT emulation
// of simt.h, beside the whole-utterance kernel it must reproduce.  Reads one utterance and a list of chunk sizes from a binary
// file written by tools/emu/run_beam_stream_emu.py, carries the search through the chunks one launch each, and after every
// chunk writes the carried search's hypotheses and those of the whole-utterance kernel over the same prefix.  The two launches
// share the emulated LDS, so the resumed one cannot lean on anything a previous launch left there.  A test tool, not a CPU path.
//   g++ -DSIMT_EMU -O1 -g -std=c++20 -pthread -I danspeech_amd/csrc -I tools/emu tools/emu/beam_stream_emu.cpp -o tools/emu/beam_stream_emu
#include "simt.h"
#include <cstdio>
#include <string>
#include <fstream>
#include "lm.h"
#include "lm.cpp.inc"
#include "lm_klm.cpp.inc"
using namespace dsmi;
namespace { alignas(16) unsigned char smem_raw[160 * 1024]; }      // (the kernel declares it inside its anonymous namespace)
#define DSMI_WAIT_STORES() __atomic_thread_fence(__ATOMIC_SEQ_CST)
#include "beam_kernel.inc"

template <bool RESUME>
static int launch(const BeamArgs& a, int grid, int BT, size_t per) {
    if (BT == 1024) {
        if (per <= 3) simt::launch(grid, BT, [&]() { beam_kernel<1024, 3, 0, 0, RESUME>(a); });
        else simt::launch(grid, BT, [&]() { beam_kernel<1024, 6, 0, 0, RESUME>(a); });
    } else {
        if (per > 9) { std::fprintf(stderr, "too many pairs per thread for the 192-thread build\n"); return 4; }
        simt::launch(grid, 192, [&]() { beam_kernel<192, 9, 0, 0, RESUME>(a); });
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: beam_stream_emu problem.bin out.bin [threads]\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    int32_t hd[8];
    f.read((char*)hd, sizeof(hd));
    const int T = hd[1], C = hd[2], beam = hd[3], blank = hd[4], top_n = hd[5], has_lm = hd[6], nlab = hd[7];
    if (hd[0] != 1) { std::fprintf(stderr, "one utterance per problem\n"); return 2; }
    double dd[3];
    f.read((char*)dd, sizeof(dd));                       // cutoff_prob, alpha, beta
    std::vector<float> probs((size_t)T * C);
    f.read((char*)probs.data(), probs.size() * 4);
    std::vector<std::string> labels;
    for (int i = 0; i < nlab; ++i) { int32_t n; f.read((char*)&n, 4); std::string s(n, 0); f.read(&s[0], n); labels.push_back(s); }
    std::string lm_path;
    { int32_t n; f.read((char*)&n, 4); lm_path.resize(n); f.read(&lm_path[0], n); }
    int32_t nchunks = 0;
    f.read((char*)&nchunks, 4);
    std::vector<int32_t> chunks(nchunks);
    f.read((char*)chunks.data(), nchunks * 4);
    const int BT = argc > 3 ? std::atoi(argv[3]) : 1024;
    HostLM lm;
    if (has_lm) { const std::string msg = lm.load(lm_path, labels); if (!msg.empty()) { std::fprintf(stderr, "%s\n", msg.c_str()); return 3; } }
    int space = -2;
    for (int i = 0; i < nlab; ++i) if (labels[i] == " ") space = i;
    if (carve(beam, C, BT).bytes > sizeof(smem_raw)) { std::fprintf(stderr, "does not fit\n"); return 4; }
    const int EW = (beam + 63) / 64, RW = has_lm ? 2 * EW : EW;
    if (BT <= 64 * RW) { std::fprintf(stderr, "too few threads for this beam\n"); return 4; }
    const size_t per = ((size_t)beam * C + (BT - 64 * RW) - 1) / (BT - 64 * RW);

    BeamArgs base{};
    base.C = C; base.blank = blank; base.space = space; base.beam = beam;
    base.cutoff_top_n = top_n; base.cutoff_prob = (float)dd[0]; base.has_lm = has_lm; base.order = has_lm ? lm.order : 1; base.alpha = dd[1]; base.beta = dd[2];
    base.lm = lm.view(); base.trie_next = lm.trie_next.data(); base.trie_word = lm.trie_word.data(); base.unk = lm.unk; base.bos = lm.bos;

    const int Tw = T > 0 ? T : 1;                          // output stride: the whole utterance
    std::vector<unsigned char> state(stream_state(beam, C).bytes);
    std::vector<NodeRec> snodes((size_t)2 + (size_t)T * beam);
    std::ofstream o(argv[2], std::ios::binary);
    int t0 = 0;
    for (int k = 0; k < nchunks; ++k) {
        const int Tc = chunks[k];
        if (Tc < 0 || t0 + Tc > T) { std::fprintf(stderr, "bad chunk list\n"); return 2; }
        // the carried search, advanced by this chunk
        std::vector<int32_t> tok((size_t)beam * Tw), step((size_t)beam * Tw), len(beam), nout(1);
        std::vector<double> score(beam);
        BeamStreamDesc d{};
        d.probs = probs.data() + (size_t)t0 * C; d.state = state.data(); d.nodes = snodes.data();
        d.out_tok = tok.data(); d.out_step = step.data(); d.out_len = len.data(); d.out_n = nout.data(); d.out_score = score.data();
        d.T = Tc; d.t0 = t0; d.n_best = beam; d.out_T = Tw;
        BeamArgs a = base;
        a.desc = &d;
        if (int rc = launch<true>(a, 1, BT, per)) return rc;
        o.write((char*)tok.data(), tok.size() * 4); o.write((char*)step.data(), step.size() * 4); o.write((char*)len.data(), len.size() * 4);
        o.write((char*)nout.data(), 4); o.write((char*)score.data(), score.size() * 8);
        t0 += Tc;
        // the whole-utterance kernel over frames 0 .. t0
        std::vector<int32_t> wtok((size_t)beam * Tw), wstep((size_t)beam * Tw), wlen(beam), wn(1), sizes{t0};
        std::vector<double> wscore(beam);
        std::vector<NodeRec> wnodes((size_t)2 + (size_t)Tw * beam);
        BeamArgs w = base;
        w.probs = probs.data(); w.sizes = sizes.data(); w.T = Tw; w.ncap = 2 + Tw * beam; w.nodes = wnodes.data();
        w.out_tok = wtok.data(); w.out_step = wstep.data(); w.out_len = wlen.data(); w.out_n = wn.data(); w.out_score = wscore.data();
        if (int rc = launch<false>(w, 1, BT, per)) return rc;
        o.write((char*)wtok.data(), wtok.size() * 4); o.write((char*)wstep.data(), wstep.size() * 4); o.write((char*)wlen.data(), wlen.size() * 4);
        o.write((char*)wn.data(), 4); o.write((char*)wscore.data(), wscore.size() * 8);
    }
    std::fprintf(stderr, "emulated %d chunks of %d frames on %d threads\n", nchunks, T, BT);
    return 0;
}
