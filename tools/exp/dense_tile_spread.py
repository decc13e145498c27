#!/usr/bin/env python3
"""Where the XCDs end inside the x-projection GEMMs while the batch pipeline runs (cfgA, four forwards of 64 clips in flight), with
the static tile order (DSMI_DENSE_TILES=0) and with tiles by demand: dsmi_debug_dense_stamps of the experiments build.

    python3 tools/exp/dense_tile_spread.py [steps]        (needs `make -C danspeech_amd/csrc exp`)

Per arm and kernel (layer GEMM, layer-0 GEMM), over the launches of the timed steps: the launch's length (first workgroup's start
to the last one's end), how far the last XCD ends behind the mean XCD and behind the first one (by the XCD a workgroup ran on,
HW_REG_XCC_ID, and by the label blockIdx.x & 7), and the tiles each XCD computed (sorted: the static order gives every label the
same share, by demand an XCD takes what its free CUs can do)."""
import os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

WORDS = 32


def child(steps):
    import numpy as np, torch
    from danspeech_amd import Recognizer, _native, synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    from danspeech_amd.audio.parsers import DeviceClips
    B, N = 32, 160000
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, **syn.TALKATIVE)
    rec = Recognizer(model=DeepSpeech("cfgA", rnn_hidden_size=800, rnn_layers=5).load_state_dict(sd))
    pcm = torch.from_numpy(np.stack([syn.make_clip(i, N) for i in range(B)])).cuda()
    clips = DeviceClips(pcm.view(-1), np.full(B, N, dtype=np.int64))
    eng = rec.danspeech_recognizer
    warm = 16
    for _ in eng.transcribe_batches((clips for _ in range(warm + steps)), lanes=4, merge_clips=64):
        pass
    torch.cuda.synchronize()
    st = np.zeros(4096 * WORDS, dtype=np.uint64)
    n = _native.lib().dsmi_debug_dense_stamps(_native._np_ptr(st), st.size)
    assert n > 0, "no stamps (%d): is DSMI_LIBRARY the experiments build and DSMI_DEBUG_TILE_STAMPS=1?" % n
    st = st[:n * WORDS].reshape(n, WORDS)
    first = n * warm // (warm + steps)          # the launches of the warm-up steps are left out
    print("%d launches stamped, %d of the timed steps" % (n, n - first))
    for kind, name in ((1, "layer GEMM   "), (2, "layer-0 GEMM ")):
        rows = [r for r in st[first:] if int(r[25]) == kind]
        if not rows:
            continue
        dur, behind_mean, last_first, lab_mean, tiles = [], [], [], [], []
        for r in rows:
            start = float(~r[24] & np.uint64(0xFFFFFFFFFFFFFFFF))
            xe = np.array([float(v) for v in r[8:16] if v], dtype=np.float64) - start       # 100 MHz ticks
            le = np.array([float(v) for v in r[0:8] if v], dtype=np.float64) - start
            d = xe.max()
            dur.append(d / 100.0)
            behind_mean.append((xe.max() - xe.mean()) / d)
            last_first.append((xe.max() - xe.min()) / d)
            lab_mean.append((le.max() - le.mean()) / d)
            tiles.append(sorted(int(v) for v in r[16:24]))
        t = np.array(tiles, dtype=np.float64)
        print("%s %3d launches, %d workgroups, by demand %d: length %7.1f us (min %6.1f max %7.1f); last XCD behind the mean XCD %4.1f %% of it "
              "(median %4.1f, max %4.1f), behind the first %4.1f %%; last label behind the mean label %4.1f %%"
              % (name, len(rows), int(rows[0][26]), int(rows[0][27]), np.mean(dur), np.min(dur), np.max(dur), 100 * np.mean(behind_mean),
                 100 * np.median(behind_mean), 100 * np.max(behind_mean), 100 * np.mean(last_first), 100 * np.mean(lab_mean)))
        print("              tiles per XCD, fewest to most, mean over the launches: %s   (one launch: %s)"
              % (" ".join("%.1f" % v for v in t.mean(axis=0)), " ".join(str(v) for v in tiles[len(tiles) // 2])))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "child":
        child(int(sys.argv[2]))
        sys.exit(0)
    from explib import exp_env
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    for arm in ("0", "1"):
        print("=== DSMI_DENSE_TILES=%s" % arm, flush=True)
        env = exp_env(DSMI_DEBUG_TILE_STAMPS=1, DSMI_DENSE_TILES=arm)
        env.setdefault("GPU_MAX_HW_QUEUES", "8")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(steps)], env=env, timeout=280)
        if r.returncode != 0:
            sys.exit("arm %s ended with %d: nothing more is started" % (arm, r.returncode))
