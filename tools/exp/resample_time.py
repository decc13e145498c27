"""Sample-rate conversion (dsmi_resample) beside the stages behind it: one batch of B = 32 clips of 10 s as 44.1 kHz stereo
int16 bytes (56 MB), already on the device.

  python tools/exp/resample_time.py [--reps 50] [--warmup 5] [--out DIR]

1. dsmi_resample of the batch to 16 kHz float64 (41 MB), for both methods: device events around the call.
2. dsmi_features of its output (32 clips of 10 s at 16 kHz).
3. The forward of those spectrograms through a synthetic cfgA model (2 conv, 5 x BiGRU 800).
Medians with min / max over --reps.  Prints one JSON line per figure; the bytes each call has to move (input read once,
output written once) are printed with it, so that the rate can be read off."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--rate", type=int, default=44100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    from danspeech_amd import synthetic as syn
    from danspeech_amd.deepspeech.model import DeepSpeech
    from danspeech_amd.audio.parsers import SpectrogramAudioParser
    assert torch.cuda.is_available(), "needs the GPU"
    sd = syn.make_state_dict(2, "gru", 800, 5, seed=0, fc_gain=8.0)
    model = DeepSpeech("cfgA", rnn_type="gru", rnn_hidden_size=800, rnn_layers=5, conv_layers=2).load_state_dict(sd).to("cuda")
    fe = SpectrogramAudioParser()._frontend()
    n = int(a.rate * a.seconds)
    rng = np.random.default_rng(11)
    frames = rng.integers(-12000, 12000, size=(a.batch, n, 2), dtype=np.int16)
    pcm = torch.from_numpy(frames.reshape(-1).view(np.uint8)).cuda()
    n_in = np.full(a.batch, n, dtype=np.int64)
    stream = torch.cuda.current_stream()
    lines = []

    def emit(d):
        print(json.dumps(d), flush=True)
        lines.append(d)

    def timed(fn, reps):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return _spread(ms)

    out = n_out = None
    for method in ("polyphase", "ratecv"):
        out, n_out = fe.resample(pcm, n_in, a.rate, method, wav_format=(2, 2))
        t = timed(lambda: fe.resample(pcm, n_in, a.rate, method, wav_format=(2, 2)), a.reps)
        emit(dict(figure="dsmi_resample", method=method, batch=a.batch, seconds=a.seconds, rate_in=a.rate, pcm="stereo int16",
                  bytes_in=int(pcm.numel()), bytes_out=int(out.numel() * 8), device_events_ms=t))
    out, n_out = fe.resample(pcm, n_in, a.rate, "polyphase", wav_format=(2, 2))
    feats, fr = fe.features(out, n_out)
    emit(dict(figure="dsmi_features", batch=a.batch, samples=int(n_out[0]), pcm="float64", frames=int(fr.max()),
              device_events_ms=timed(lambda: fe.features(out, n_out), a.reps)))
    # the same spectrograms from int16 samples, what a 16 kHz file costs
    out16 = out.round().clamp(-32768, 32767).to(torch.int16)
    emit(dict(figure="dsmi_features", batch=a.batch, samples=int(n_out[0]), pcm="int16", frames=int(fr.max()),
              device_events_ms=timed(lambda: fe.features(out16, n_out), a.reps)))
    lens = torch.from_numpy(fr.astype(np.int32))
    emit(dict(figure="forward", batch=a.batch, model="cfgA 2 conv + 5 x BiGRU 800",
              device_events_ms=timed(lambda: model.forward(feats, lens), max(10, a.reps // 5))))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "resample_time.jsonl"), "w") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
