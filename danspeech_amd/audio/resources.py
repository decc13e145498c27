"""Audio file loading for the drop-in surface (reference danspeech/audio/resources.py:22-82).

Only what ``recognize()`` needs: ``load_audio`` for PCM WAV files with the reference's semantics
(4096-frame chunks, optional duration/offset, stereo -> mono as the *saturating sum* L+R of
``audioop.tomono(buf, width, 1, 1)`` at resources.py:302-303, samples returned as float64 at
their integer scale, resources.py:630-640) and ``load_audio_wavPCM`` (channel *mean*).
AIFF/FLAC decoding, the microphone classes and ``AudioData`` are outside the hot path.
"""
import wave

import numpy as np


def _frames_to_int(buf, width):
    if width == 1:      # unsigned 8-bit; AudioData.get_raw_data biases by -128 (resources.py:551-554)
        return np.frombuffer(buf, dtype=np.uint8).astype(np.int64) - 128
    if width == 2:
        return np.frombuffer(buf, dtype="<i2").astype(np.int64)
    if width == 4:
        return np.frombuffer(buf, dtype="<i4").astype(np.int64)
    if width == 3:
        a = np.frombuffer(buf, dtype=np.uint8).reshape(-1, 3).astype(np.int64)
        v = a[:, 0] | (a[:, 1] << 8) | (a[:, 2] << 16)
        return np.where(v >= 1 << 23, v - (1 << 24), v)
    raise ValueError("unsupported sample width %d" % width)


def read_wav_frames(path, duration=None, offset=None):
    """The byte stream ``load_audio`` decodes, undecoded: (raw frames, sample width, channels).

    Same chunked reading as resources.py:41-57 (4096-frame chunks, optional duration/offset at
    the pinned 16 kHz).  The bytes can go to the GPU as they are: ``dsmi_features`` decodes the
    sample width and folds two channels (``Recognizer.recognize_files``)."""
    try:
        reader = wave.open(path, "rb")
    except (wave.Error, EOFError):
        raise ValueError("Audio file could not be read as PCM WAV; AIFF/FLAC decoding is outside this package's scope")
    with reader:
        nch, width = reader.getnchannels(), reader.getsampwidth()
        assert 1 <= nch <= 2, "Audio must be mono or stereo"
        chunk = 4096
        seconds_per_buffer = (chunk + 0.0) / 16000      # SpeechFile pins sampling_rate = 16000 (resources.py:192)
        elapsed_time = 0
        offset_time = 0
        offset_reached = False
        parts = []
        while True:                                      # resources.py:41-57
            if offset and not offset_reached:
                offset_time += seconds_per_buffer
                if offset_time > offset:
                    offset_reached = True
            buf = reader.readframes(chunk)
            if len(buf) == 0:
                break
            if offset_reached or not offset:
                elapsed_time += seconds_per_buffer
                if duration and elapsed_time > duration:
                    break
                parts.append(buf)
    if nch == 2 and width == 1:
        raise ValueError("8-bit stereo WAV is not supported")
    return b"".join(parts), width, nch


def read_wav_frames_rate(path, duration=None, offset=None):
    """(raw frames, sample width, channels, frame rate) of a PCM WAV file: what ``read_wav_frames`` returns together with the
    rate the file's header states, for callers that resample (``Recognizer.recognize_files(..., resample=...)``).  ``offset``
    and ``duration`` are seconds of the file's OWN rate, cut to whole frames -- not ``read_wav_frames``' 4096-frame chunks
    at the pinned 16 kHz, which are the reference's bookkeeping and stay as they are."""
    try:
        reader = wave.open(path, "rb")
    except (wave.Error, EOFError):
        raise ValueError("Audio file could not be read as PCM WAV; AIFF/FLAC decoding is outside this package's scope")
    with reader:
        nch, width, rate = reader.getnchannels(), reader.getsampwidth(), reader.getframerate()
        assert 1 <= nch <= 2, "Audio must be mono or stereo"
        if nch == 2 and width == 1:
            raise ValueError("8-bit stereo WAV is not supported")
        if offset:
            reader.setpos(min(int(round(offset * rate)), reader.getnframes()))
        left = reader.getnframes() - reader.tell()
        raw = reader.readframes(min(int(round(duration * rate)), left) if duration else left)
    return raw, width, nch, rate


def resample(audio, rate_in, rate_out=16000, method="polyphase", device=0):
    """Samples at ``rate_in`` Hz -> float64 samples at ``rate_out`` Hz, converted on the GPU (``dsmi_resample``).  A numpy array
    (int16 / float32 / float64; anything else is taken as float64) comes back as a numpy array, a 1-D CUDA tensor as a CUDA
    tensor.  ``method``: "polyphase" (Kaiser-windowed sinc, ``scipy.signal.resample_poly``'s default design) or "ratecv"
    (``audioop.ratecv``, what the reference's ``AudioData.get_array_data(convert_rate=...)`` applies; int16 samples only here)."""
    import torch
    from .. import _native
    key = (int(rate_out), int(device) if not torch.is_tensor(audio) else int(audio.device.index))
    if key not in _RESAMPLERS:
        _RESAMPLERS[key] = _native.NativeFrontend(dict(sampling_rate=int(rate_out)), device=key[1])
    if torch.is_tensor(audio):
        out, _ = _RESAMPLERS[key].resample(audio.reshape(-1), [audio.numel()], rate_in, method)
        return out
    a = np.ascontiguousarray(audio).reshape(-1)
    if a.dtype not in (np.dtype(np.int16), np.dtype(np.float32), np.dtype(np.float64)):
        a = a.astype(np.float64)
    out, _ = _RESAMPLERS[key].resample(torch.from_numpy(a).to("cuda:%d" % key[1]), [len(a)], rate_in, method)
    return out.cpu().numpy()


_RESAMPLERS = {}      # (rate_out, device) -> the frontend handle that keeps the filters of `resample`


def load_audio(path, duration=None, offset=None):
    """PCM WAV -> float64 numpy array ready for ``Recognizer.recognize``."""
    raw, width, nch = read_wav_frames(path, duration=duration, offset=offset)
    data = _frames_to_int(raw, width)
    if nch == 2:
        data = data.reshape(-1, 2)
        lim = 1 << (8 * width - 1)
        data = np.clip(data[:, 0] + data[:, 1], -lim, lim - 1)     # audioop.tomono(buf, width, 1, 1) saturates
    return data.astype(float)


def load_audio_wavPCM(path):
    """resources.py:64-82: scipy-style read, multi-channel averaged."""
    import scipy.io.wavfile as wav
    _, sound = wav.read(path)
    if len(sound.shape) > 1:
        if sound.shape[1] == 1:
            sound = sound.squeeze()
        else:
            sound = sound.mean(axis=1)
    return sound.astype(float)
