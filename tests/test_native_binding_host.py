"""CPU-side checks of the ctypes binding (danspeech_amd/_native.py) against include/dsmi.h: every constant the binding restates
has the header's value and every descriptor the header's members; the one function that derives a DSMI_PCM_* code, the one that
cuts a call over many sessions into native calls, and the handle base (on NativeLM, the handle that needs no GPU)."""
import itertools
import os
import re

import numpy as np
import pytest

from danspeech_amd import _native
from danspeech_amd import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "dsmi.h"), encoding="utf-8").read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _header_constants():
    """#define DSMI_X <integer> and the enumerators DSMI_X = <integer>."""
    src = _header()
    found = re.findall(r"^#define\s+(DSMI_[A-Z0-9_]+)\s+(-?\d+)\s*$", src, flags=re.M)
    found += re.findall(r"\b(DSMI_[A-Z0-9_]+)\s*=\s*(-?\d+)\s*[,}]", src)
    values = {name: int(v) for name, v in found}
    assert len(values) == len(found)
    return values


def _header_struct(name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, _header()).group(1)
    return re.findall(r"\b(\w+)\s*;", body)


def test_constants_have_the_headers_values():
    H = _header_constants()
    mirrored = [k for k in vars(_native) if k.startswith("DSMI_")]
    assert {"DSMI_ERR_INVALID", "DSMI_ERR_CONV", "DSMI_ERR_NOT_READY", "DSMI_ERR_UNSORTED", "DSMI_ERR_CAPACITY", "DSMI_ERR_TIMEOUT",
            "DSMI_ERR_COMM", "DSMI_RECOMPUTED"} <= set(mirrored)
    for k in mirrored:
        assert getattr(_native, k) == H[k], k
    for k in ("RESAMPLE_STREAM_MAX", "ENDPOINT_MAX", "STREAM_MANY_MAX", "BEAM_STREAM_MANY_MAX", "ALIGN_MAX_TOKENS"):
        assert getattr(_native, k) == H["DSMI_" + k], k
    assert _native.RESAMPLE_METHODS == {"polyphase": H["DSMI_RESAMPLE_POLYPHASE"], "ratecv": H["DSMI_RESAMPLE_RATECV"]}
    assert _native.WINDOWS == {"hamming": H["DSMI_WIN_HAMMING"], "hann": H["DSMI_WIN_HANN"], "blackman": H["DSMI_WIN_BLACKMAN"],
                               "bartlett": H["DSMI_WIN_BARTLETT"]}
    assert _native.PAD_MODES == {"reflect": H["DSMI_PAD_REFLECT"], "constant": H["DSMI_PAD_CONSTANT"]}
    assert _native.RNN_TYPES == {"gru": H["DSMI_RNN_GRU"], "lstm": H["DSMI_RNN_LSTM"], "rnn": H["DSMI_RNN_TANH"]}
    assert _native.PCM_DTYPES == {np.dtype(np.int16): H["DSMI_PCM_I16"], np.dtype(np.float32): H["DSMI_PCM_F32"],
                                  np.dtype(np.float64): H["DSMI_PCM_F64"]}
    assert _native.WAV_WIDTH_DTYPE == {1: H["DSMI_PCM_U8"], 2: H["DSMI_PCM_I16"], 3: H["DSMI_PCM_I24"], 4: H["DSMI_PCM_I32"]}
    assert _native.PCM_STEREO == H["DSMI_PCM_STEREO"]
    assert _native.NativeFrontend.PCM_STEREO == _native.PCM_STEREO and _native.NativeFrontend.WAV_WIDTH_DTYPE == _native.WAV_WIDTH_DTYPE


@pytest.mark.parametrize("desc, struct", [(_native.ModelDesc, "dsmi_model_desc"), (_native.FrontendDesc, "dsmi_frontend_desc"),
                                          (_native.EndpointerDesc, "dsmi_endpointer_desc")])
def test_descriptors_have_the_headers_members(desc, struct):
    assert [f[0] for f in desc._fields_] == _header_struct(struct)


# the table of include/dsmi.h, written out
DTYPE_CODE = {"int16": 0, "float32": 1, "float64": 2}
WIDTH_CODE = {1: 3, 2: 0, 3: 4, 4: 5}
CODE_BYTES = {0: 2, 1: 4, 2: 8, 3: 1, 4: 3, 5: 4}


def test_pcm_code_of_every_input():
    torch = pytest.importorskip("torch")
    for name, code in DTYPE_CODE.items():
        for dtype in (np.dtype(name), getattr(np, name), name, getattr(torch, name), torch.zeros(1, dtype=getattr(torch, name)).dtype):
            assert _native._pcm_code(dtype) == code, dtype
        assert _native._pcm_frame_bytes(code) == CODE_BYTES[code] == np.dtype(name).itemsize
    raw = torch.zeros(24, dtype=torch.uint8)
    for width, channels in itertools.product((1, 2, 3, 4), (1, 2)):
        code = WIDTH_CODE[width] + (16 if channels == 2 else 0)
        assert _native._pcm_code(None, (width, channels)) == code
        assert _native._pcm_code(raw.dtype, (width, channels)) == code
        assert _native._pcm_code(raw.dtype, (width, channels), 24 // (width * channels), raw.numel()) == code
        assert _native._pcm_frame_bytes(code) == CODE_BYTES[WIDTH_CODE[width]] * channels == width * channels


def test_pcm_code_refusals():
    torch = pytest.importorskip("torch")
    raw = torch.zeros(24, dtype=torch.uint8)
    for dtype, wav_format, n_frames, nbytes in ((raw.dtype, (5, 1), None, None), (None, (5, 1), None, None), (raw.dtype, (0, 1), None, None),
                                                (raw.dtype, (2, 3), None, None), (None, (2, 0), None, None),
                                                (torch.int16, (2, 1), None, None), (torch.float32, (4, 2), 3, 24),
                                                (raw.dtype, (2, 2), 5, 24), (raw.dtype, (3, 1), 7, 24), (raw.dtype, (1, 1), 25, 24)):
        with pytest.raises(ValueError):
            _native._pcm_code(dtype, wav_format, n_frames, nbytes)


@pytest.mark.parametrize("size", [0, 1, 4, 5, 11])
def test_cut_gives_slices_of_at_most_max_n_that_join_to_the_lists(size):
    max_n = 4
    a, b, c = list(range(size)), [str(k) for k in range(size)], np.arange(size) * 3
    cuts = list(_native._cut(max_n, a, b, c))
    assert len(cuts) == -(-size // max_n)
    assert [len(s[0]) for s in cuts] == [max_n] * (size // max_n) + ([size % max_n] if size % max_n else [])
    assert all(len(s) == 3 and len(s[0]) == len(s[1]) == len(s[2]) for s in cuts)
    assert sum((list(s[0]) for s in cuts), []) == a and sum((list(s[1]) for s in cuts), []) == b
    assert np.array_equal(np.concatenate([s[2] for s in cuts] + [c[:0]]), c)


def test_handle_base_on_a_handle_that_needs_no_gpu(tmp_path):
    arpa = str(tmp_path / "syn3.arpa")
    syn.make_arpa(arpa, order=3, n_words=300, seed=8, ngrams_per_order=800)
    made = _native._handles[0]
    lm = _native.NativeLM(arpa)
    assert lm._h and lm.order == 3 and lm.kind == "arpa"
    assert _native._handles[0] == made          # a host-only handle says nothing about the GPU runtime
    lm.close()
    assert not lm._h
    lm.close()
    assert not lm._h
    # a failed open: DsmiError with the library's text, and no handle
    lm = _native.NativeLM.__new__(_native.NativeLM)
    with pytest.raises(_native.DsmiError) as e:
        lm.__init__(str(tmp_path / "missing.arpa"))
    text = (_native.lib().dsmi_lm_last_error(None) or b"").decode()
    assert e.value.code == _header_constants()["DSMI_ERR_IO"] and text and e.value.msg == text and text in str(e.value)
    assert not hasattr(lm, "_h")
    lm.close()


def test_push_many_refusals_keep_their_texts_and_come_before_any_native_call():
    """What Python itself refuses, in the words it has always used; stand-ins for the handles show that no native call is reached."""
    torch = pytest.importorskip("torch")
    from types import SimpleNamespace as NS
    fe = NS(_h=1)
    chunk = torch.zeros(8, dtype=torch.int16)          # (not on a GPU)

    def refusal(cls, sessions, pcms):
        with pytest.raises(ValueError) as e:
            cls.push_many(sessions, pcms, [False] * len(sessions))
        return str(e.value)

    R, E = _native.NativeResampler, _native.NativeEndpointer
    live, closed, orphan = NS(_h=1, frontend=fe, frame_bytes=2), NS(_h=None, frontend=fe, frame_bytes=2), NS(_h=1, frontend=NS(_h=None), frame_bytes=2)
    assert refusal(R, [live], [chunk]) == "chunks must be contiguous CUDA tensors"
    assert refusal(E, [live], [chunk]) == "pushes must be contiguous CUDA tensors"
    assert refusal(R, [live, closed], [None, None]) == "session 1: the resampler or its frontend has been closed"
    assert refusal(R, [live, live, orphan], [None, chunk, None]) == "session 2: the resampler or its frontend has been closed"
    assert refusal(E, [live, closed], [None, None]) == "session 1: the endpointer or its frontend has been closed"
    assert refusal(R, [live], []) == "resamplers, pcms and is_last must have one entry per session"
    assert refusal(E, [live], []) == "endpointers, pcms and end_of_stream must have one entry per session"
    with pytest.raises(ValueError, match="^streams, feats, is_first and is_last must have one entry per session$"):
        _native.NativeStream.forward_many([live], [], [False], [False])
    with pytest.raises(ValueError, match="^streams and probs_list must have one entry per stream$"):
        _native.NativeBeamStream.advance_many([live], [])
    # a look-ahead: the closed handle of the second native call is found before the first call is made
    many = [live] * _native.RESAMPLE_STREAM_MAX + [closed]
    assert refusal(R, many, [None] * len(many)) == "session %d: the resampler or its frontend has been closed" % _native.RESAMPLE_STREAM_MAX
