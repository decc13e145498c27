"""CPU checks of the resumable beam search's C ABI (dsmi_beam_stream_*): the refusals that happen before any handle is
dereferenced or any HIP call is made -- null handles and arguments, n <= 0, a handle listed twice -- and the Python binding's
argument checks.  No kernels run."""
import ctypes

import pytest


def _L():
    from danspeech_amd import _native
    return _native, _native.lib()


def test_create_refuses_a_null_decoder():
    native, L = _L()
    h = ctypes.c_void_p()
    assert L.dsmi_beam_stream_create(None, 64, 40, 1.0, ctypes.byref(h)) == native.DSMI_ERR_INVALID
    assert h.value is None
    assert b"bad beam stream arguments" in L.dsmi_beam_stream_last_error(None)


def test_handle_calls_refuse_null():
    native, L = _L()
    f = ctypes.c_int64(7)
    assert L.dsmi_beam_stream_reset(None) == native.DSMI_ERR_INVALID
    assert L.dsmi_beam_stream_frames(None, ctypes.byref(f)) == native.DSMI_ERR_INVALID
    assert f.value == 7
    L.dsmi_beam_stream_destroy(None)          # a no-op


def test_advance_refusals_that_need_no_device():
    native, L = _L()
    fr = (ctypes.c_int32 * 2)(3, 3)
    pp = (ctypes.c_void_p * 2)(None, None)
    hs = (ctypes.c_void_p * 2)(None, None)
    assert L.dsmi_beam_stream_advance_many(None, 1, pp, fr, 0, None) == native.DSMI_ERR_INVALID
    for n in (0, -1, native.BEAM_STREAM_MANY_MAX + 1):
        assert L.dsmi_beam_stream_advance_many(hs, n, pp, fr, 0, None) == native.DSMI_ERR_INVALID
    assert L.dsmi_beam_stream_advance_many(hs, 2, pp, None, 0, None) == native.DSMI_ERR_INVALID
    assert L.dsmi_beam_stream_advance_many(hs, 2, pp, fr, 0, None) == native.DSMI_ERR_INVALID
    assert b"beam stream 0: null handle" in L.dsmi_beam_stream_last_error(None)
    # a handle listed twice is refused before any handle is looked at (the address is never dereferenced)
    fake = ctypes.create_string_buffer(64)
    dup = (ctypes.c_void_p * 2)(ctypes.addressof(fake), ctypes.addressof(fake))
    assert L.dsmi_beam_stream_advance_many(dup, 2, pp, fr, 1, None) == native.DSMI_ERR_INVALID
    assert b"appears twice" in L.dsmi_beam_stream_last_error(None)


def test_collect_refusals_that_need_no_device():
    native, L = _L()
    i32 = (ctypes.c_int32 * 64)()
    f32 = (ctypes.c_float * 64)()
    hs = (ctypes.c_void_p * 2)(None, None)
    assert L.dsmi_beam_stream_collect_many(None, 1, 1, 4, i32, i32, i32, f32, i32) == native.DSMI_ERR_INVALID
    assert L.dsmi_beam_stream_collect_many(hs, 0, 1, 4, i32, i32, i32, f32, i32) == native.DSMI_ERR_INVALID
    assert L.dsmi_beam_stream_collect_many(hs, 2, 0, 4, i32, i32, i32, f32, i32) == native.DSMI_ERR_INVALID
    assert L.dsmi_beam_stream_collect_many(hs, 2, 1, 0, i32, i32, i32, f32, i32) == native.DSMI_ERR_INVALID
    assert L.dsmi_beam_stream_collect_many(hs, 2, 1, 4, None, i32, i32, f32, i32) == native.DSMI_ERR_INVALID
    assert L.dsmi_beam_stream_collect_many(hs, 2, 1, 4, i32, i32, i32, f32, i32) == native.DSMI_ERR_INVALID
    fake = ctypes.create_string_buffer(64)
    dup = (ctypes.c_void_p * 2)(ctypes.addressof(fake), ctypes.addressof(fake))
    assert L.dsmi_beam_stream_collect_many(dup, 2, 1, 4, i32, i32, i32, f32, i32) == native.DSMI_ERR_INVALID
    assert b"appears twice" in L.dsmi_beam_stream_last_error(None)


def test_python_advance_many_checks_its_lists():
    native, _ = _L()
    with pytest.raises(ValueError):
        native.NativeBeamStream.advance_many([object()], [], 1)
    assert native.NativeBeamStream.advance_many([], [], 0) is None
    assert native.NativeBeamStream.advance_many([], [], 2) == []


def test_lm_partials_needs_a_language_model():
    """enable_streaming(lm_partials=True) on a greedy recogniser is refused before anything is set up"""
    from danspeech_amd.DanSpeechRecognizer import DanSpeechRecognizer
    rec = DanSpeechRecognizer.__new__(DanSpeechRecognizer)
    rec.lm = "greedy"
    rec.decoder = None
    rec._session = None
    with pytest.raises(ValueError):
        rec.enable_streaming(lm_partials=True)
    assert rec._session is None
