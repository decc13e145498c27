"""ctypes binding of libdsmi.so (include/dsmi.h).

The HIP library is the product: there is no CPU or eager-PyTorch fallback.  If the
shared object is missing, importing this module's users works (so that pure-host
logic can be tested without a GPU) but the first call that needs a kernel raises
``NativeLibraryMissing`` with the build command.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSMI_LIBRARY: another build of the same ABI -- tools/exp/ load lib/libdsmi_exp.so (`make -C danspeech_amd/csrc exp`: the timing
# instantiations and A/B switches that libdsmi.so does not carry)
LIB_PATH = os.environ.get("DSMI_LIBRARY") or os.path.join(_HERE, "lib", "libdsmi.so")

# The values of include/dsmi.h, restated (tests/test_native_binding_host.py holds every one of them against the header).
RNN_TYPES = {"gru": 0, "lstm": 1, "rnn": 2}
WINDOWS = {"hamming": 0, "hann": 1, "blackman": 2, "bartlett": 3}
PCM_DTYPES = {np.dtype(np.int16): 0, np.dtype(np.float32): 1, np.dtype(np.float64): 2}
WAV_WIDTH_DTYPE = {1: 3, 2: 0, 3: 4, 4: 5}            # sample width in bytes -> DSMI_PCM_{U8,I16,I24,I32}
PCM_STEREO = 16
_PCM_BYTES = (2, 4, 8, 1, 3, 4)                       # DSMI_PCM_* (without the stereo bit) -> bytes per sample
PAD_MODES = {"reflect": 0, "constant": 1}
RESAMPLE_METHODS = {"polyphase": 0, "ratecv": 1}      # DSMI_RESAMPLE_*
RESAMPLE_STREAM_MAX = 256       # sessions of one dsmi_resampler_push_many call
ENDPOINT_MAX = 256              # sessions of one dsmi_endpointer_push_many call
STREAM_MANY_MAX = 256           # sessions of one dsmi_stream_forward_many call
BEAM_STREAM_MANY_MAX = 4096     # streams of one dsmi_beam_stream_advance_many launch
ALIGN_MAX_TOKENS = 4096         # the longest transcript dsmi_align takes (L_stride)
ALIGN_LONG_MAX_TOKENS = 1 << 20 # the longest transcript dsmi_align_long takes
ALIGN_LONG_MAX_FRAMES = 1 << 22 # the most frames dsmi_align_long takes
SPOT_MAX_TOKENS = 128           # the longest phrase dsmi_spot takes (L_stride)
SPOT_MAX_PHRASES = 4096         # phrases of one dsmi_spot call
SPOT_MAX_HITS = 64              # hits per (clip, phrase) of one dsmi_spot call
SPOT_STREAM_MANY_MAX = 4096     # streams of one dsmi_spot_stream_advance_many launch
SCORE_MAX_TOKENS = 2048         # the longest candidate dsmi_score takes (L_stride)
ALT_MAX_TOKENS = 1024           # the longest candidate dsmi_alternatives takes (L_stride)
OCC_MAX_TOKENS = 1024           # the longest candidate dsmi_occupancy takes (L_stride)
GRAMMAR_MAX_NODES = 2048        # the most nodes of one graph dsmi_grammar takes
GRAMMAR_MAX_ARCS = 8192         # the most arcs of one graph dsmi_grammar takes
GRAMMAR_STREAM_MANY_MAX = 4096  # streams of one dsmi_grammar_stream_advance_many launch
GRAMMAR_STREAM_MAX_FRAMES = 1 << 20      # the most frames of one dsmi_grammar_stream's utterance
GRAMMAR_START, GRAMMAR_FINAL = 1, 2   # DSMI_GRAMMAR_START, DSMI_GRAMMAR_FINAL: a node's flags
EDIT_MAX_TOKENS = 4096          # the longest sequence dsmi_edit_distance takes (L_stride)
LM_SCORE_MAX_TOKENS = 4096      # the longest sequence dsmi_lm_score takes (L_stride)

DSMI_ERR_INVALID = -1
DSMI_ERR_CONV = -2
DSMI_ERR_NOT_READY = -3
DSMI_ERR_UNSORTED = -4
DSMI_ERR_CAPACITY = -8
DSMI_ERR_TIMEOUT = -9
DSMI_ERR_COMM = -10
DSMI_RECOMPUTED = 1


class NativeLibraryMissing(RuntimeError):
    pass


class DsmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libdsmi error %d: %s" % (code, msg))
        self.code = code
        self.msg = msg


class ModelDesc(C.Structure):
    _fields_ = [
        ("conv_layers", C.c_int32), ("rnn_type", C.c_int32), ("rnn_hidden_size", C.c_int32),
        ("rnn_layers", C.c_int32), ("bidirectional", C.c_int32), ("context", C.c_int32),
        ("n_labels", C.c_int32), ("sample_rate", C.c_int32), ("window_size", C.c_double),
    ]


class EndpointerDesc(C.Structure):
    _fields_ = [
        ("chunk", C.c_int32), ("rate", C.c_int32), ("pcm_dtype", C.c_int32), ("energy_threshold", C.c_double),
        ("pause_threshold", C.c_double), ("phrase_threshold", C.c_double), ("non_speaking_duration", C.c_double),
    ]


class FrontendDesc(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_int32), ("window_size", C.c_double), ("window_stride", C.c_double),
        ("window", C.c_int32), ("normalize", C.c_int32), ("pad_mode", C.c_int32),
    ]


class GrammarPool(C.Structure):
    _fields_ = [
        ("K", C.c_int32), ("node_off", C.c_void_p), ("labels", C.c_void_p), ("weights", C.c_void_p), ("flags", C.c_void_p),
        ("arc_off", C.c_void_p), ("arc_pred", C.c_void_p), ("empty_ok", C.c_void_p),
    ]


_lib = None

_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f32p = C.POINTER(C.c_float)
_vp = C.c_void_p

_PROTOS = {
    "dsmi_model_create": (C.c_int, [C.POINTER(ModelDesc), C.c_int, C.POINTER(_vp)]),
    "dsmi_model_load_tensor": (C.c_int, [_vp, C.c_char_p, _vp, _i64p, C.c_int]),
    "dsmi_model_finalize": (C.c_int, [_vp]),
    "dsmi_reserve": (C.c_int, [_vp, C.c_int, C.c_int]),
    "dsmi_model_destroy": (None, [_vp]),
    "dsmi_last_error": (C.c_char_p, [_vp]),
    "dsmi_seq_lens": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "dsmi_frontend_create": (C.c_int, [C.POINTER(FrontendDesc), C.c_int, C.POINTER(_vp)]),
    "dsmi_frontend_destroy": (None, [_vp]),
    "dsmi_frontend_last_error": (C.c_char_p, [_vp]),
    "dsmi_features": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, _vp]),
    "dsmi_features_stream": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, _vp, _vp, C.c_int, _vp, _vp]),
    "dsmi_resample": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64, _vp, _vp]),
    "dsmi_resample_count": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int64]),
    "dsmi_resample_taps": (C.c_int, [C.c_int, C.c_int, _vp, C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dsmi_resampler_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsmi_resampler_destroy": (None, [_vp]),
    "dsmi_resampler_last_error": (C.c_char_p, [_vp]),
    "dsmi_resampler_reset": (C.c_int, [_vp]),
    "dsmi_resampler_position": (C.c_int, [_vp, _i64p, _i64p]),
    "dsmi_resample_ready": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int64]),
    "dsmi_resampler_push_many": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp]),
    "dsmi_endpoint_counts": (C.c_int, [_vp, _vp]),
    "dsmi_endpoint_gate": (C.c_int64, [C.c_double, C.c_int64, C.c_int64, C.c_int64, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp,
                                       C.c_int64, _vp]),
    "dsmi_endpointer_create": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "dsmi_endpointer_destroy": (None, [_vp]),
    "dsmi_endpointer_last_error": (C.c_char_p, [_vp]),
    "dsmi_endpointer_reset": (C.c_int, [_vp]),
    "dsmi_endpointer_position": (C.c_int, [_vp, _i64p, _i64p, _i64p]),
    "dsmi_endpointer_push_many": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_int, C.POINTER(C.c_int), _vp,
                                            _vp]),
    "dsmi_stream_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "dsmi_stream_destroy": (None, [_vp]),
    "dsmi_stream_last_error": (C.c_char_p, [_vp]),
    "dsmi_stream_reset": (C.c_int, [_vp]),
    "dsmi_stream_forward": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp]),
    "dsmi_stream_forward_many": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, _vp]),
    "dsmi_features_stream_many": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp]),
    "dsmi_segment": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, C.c_int, C.c_double, C.c_int, C.c_int, _vp, _vp, C.c_int,
                               C.POINTER(C.c_int), _vp, _vp]),
    "dsmi_decoder_create": (C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsmi_decoder_destroy": (None, [_vp]),
    "dsmi_decoder_last_error": (C.c_char_p, [_vp]),
    "dsmi_decoder_set_lm": (C.c_int, [_vp, C.c_char_p, C.c_double, C.c_double]),
    "dsmi_beam": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_forward": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "dsmi_forward_ready": (C.c_int, [_vp]),
    "dsmi_forward_status": (C.c_int, [_vp]),
    "dsmi_recompute_count": (C.c_int, [_vp]),
    "dsmi_model_set_inflight": (C.c_int, [_vp, C.c_int]),
    "dsmi_model_set_ring_windows": (C.c_int, [_vp, C.c_int]),
    "dsmi_pack_pcm_i16": (C.c_int, [_vp, C.c_int64, _vp]),
    "dsmi_upload": (C.c_int, [C.c_int, _vp, _vp, C.c_int64, _vp]),
    "dsmi_conv_stack": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "dsmi_rnn_layer": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "dsmi_head": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    "dsmi_greedy": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "dsmi_greedy_enqueue": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp]),
    "dsmi_greedy_collect": (C.c_int, [_vp, _vp, _vp, _vp]),
    "dsmi_set_profiling": (C.c_int, [_vp, C.c_int]),
    "dsmi_stage_time_us": (C.c_double, [_vp, C.c_int]),
    "dsmi_kernel_stats": (C.c_int, [_vp, C.c_int, _i64p, _i64p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsmi_reset_kernel_stats": (C.c_int, [_vp]),
    "dsmi_debug_persist_stamps": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64]),
    "dsmi_debug_step_stamps": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int64]),
    "dsmi_debug_last_rnn_plan": (C.c_int, [_vp, C.c_char_p, C.c_int64]),
    "dsmi_debug_xproj": (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp]),
    "dsmi_debug_conv_workgroups": (C.c_int, [_vp, _vp, C.c_int32]),
    "dsmi_debug_dense_stamps": (C.c_int, [_vp, C.c_int64]),
    "dsmi_last_forward_stats": (C.c_int, [_vp, _i64p, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsmi_lm_open": (C.c_int, [C.c_char_p, C.POINTER(_vp)]),
    "dsmi_lm_close": (None, [_vp]),
    "dsmi_lm_last_error": (C.c_char_p, [_vp]),
    "dsmi_lm_info": (C.c_int, [_vp, C.POINTER(C.c_int), _i64p, C.POINTER(C.c_int)]),
    "dsmi_lm_word_index": (C.c_int, [_vp, C.c_char_p]),
    "dsmi_lm_lookup": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "dsmi_lm_cond_log10": (C.c_double, [_vp, _vp, C.c_int]),
    "dsmi_beam_enqueue": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _vp]),
    "dsmi_beam_collect": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "dsmi_decoder_beam_stats": (C.c_int, [_vp, _vp]),
    "dsmi_debug_beam_stamps": (C.c_int, [_vp, _vp, C.c_int64]),
    "dsmi_beam_stream_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.POINTER(_vp)]),
    "dsmi_beam_stream_destroy": (None, [_vp]),
    "dsmi_beam_stream_last_error": (C.c_char_p, [_vp]),
    "dsmi_beam_stream_reset": (C.c_int, [_vp]),
    "dsmi_beam_stream_frames": (C.c_int, [_vp, _i64p]),
    "dsmi_beam_stream_advance_many": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp]),
    "dsmi_beam_stream_collect_many": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_align": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_align_long": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_align_long_plan": (C.c_int, [C.c_int, C.c_int, _i64p]),
    "dsmi_spot_plan": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "dsmi_spot": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_spot_watch_create": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(_vp)]),
    "dsmi_spot_watch_destroy": (None, [_vp]),
    "dsmi_spot_watch_last_error": (C.c_char_p, [_vp]),
    "dsmi_spot_watch_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dsmi_spot_stream_create": (C.c_int, [_vp, C.POINTER(_vp)]),
    "dsmi_spot_stream_destroy": (None, [_vp]),
    "dsmi_spot_stream_last_error": (C.c_char_p, [_vp]),
    "dsmi_spot_stream_reset": (C.c_int, [_vp]),
    "dsmi_spot_stream_frames": (C.c_int, [_vp, _i64p]),
    "dsmi_spot_stream_advance_many": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "dsmi_spot_watch_pick": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    "dsmi_score_plan": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "dsmi_score": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    "dsmi_alternatives": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "dsmi_grammar": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(GrammarPool), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_grammar_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _i64p]),
    "dsmi_grammar_posterior": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(GrammarPool), _vp, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_grammar_posterior_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _i64p]),
    "dsmi_grammar_net_create": (C.c_int, [_vp, C.POINTER(GrammarPool), C.POINTER(_vp)]),
    "dsmi_grammar_net_destroy": (None, [_vp]),
    "dsmi_grammar_net_last_error": (C.c_char_p, [_vp]),
    "dsmi_grammar_net_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dsmi_grammar_stream_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsmi_grammar_stream_destroy": (None, [_vp]),
    "dsmi_grammar_stream_last_error": (C.c_char_p, [_vp]),
    "dsmi_grammar_stream_reset": (C.c_int, [_vp]),
    "dsmi_grammar_stream_frames": (C.c_int, [_vp, _i64p]),
    "dsmi_grammar_stream_advance_many": (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_grammar_stream_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _i64p]),
    "dsmi_occupancy": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "dsmi_edit_plan": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp]),
    "dsmi_edit_distance": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _vp, _vp]),
    "dsmi_lm_score_plan": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int]),
    "dsmi_lm_score": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "dsmi_lm_sentence_ln": (C.c_double, [_vp, _vp, C.c_int, _vp, C.c_int]),
    "dsmi_model_info": (C.c_int, [_vp, C.POINTER(ModelDesc), C.POINTER(C.c_int)]),
    "dsmi_frontend_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dsmi_decoder_info": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dsmi_decoder_label": (C.c_char_p, [_vp, C.c_int]),
    "dsmi_session_create": (C.c_int, [_vp, _vp, _vp, C.POINTER(_vp)]),
    "dsmi_session_destroy": (None, [_vp]),
    "dsmi_session_last_error": (C.c_char_p, [_vp]),
    "dsmi_recognize_batch": (C.c_int, [_vp, C.POINTER(_vp), _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, _vp]),
    "dsmi_recognize_enqueue": (C.c_int, [_vp, C.POINTER(_vp), _vp, C.c_int, C.c_int]),
    "dsmi_recognize_enqueue_device": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    "dsmi_recognize_collect": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _vp, _vp]),
    "dsmi_plan_shards": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "dsmi_comm_unique_id": (C.c_int, [_vp]),
    "dsmi_comm_init": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "dsmi_comm_destroy": (None, [_vp]),
    "dsmi_comm_last_error": (C.c_char_p, [_vp]),
    "dsmi_comm_scatter": (C.c_int, [_vp, C.c_int, C.POINTER(_vp), _vp, C.c_int, C.c_int, C.POINTER(_vp), _vp, _vp, C.c_int,
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _vp]),
    "dsmi_comm_gather_text": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp]),
}


def declared_symbols():
    """Every function include/dsmi.h declares (used by the CPU-side export test)."""
    return sorted(_PROTOS)


_hw_queue_note = [False]


def want_hw_queues(n=8):
    """The batch pipeline keeps four forwards in flight on four streams beside a decode stream; the ROCm runtime maps a process's
    streams onto FOUR hardware queues by default, and two streams that share one run one after the other (a forward's persistent
    recurrent kernel behind another forward's dense kernels: 9.7 against 5.9 ms per batch, tools/exp/pipeline_lanes.py).  The
    runtime reads GPU_MAX_HW_QUEUES once, at the process's first GPU call: an engine asks for ``n`` when it is made
    (``DanSpeechRecognizer.__init__``), which takes effect if nothing has touched the GPU yet; a value the caller has set is kept;
    otherwise one warning says what the pipeline will cost."""
    if os.environ.get("GPU_MAX_HW_QUEUES"):
        return
    touched = _lib is not None and _handles[0] > 0
    try:
        import torch
        touched = touched or torch.cuda.is_initialized()
    except ImportError:
        pass
    if not touched:
        os.environ["GPU_MAX_HW_QUEUES"] = str(n)
    elif not _hw_queue_note[0]:
        _hw_queue_note[0] = True
        import warnings
        warnings.warn("danspeech_amd: the GPU runtime was initialised before the recognizer was made and GPU_MAX_HW_QUEUES is not set: "
                      "the batch pipeline's streams will share four hardware queues (recognize_batches runs up to 1.6x slower). "
                      "Set GPU_MAX_HW_QUEUES=8 in the environment, or create the Recognizer before the first GPU call.", RuntimeWarning)


_handles = [0]          # native handles made so far (any of them has initialised the GPU runtime)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                "%s not found: build it with `make -C danspeech_amd/csrc` (hipcc, gfx950) or "
                "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _np_ptr(a):
    return a.ctypes.data_as(_vp)       # (the pointer keeps ``a`` alive)


def _stream(device=None):
    """The torch stream current on ``device`` (the HANDLE's device, not torch's current device)."""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _Handle:
    """Owns one native handle, ``_h``.  A subclass names the two entry points that go with it: ``_destroy`` and ``_last_error``
    (which, given no handle, tells the calling thread's last error: that of a failed create or of a call over many handles)."""
    _destroy = _last_error = None
    _host_only = False      # no GPU behind the handle: making one says nothing to want_hw_queues
    _finalise = True        # close when the object is collected

    def _create(self, create, *args):
        if not self._host_only:
            _handles[0] += 1
        h = _vp()
        self._check_thread(getattr(lib(), create)(*args, C.byref(h)))
        self._h = h

    @classmethod
    def _error(cls, h=None):
        return (getattr(lib(), cls._last_error)(h) or b"").decode()

    @classmethod
    def _check_thread(cls, rc):
        if rc != 0:
            raise DsmiError(rc, cls._error())

    def _check(self, rc):
        if rc != 0:
            raise DsmiError(rc, self._error(self._h))

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        if self._finalise:
            try:
                self.close()
            except Exception:
                pass


# ---- the DSMI_PCM_* code of a buffer
_TORCH_CODES = {}       # torch dtype -> DSMI_PCM_*: PCM_DTYPES by name, made when the first tensor arrives (torch stays a lazy import)


def _pcm_code(dtype, wav_format=None, n_frames=None, nbytes=None):
    """DSMI_PCM_* of samples of ``dtype`` (numpy or torch: int16 / float32 / float64) -- or, with ``wav_format=(sample_width,
    channels)``, of the raw frames of a PCM WAV file, which a tensor holds as uint8 (``dtype`` None: there is no tensor yet).
    ``n_frames`` with ``nbytes``: the frames must fill a buffer of that many bytes."""
    of_torch = type(dtype).__module__ == "torch"
    if of_torch:
        import torch
    if wav_format is None:
        if not of_torch:
            return PCM_DTYPES[np.dtype(dtype)]
        if not _TORCH_CODES:
            _TORCH_CODES.update((getattr(torch, d.name), code) for d, code in PCM_DTYPES.items())
        return _TORCH_CODES[dtype]
    width, channels = wav_format
    raw = dtype is None or (dtype == torch.uint8 if of_torch else np.dtype(dtype) == np.uint8)
    if not raw or width not in WAV_WIDTH_DTYPE or channels not in (1, 2):
        raise ValueError("raw WAV frames: %ssample width 1..4, one or two channels" % ("" if dtype is None else "uint8 tensor, "))
    if nbytes is not None and int(n_frames) * width * channels != nbytes:
        raise ValueError("frame counts do not add up to the size of the byte buffer")
    return WAV_WIDTH_DTYPE[width] | (PCM_STEREO if channels == 2 else 0)


def _pcm_frame_bytes(code):
    return _PCM_BYTES[code & 15] * (2 if code & PCM_STEREO else 1)


# ---- the calls over many sessions: everything Python checks is checked for all of them before the first native call
def _cut(max_n, *lists):
    """Parallel lists -> the tuples of their slices of at most ``max_n`` entries, in order: the lists themselves when they are
    no longer than that, nothing when they are empty."""
    n = len(lists[0])
    if n <= max_n:
        return [lists] if n else []
    return [tuple(l[k:k + max_n] for l in lists) for k in range(0, n, max_n)]


def _handle_array(objs):
    return (C.c_void_p * len(objs))(*[o._h for o in objs])


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def _flag_array(flags):
    return np.array([int(bool(v)) for v in flags], dtype=np.int32)


def _pushes(sessions, pcms, kind, push, pushes):
    """Of the sessions of a ``push_many`` (handles on a frontend, with ``frame_bytes``) and what each is given: refuse a closed
    handle, a tensor the library cannot read and a tensor that is no whole number of frames.
    -> (frames per session, the tensors with None for every empty one)."""
    for i, s in enumerate(sessions):
        # the handle points into its frontend (the filters): a push after either was closed would read freed memory
        if not getattr(s, "_h", None) or not getattr(s.frontend, "_h", None):
            raise ValueError("session %d: the %s or its frontend has been closed" % (i, kind))
    for p in pcms:
        if p is not None and not (p.is_cuda and p.is_contiguous()):
            raise ValueError("%s must be contiguous CUDA tensors" % pushes)
    frames, given = [], []
    for s, p in zip(sessions, pcms):
        nbytes = 0 if p is None else p.numel() * p.element_size()
        if nbytes % s.frame_bytes:
            raise ValueError("the %s is not a whole number of samples of the %s's type" % (push, kind))
        frames.append(nbytes // s.frame_bytes)
        given.append(p if nbytes else None)
    return frames, given


class NativeModel(_Handle):
    """Owns one dsmi_model handle (one GPU)."""
    _destroy, _last_error = "dsmi_model_destroy", "dsmi_last_error"

    def __init__(self, cfg, state_dict, device=0, audio_conf=None, n_labels=33):
        L = lib()
        ac = audio_conf or {}
        d = ModelDesc()
        d.conv_layers = int(cfg["conv_layers"])
        d.rnn_type = RNN_TYPES[cfg["rnn_type"]]
        d.rnn_hidden_size = int(cfg["rnn_hidden_size"])
        d.rnn_layers = int(cfg["rnn_layers"])
        d.bidirectional = int(bool(cfg["bidirectional"]))
        d.context = int(cfg.get("context", 20))
        d.n_labels = int(n_labels)
        d.sample_rate = int(ac.get("sampling_rate", 16000))
        d.window_size = float(ac.get("window_size", 0.02))
        self.desc = d
        self.n_labels = int(n_labels)
        self.device = device
        self._create("dsmi_model_create", C.byref(d), device)
        for name, t in state_dict.items():
            a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
            if a.dtype == np.int64:   # num_batches_tracked
                continue
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (C.c_int64 * max(a.ndim, 1))(*a.shape)
            self._check(L.dsmi_model_load_tensor(self._h, name.encode(), _np_ptr(a), shape, a.ndim))
        self._check(L.dsmi_model_finalize(self._h))

    # ---- host arithmetic
    def seq_lens(self, lens):
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        out = np.empty_like(lens)
        self._check(lib().dsmi_seq_lens(self._h, _np_ptr(lens), len(lens), _np_ptr(out)))
        return out

    def reserve(self, max_batch, max_frames):
        self._check(lib().dsmi_reserve(self._h, int(max_batch), int(max_frames)))

    # ---- device entry points (torch tensors only as containers)
    def _stream(self):
        return _stream(self.device)

    def _on_device(self, t):
        assert t.is_cuda and t.device.index == self.device, "tensor on %s, handle on cuda:%d" % (t.device, self.device)

    def forward(self, feat, lens, out=None, check=True):
        """feat: CUDA float32 [B,1,F,T] contiguous; lens sorted descending. -> (probs [B,T',C], out_lens).

        The kernels are enqueued asynchronously.  With ``check=True`` (default) the call then waits for them and
        collects the forward's status (``dsmi_forward_status``: a batch whose persistent recurrent kernel timed
        out is recomputed before this returns), so the probabilities are valid for any consumer.  A pipelining
        caller passes ``check=False`` and calls ``status()`` itself before consuming ``probs``."""
        import torch
        assert feat.dtype == torch.float32 and feat.is_contiguous()
        self._on_device(feat)
        B, T = feat.shape[0], feat.shape[-1]
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        To = int(self.seq_lens(np.array([T], dtype=np.int32))[0])
        probs = out if out is not None else torch.empty((B, To, self.n_labels), dtype=torch.float32, device=feat.device)
        out_lens = np.empty(B, dtype=np.int32)
        self._check(lib().dsmi_forward(self._h, feat.data_ptr(), _np_ptr(lens), B, T, probs.data_ptr(),
                                       _np_ptr(out_lens), self._stream()))
        if not hasattr(self, "_inflight"):
            self._inflight = []
        self._inflight.append((feat, probs))      # dsmi_forward_status may recompute from / into these buffers
        del self._inflight[:-4]
        if check:
            self.status()
        return probs, out_lens

    def status(self):
        """Wait for the oldest forward whose status has not been collected and collect it.  True when the batch had
        to be recomputed on the per-step path (results are valid either way; raises if the recompute failed)."""
        rc = lib().dsmi_forward_status(self._h)
        if getattr(self, "_inflight", None):
            self._inflight.pop(0)
        if rc == DSMI_RECOMPUTED:
            import warnings
            warnings.warn(self._error(self._h), RuntimeWarning)
            return True
        self._check(rc)
        return False

    def ready(self):
        """Has the oldest uncollected forward finished on the device (``status()`` would not block)?  Never blocks."""
        rc = lib().dsmi_forward_ready(self._h)
        if rc < 0:
            self._check(rc)
        return rc == 1

    def recompute_count(self):
        return int(lib().dsmi_recompute_count(self._h))

    RNN_LAUNCH_FIELDS = ("kernel", "at", "n", "nwin", "gate", "slot0", "nslots", "cus", "ticket", "part")

    def last_rnn_plan(self):
        """``(x16, [launch dict])``: the launches the last recurrent layer of this handle actually made, after any fallback
        (``dsmi_debug_last_rnn_plan``; csrc/rnn_plan.h ``RnnLaunch``).  ``kernel`` is one of steps, persist8, p16w8, p16w4, duo,
        ring8, ring4.  ``(False, [])`` before the first layer; of a layer of more than eight launches, the first eight."""
        buf = C.create_string_buffer(1400)
        rc = lib().dsmi_debug_last_rnn_plan(self._h, buf, len(buf))
        if rc < 0:
            self._check(rc)
        order, _, rest = buf.value.decode().partition("|")
        launches = []
        for item in rest.split(";")[:-1]:
            launches.append({k: (v if k in ("kernel", "gate") else (float(v) if k == "part" else int(v)))
                             for k, v in zip(self.RNN_LAUNCH_FIELDS, item.split())})
        return order == "x16", launches

    def set_inflight(self, batches):
        """How many batches the caller keeps in flight on this device (one handle + stream each): 2 selects the
        throughput variant of the recurrent kernel."""
        self._check(lib().dsmi_model_set_inflight(self._h, int(batches)))

    def set_ring_windows(self, windows):
        """Ring windows the next forwards' recurrent layers take side by side (0: what ``set_inflight`` implies)."""
        self._check(lib().dsmi_model_set_ring_windows(self._h, int(windows)))

    def conv_stack(self, feat, lens):
        import torch
        B, T = feat.shape[0], feat.shape[-1]
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        To = int(self.seq_lens(np.array([T], dtype=np.int32))[0])
        from .synthetic import CONV_SPECS, conv_out_freq
        cl = self.desc.conv_layers
        n_freq = int(self.desc.sample_rate * self.desc.window_size) // 2 + 1
        C_ = CONV_SPECS[cl - 1][1]
        F_ = conv_out_freq(n_freq, cl)
        out = torch.empty((B, C_, F_, To), dtype=torch.float32, device=feat.device)
        self._check(lib().dsmi_conv_stack(self._h, feat.data_ptr(), _np_ptr(lens), B, T, out.data_ptr(), self._stream()))
        return out

    def rnn_layer(self, layer, x, out_lens):
        """x: CUDA [T,B,I] -> [T,B,H] (one BatchRNN of the model)."""
        import torch
        T, B = x.shape[0], x.shape[1]
        out_lens = np.ascontiguousarray(out_lens, dtype=np.int32)
        y = torch.empty((T, B, self.desc.rnn_hidden_size), dtype=torch.float32, device=x.device)
        self._check(lib().dsmi_rnn_layer(self._h, int(layer), x.data_ptr(), _np_ptr(out_lens), B, T, y.data_ptr(), self._stream()))
        return y

    def head(self, x_fwd, x_rev=None):
        """x_fwd, x_rev: CUDA float32 [T,B,H], the last layer's outputs per direction (x_rev exactly when the model is
        bidirectional) -> probs [B,T,n_labels]: (Lookahead + Hardtanh for a unidirectional model,) BatchNorm1d, Linear, softmax."""
        import torch
        for x in (x_fwd,) + (() if x_rev is None else (x_rev,)):
            assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == tuple(x_fwd.shape) and x.dim() == 3
            assert x.shape[2] == self.desc.rnn_hidden_size, "rows of %d units, the model has %d" % (x.shape[2], self.desc.rnn_hidden_size)
            self._on_device(x)
        T, B = x_fwd.shape[0], x_fwd.shape[1]
        probs = torch.empty((B, T, self.n_labels), dtype=torch.float32, device=x_fwd.device)
        self._check(lib().dsmi_head(self._h, x_fwd.data_ptr(), None if x_rev is None else x_rev.data_ptr(), B, T, probs.data_ptr(), self._stream()))
        return probs

    KERNEL_KINDS = ["unused", "conv1", "conv2", "conv3", "gemm_l0", "gemm", "rnn_step", "head", "greedy", "beam", "rnn_layer_persistent"]

    def set_profiling(self, level):
        self._check(lib().dsmi_set_profiling(self._h, int(level)))

    def kernel_stats(self):
        """dict kind -> dict(launches, samples, avg_us, flops_per_launch, bytes_per_launch)."""
        out = {}
        for k, name in enumerate(self.KERNEL_KINDS):
            n = C.c_int64(); sm = C.c_int64(); us = C.c_double(); fl = C.c_double(); by = C.c_double()
            self._check(lib().dsmi_kernel_stats(self._h, k, C.byref(n), C.byref(sm), C.byref(us), C.byref(fl), C.byref(by)))
            if n.value:
                out[name] = dict(launches=n.value, samples=sm.value, avg_us=us.value,
                                 flops_per_launch=fl.value, bytes_per_launch=by.value)
        return out

    def reset_kernel_stats(self):
        self._check(lib().dsmi_reset_kernel_stats(self._h))

    def stage_time_us(self, stage):
        return float(lib().dsmi_stage_time_us(self._h, int(stage)))

    def last_forward_stats(self):
        n = C.c_int64(); a = C.c_double(); b = C.c_double()
        self._check(lib().dsmi_last_forward_stats(self._h, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value


def _resample_method(method):
    if method not in RESAMPLE_METHODS:
        raise ValueError("resample method must be one of %s" % sorted(RESAMPLE_METHODS))
    return RESAMPLE_METHODS[method]


class NativeFrontend(_Handle):
    """Owns one dsmi_frontend handle: SpectrogramAudioParser on one GPU."""
    _destroy, _last_error = "dsmi_frontend_destroy", "dsmi_frontend_last_error"
    PCM_STEREO = PCM_STEREO
    WAV_WIDTH_DTYPE = WAV_WIDTH_DTYPE

    def __init__(self, audio_conf=None, device=0, pad_mode="reflect"):
        ac = audio_conf or {}
        d = FrontendDesc()
        d.sample_rate = int(ac.get("sampling_rate", 16000))
        d.window_size = float(ac.get("window_size", 0.02))
        d.window_stride = float(ac.get("window_stride", 0.01))
        d.window = WINDOWS[ac.get("window", "hamming")]
        d.normalize = int(bool(ac.get("normalize", True)))
        d.pad_mode = PAD_MODES[pad_mode]
        self.desc = d
        self.device = device
        self.n_fft = int(d.sample_rate * d.window_size)
        self.hop = int(d.sample_rate * d.window_stride)
        self.n_freq = self.n_fft // 2 + 1
        self._create("dsmi_frontend_create", C.byref(d), device)

    def features(self, pcm_dev, n_samples, t_stride=None, wav_format=None, device=None):
        """pcm_dev: 1-D CUDA tensor (int16/float32/float64), clips back to back; or, with
        ``wav_format=(sample_width, channels)``, a uint8 tensor holding the raw frames of PCM WAV
        files back to back (``n_samples`` then counts frames; stereo is folded on the device).
        -> (feat [B,1,F,t_stride] float32 CUDA, frames int32[B])."""
        import torch
        n_samples = np.ascontiguousarray(n_samples, dtype=np.int64)
        B = len(n_samples)
        frames = 1 + n_samples // self.hop
        if t_stride is None:
            t_stride = int(frames.max())
        dt = _pcm_code(pcm_dev.dtype, wav_format, n_samples.sum(), pcm_dev.numel())
        feat = torch.empty((B, 1, self.n_freq, t_stride), dtype=torch.float32, device=device if device is not None else pcm_dev.device)
        fr = np.empty(B, dtype=np.int32)
        self._check(lib().dsmi_features(self._h, pcm_dev.data_ptr(), dt, _np_ptr(n_samples), B, feat.data_ptr(),
                                        int(t_stride), _np_ptr(fr), _stream(self.device)))
        return feat, fr

    def resample_count(self, n_samples, rate_in, method="polyphase"):
        """dsmi_resample_count: the lengths clips of ``n_samples`` samples at ``rate_in`` have at the frontend's rate (int64 array)."""
        m = _resample_method(method)
        out = np.array([lib().dsmi_resample_count(m, int(rate_in), int(self.desc.sample_rate), int(n))
                        for n in np.atleast_1d(n_samples)], dtype=np.int64)
        if (out < 0).any():
            raise DsmiError(DSMI_ERR_INVALID, "bad resample arguments (rate_in %r)" % (rate_in,))
        return out

    def resample(self, pcm_dev, n_samples, rate_in, method="polyphase", wav_format=None):
        """dsmi_resample: clips of ``rate_in`` Hz back to back in ``pcm_dev`` (a sample tensor, or raw WAV frames with
        ``wav_format=(sample_width, channels)``, as for ``features``) -> (float64 CUDA tensor with the clips at the frontend's
        rate back to back, their lengths int64[B]).  One launch on the current stream; nothing is synchronised."""
        import torch
        m = _resample_method(method)
        n_samples = np.ascontiguousarray(n_samples, dtype=np.int64)
        dt = _pcm_code(pcm_dev.dtype, wav_format, n_samples.sum(), pcm_dev.numel())
        if wav_format is None and int(n_samples.sum()) != pcm_dev.numel():
            raise ValueError("sample counts do not add up to the size of the buffer")
        counts = self.resample_count(n_samples, rate_in, method)
        total = int(counts.sum())
        if pcm_dev.numel() == 0:            # nothing but empty clips: nothing to launch
            return torch.empty(0, dtype=torch.float64, device=pcm_dev.device), counts
        out = torch.empty(max(total, 1), dtype=torch.float64, device=pcm_dev.device)
        n_out = np.zeros(len(n_samples), dtype=np.int64)
        self._check(lib().dsmi_resample(self._h, pcm_dev.data_ptr(), dt, _np_ptr(n_samples), len(n_samples), int(rate_in), m,
                                        out.data_ptr(), total, _np_ptr(n_out), _stream(self.device)))
        return out[:total], n_out

    def segment(self, pcm_dev, energy_threshold=600, step=1024, pause_hops=9, phrase_hops=4, wav_format=None,
                max_segments=None, return_energies=False):
        """dsmi_segment over ONE recording resident on the GPU -> int64 [n,2] sample ranges [start, end)
        (and the float64 hop energies)."""
        dt = _pcm_code(pcm_dev.dtype if wav_format is None else None, wav_format)
        n = pcm_dev.numel() if wav_format is None else pcm_dev.numel() // _pcm_frame_bytes(dt)
        nhops = max((n - 1) // step, 0) if n > step else 0
        cap = int(max_segments) if max_segments is not None else nhops // 2 + 1
        st = np.zeros(max(cap, 1), dtype=np.int64); en = np.zeros(max(cap, 1), dtype=np.int64)
        e = np.zeros(max(nhops, 1), dtype=np.float64)
        found = C.c_int(0)
        self._check(lib().dsmi_segment(self._h, pcm_dev.data_ptr(), dt, n, int(step), float(energy_threshold), int(pause_hops),
                                       int(phrase_hops), _np_ptr(st), _np_ptr(en), cap, C.byref(found), _np_ptr(e), _stream(self.device)))
        seg = np.stack([st[:found.value], en[:found.value]], axis=1)
        return (seg, e[:nhops]) if return_energies else seg

    def _stream_frames(self, n):
        """Frames the streaming parser makes of a chunk of ``n`` samples."""
        return 1 + (n - self.n_fft) // self.hop if n >= self.n_fft else 0

    def features_stream(self, pcm_dev, state):
        """dsmi_features_stream: one chunk of the streaming parser.  ``state`` = float64[3] (input_mean, input_std,
        alpha), updated in place.  -> feat [n_freq, frames] float32 CUDA."""
        import torch
        n = pcm_dev.numel()
        feat = torch.empty((self.n_freq, max(self._stream_frames(n), 1)), dtype=torch.float32, device=pcm_dev.device)
        fr = np.zeros(1, dtype=np.int32)
        self._check(lib().dsmi_features_stream(self._h, pcm_dev.data_ptr(), _pcm_code(pcm_dev.dtype), n, _np_ptr(state), feat.data_ptr(),
                                               feat.shape[1], _np_ptr(fr), _stream(self.device)))
        return feat[:, :int(fr[0])]

    def features_stream_many(self, pcms, states):
        """dsmi_features_stream_many: the next chunk of several streaming parsers in one pass.  ``pcms``: CUDA tensors of one
        dtype (one chunk per parser, each at least one window long), ``states``: their float64[3] running statistics, updated in
        place.  -> [feat [n_freq, frames_i] float32 CUDA] (views of one batch buffer), equal to ``features_stream`` one by one."""
        import torch
        n = len(pcms)
        if n == 0:
            return []
        ns = np.array([p.numel() for p in pcms], dtype=np.int64)
        pcm = torch.cat([p.reshape(-1) for p in pcms]).contiguous()
        t_stride = max(max(self._stream_frames(int(k)) for k in ns), 1)
        feat = torch.empty((n, self.n_freq, t_stride), dtype=torch.float32, device=pcm.device)
        st = np.ascontiguousarray(np.stack([np.asarray(s, dtype=np.float64).reshape(3) for s in states]))
        fr = np.zeros(n, dtype=np.int32)
        self._check(lib().dsmi_features_stream_many(self._h, pcm.data_ptr(), _pcm_code(pcms[0].dtype), _np_ptr(ns), n, _np_ptr(st),
                                                    feat.data_ptr(), t_stride, _np_ptr(fr), _stream(self.device)))
        for s_, row in zip(states, st):
            s_[:] = row
        return [feat[i, :, :int(fr[i])] for i in range(n)]


def resample_taps(rate_in, rate_out=16000):
    """dsmi_resample_taps (host only): (h[-half .. half] float64, up, down) of the polyphase filter for this rate pair."""
    up, down = C.c_int(0), C.c_int(0)
    rc = lib().dsmi_resample_taps(int(rate_in), int(rate_out), None, 0, C.byref(up), C.byref(down))
    if rc == 0:
        h = np.empty(20 * max(up.value, down.value) + 1, dtype=np.float64)
        rc = lib().dsmi_resample_taps(int(rate_in), int(rate_out), _np_ptr(h), len(h), C.byref(up), C.byref(down))
    NativeFrontend._check_thread(rc)
    return h, up.value, down.value


def resample_ready(n_in, rate_in, rate_out=16000, method="polyphase"):
    """dsmi_resample_ready (host only): how many outputs are final once the first ``n_in`` samples of an utterance are known."""
    out = lib().dsmi_resample_ready(_resample_method(method), int(rate_in), int(rate_out), int(n_in))
    if out < 0:
        raise DsmiError(DSMI_ERR_INVALID, "bad resample arguments (rate_in %r, n_in %r)" % (rate_in, n_in))
    return int(out)


class NativeResampler(_Handle):
    """Owns one dsmi_resampler handle: the sample-rate conversion of one utterance that arrives in chunks, from ``rate_in`` to
    the rate of ``frontend`` (a ``NativeFrontend``, which keeps the filters).  ``dtype``: the chunks' sample type (int16 /
    float32 / float64), or ``wav_format=(sample_width, channels)`` for raw WAV frames.  The outputs of the pushes laid end to
    end are bit for bit ``frontend.resample`` of the whole utterance."""
    _destroy, _last_error = "dsmi_resampler_destroy", "dsmi_resampler_last_error"

    def __init__(self, frontend, rate_in, method="polyphase", dtype=np.int16, wav_format=None):
        m = _resample_method(method)
        dt = _pcm_code(dtype if wav_format is None else None, wav_format)
        self.frontend, self.rate_in, self.method, self.pcm_dtype = frontend, int(rate_in), method, dt
        self.rate_out = int(frontend.desc.sample_rate)
        self.frame_bytes = _pcm_frame_bytes(dt)
        self._create("dsmi_resampler_create", frontend._h, self.rate_in, m, dt)

    def position(self):
        """(samples consumed, outputs written) since the utterance began."""
        a, b = C.c_int64(0), C.c_int64(0)
        rc = lib().dsmi_resampler_position(self._h, C.byref(a), C.byref(b))
        if rc != 0:
            raise DsmiError(rc, "dsmi_resampler_position failed")
        return a.value, b.value

    def _due(self, n_new, is_last):
        """Outputs the next push of ``n_new`` samples writes (host arithmetic, as the library does it)."""
        n_in, n_out = self.position()
        L = lib()
        m = RESAMPLE_METHODS[self.method]
        total = (L.dsmi_resample_count if is_last else L.dsmi_resample_ready)(m, self.rate_in, self.rate_out, n_in + n_new)
        return max(int(total) - n_out, 0)

    @staticmethod
    def push_many(resamplers, pcms, is_last):
        """dsmi_resampler_push_many: the next chunk of several utterances (distinct handles of one frontend) in one call.
        ``pcms[i]``: a contiguous CUDA tensor holding session i's new samples in its handle's sample type (any tensor dtype:
        the bytes are what counts; ``None`` or empty for no samples); ``is_last[i]`` flushes and ends that utterance.
        -> a list of float64 CUDA tensors (views of one buffer): what each session emits now.  Nothing is synchronised.
        Longer lists than RESAMPLE_STREAM_MAX run as several calls, after Python's own checks have passed for all of them."""
        import torch
        if not (len(pcms) == len(is_last) == len(resamplers)):
            raise ValueError("resamplers, pcms and is_last must have one entry per session")
        frames, pcms = _pushes(resamplers, pcms, "resampler", "chunk", "chunks")
        outs = []
        for rs, ps, ks, flags in _cut(RESAMPLE_STREAM_MAX, resamplers, pcms, frames, is_last):
            n, fe = len(rs), rs[0].frontend
            total = sum([r._due(k, bool(l)) for r, k, l in zip(rs, ks, flags)])
            out = torch.empty(max(total, 1), dtype=torch.float64, device="cuda:%d" % fe.device)
            ns, last, n_out = np.array(ks, dtype=np.int64), _flag_array(flags), np.zeros(n, dtype=np.int64)
            NativeResampler._check_thread(lib().dsmi_resampler_push_many(
                _handle_array(rs), n, _ptr_array(ps), _np_ptr(ns), _np_ptr(last), out.data_ptr(), total, _np_ptr(n_out), _stream(fe.device)))
            off = 0
            for k in n_out.tolist():
                outs.append(out[off:off + k])
                off += k
        return outs

    def push(self, pcm, is_last=False):
        """One chunk of this utterance -> the float64 CUDA tensor of the outputs that are final now."""
        return NativeResampler.push_many([self], [pcm], [is_last])[0]

    def reset(self):
        rc = lib().dsmi_resampler_reset(self._h)
        if rc != 0:
            raise DsmiError(rc, "dsmi_resampler_reset failed")


def endpoint_counts(chunk, rate, pause_threshold=0.8, phrase_threshold=0.3, non_speaking_duration=0.35, energy_threshold=1000, pcm_dtype=0):
    """dsmi_endpoint_counts (host only): (pause_n, phrase_n, keep_n), the gate's buffer counts for a source of ``chunk`` / ``rate``."""
    d = EndpointerDesc(int(chunk), int(rate), int(pcm_dtype), float(energy_threshold), float(pause_threshold), float(phrase_threshold),
                       float(non_speaking_duration))
    out = np.zeros(3, dtype=np.int64)
    rc = lib().dsmi_endpoint_counts(C.byref(d), _np_ptr(out))
    if rc != 0:
        raise DsmiError(rc, "bad endpointer parameters")
    return tuple(int(v) for v in out)


def endpoint_gate(energy_threshold, pause_n, phrase_n, keep_n, state, sums, lens, end_of_stream=False, max_events=None):
    """dsmi_endpoint_gate (host only): one session's gate over a run of buffers given by their sums of squares and sample counts.
    ``state``: int64[4], updated in place.  -> (events int64 [k, 3] of (first_buffer, n_buffers, last), energies uint32[n])."""
    sums = np.ascontiguousarray(sums, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.int64)
    n = len(sums)
    if len(lens) != n or state.dtype != np.int64 or len(state) != 4:
        raise ValueError("sums and lens must have one entry per buffer; state is int64[4]")
    cap = n + 1 if max_events is None else int(max_events)
    first = np.zeros(max(cap, 1), dtype=np.int64); count = np.zeros(max(cap, 1), dtype=np.int64); last = np.zeros(max(cap, 1), dtype=np.int32)
    e = np.zeros(max(n, 1), dtype=np.uint32)
    k = lib().dsmi_endpoint_gate(float(energy_threshold), int(pause_n), int(phrase_n), int(keep_n), _np_ptr(state), _np_ptr(sums), _np_ptr(lens),
                                 n, int(bool(end_of_stream)), _np_ptr(first), _np_ptr(count), _np_ptr(last), cap, _np_ptr(e))
    if k < 0:
        raise DsmiError(int(k), "bad gate arguments")
    if k > cap:
        raise DsmiError(DSMI_ERR_CAPACITY, "%d events, room for %d" % (k, cap))
    return np.stack([first[:k], count[:k], last[:k].astype(np.int64)], axis=1), e[:n]


class NativeEndpointer(_Handle):
    """Owns one dsmi_endpointer handle: the energy gate of ``Recognizer.listen_stream`` over one continuous stream that arrives in
    pushes of any size.  ``dtype``: the pushes' sample type (int16 / float32 / float64), ``channels=2`` for interleaved int16
    frames.  However the stream is cut into pushes, the segments laid end to end and the last marks are those of one push."""
    _destroy, _last_error = "dsmi_endpointer_destroy", "dsmi_endpointer_last_error"

    def __init__(self, frontend, chunk=1024, rate=16000, energy_threshold=1000, pause_threshold=0.8, phrase_threshold=0.3,
                 non_speaking_duration=0.35, dtype=np.int16, channels=1, pcm_dtype=None):
        if pcm_dtype is None:
            pcm_dtype = _pcm_code(dtype) | (PCM_STEREO if channels == 2 else 0)
        self.frontend, self.chunk, self.rate, self.pcm_dtype = frontend, int(chunk), int(rate), int(pcm_dtype)
        d = EndpointerDesc(self.chunk, self.rate, self.pcm_dtype, float(energy_threshold), float(pause_threshold), float(phrase_threshold),
                           float(non_speaking_duration))
        self._create("dsmi_endpointer_create", frontend._h, C.byref(d))      # (refuses a code that is no DSMI_PCM_*)
        self.frame_bytes = _pcm_frame_bytes(self.pcm_dtype)
        self._ended = False

    def position(self):
        """(samples consumed since the stream began, utterances closed, samples held on the device)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        rc = lib().dsmi_endpointer_position(self._h, C.byref(a), C.byref(b), C.byref(c))
        if rc != 0:
            raise DsmiError(rc, "dsmi_endpointer_position failed")
        return a.value, b.value, c.value

    @staticmethod
    def push_many(endpointers, pcms, end_of_stream, return_energies=False):
        """dsmi_endpointer_push_many: the next samples of several streams (distinct handles of one frontend) in one call.
        ``pcms[i]``: a contiguous CUDA tensor in the handle's sample type (``None`` or empty for no samples);
        ``end_of_stream[i]`` ends that stream after them.  -> a list, per session, of its segments ``(float64 CUDA tensor, last)``
        in order (views of one buffer) -- and, with ``return_energies``, a list of uint32 arrays: the energy of every buffer the
        session gated in this call.  One host synchronisation.  Longer lists than ENDPOINT_MAX run as several calls, after
        everything that could refuse one of them has been looked for in all of them."""
        import torch
        if not (len(pcms) == len(end_of_stream) == len(endpointers)):
            raise ValueError("endpointers, pcms and end_of_stream must have one entry per session")
        frames, pcms = _pushes(endpointers, pcms, "endpointer", "push", "pushes")
        if len(endpointers) > ENDPOINT_MAX:
            # what the library refuses before it touches a handle, it refuses for the handles of ONE call: with several calls to
            # make, it is looked for in all of them first
            if len(set(id(e) for e in endpointers)) != len(endpointers):
                raise ValueError("an endpointer appears twice")
            for i, e in enumerate(endpointers):
                if e.frontend is not endpointers[0].frontend:
                    raise ValueError("session %d: the endpointer belongs to another frontend" % i)
                if frames[i] > 0 and e._ended:
                    raise ValueError("session %d: samples after end_of_stream: reset the session first" % i)
        all_segs, all_energies = [], []
        for es, ps, ks, flags in _cut(ENDPOINT_MAX, endpointers, pcms, frames, end_of_stream):
            n, fe = len(es), es[0].frontend
            # (a stream that has ended gates nothing more until it is reset)
            ends = [int(bool(v) and not e._ended) for e, v in zip(es, flags)]
            # the worst case the library sizes: all a session holds and is given, one segment per gated buffer and one more
            nb, cap_out = [], 0
            for e, k, end in zip(es, ks, ends):
                n_in, _, held = e.position()
                total = n_in + k
                nb.append(total // e.chunk - n_in // e.chunk + (1 if end and total % e.chunk else 0))
                cap_out += held + k
            n_gated = sum(nb)
            cap_seg = n_gated + n
            out = torch.empty(max(cap_out, 1), dtype=torch.float64, device="cuda:%d" % fe.device)
            ns, eos = np.array(ks, dtype=np.int64), np.array(ends, dtype=np.int32)
            seg_session = np.zeros(cap_seg, dtype=np.int32); seg_len = np.zeros(cap_seg, dtype=np.int64); seg_last = np.zeros(cap_seg, dtype=np.int32)
            energies = np.zeros(max(n_gated, 1), dtype=np.uint32)
            found = C.c_int(0)
            NativeEndpointer._check_thread(lib().dsmi_endpointer_push_many(
                _handle_array(es), n, _ptr_array(ps), _np_ptr(ns), _np_ptr(eos), out.data_ptr(), cap_out, _np_ptr(seg_session), _np_ptr(seg_len),
                _np_ptr(seg_last), cap_seg, C.byref(found), _np_ptr(energies), _stream(fe.device)))
            for e, end in zip(es, ends):
                e._ended = e._ended or bool(end)
            segs = [[] for _ in range(n)]
            off, k = 0, found.value
            for i, length, last in zip(seg_session[:k].tolist(), seg_len[:k].tolist(), seg_last[:k].tolist()):
                segs[i].append((out[off:off + length], bool(last)))
                off += length
            all_segs += segs
            if return_energies:
                off = 0
                for k in nb:
                    all_energies.append(energies[off:off + k].copy())
                    off += k
        return (all_segs, all_energies) if return_energies else all_segs

    def push(self, pcm, end_of_stream=False, return_energies=False):
        """One push of this stream -> its segments [(float64 CUDA tensor, last), ...]."""
        r = NativeEndpointer.push_many([self], [pcm], [end_of_stream], return_energies)
        return (r[0][0], r[1][0]) if return_energies else r[0]

    def reset(self):
        rc = lib().dsmi_endpointer_reset(self._h)
        if rc != 0:
            raise DsmiError(rc, "dsmi_endpointer_reset failed")
        self._ended = False


class NativeStream(_Handle):
    """Owns one dsmi_stream handle: the carried state of one utterance streamed through a unidirectional model."""
    _destroy, _last_error = "dsmi_stream_destroy", "dsmi_stream_last_error"

    def __init__(self, model):
        self.model = model
        self._create("dsmi_stream_create", model._h)

    def forward(self, feat, is_first, is_last):
        """feat: CUDA float32 [F,T] (or [1,1,F,T]) -> probs [1,T_out,C] CUDA, or None while the lookahead buffers."""
        import torch
        feat = feat.reshape(feat.shape[-2], feat.shape[-1]).contiguous()
        assert feat.is_cuda and feat.dtype == torch.float32
        T = feat.shape[1]
        cap = T + 4 * int(self.model.desc.context) + 2048 if not hasattr(self, "_cap") else self._cap
        while True:
            probs = torch.empty((cap, self.model.n_labels), dtype=torch.float32, device=feat.device)
            tout = np.zeros(1, dtype=np.int32)
            rc = lib().dsmi_stream_forward(self._h, feat.data_ptr(), T, int(bool(is_first)), int(bool(is_last)),
                                           probs.data_ptr(), cap, _np_ptr(tout), _stream(self.model.device))
            if rc == DSMI_ERR_CAPACITY and cap < (1 << 24):
                # nothing was consumed: the capacity check precedes every state update of the lookahead
                cap *= 4
                continue
            self._check(rc)
            break
        n = int(tout[0])
        return probs[:n].unsqueeze(0) if n > 0 else None

    @staticmethod
    def forward_many(streams, feats, is_first, is_last):
        """dsmi_stream_forward_many: advance several sessions (distinct ``NativeStream`` of one model) by one chunk each in
        one batched pass.  ``feats[i]``: CUDA float32 [F,T_i] (or [1,1,F,T_i]); ``is_first`` / ``is_last``: one flag per
        session.  -> a list of probs [1,T_out,C] CUDA, or None for a session whose lookahead is still buffering, each equal to
        what ``forward`` returns for that session alone.  Longer lists than STREAM_MANY_MAX run as several passes."""
        import torch
        if not (len(feats) == len(is_first) == len(is_last) == len(streams)):
            raise ValueError("streams, feats, is_first and is_last must have one entry per session")
        feats = [f.reshape(f.shape[-2], f.shape[-1]).contiguous() for f in feats]
        for f in feats:
            assert f.is_cuda and f.dtype == torch.float32
        outs = []
        for ss, fs, firsts, lasts in _cut(STREAM_MANY_MAX, streams, feats, is_first, is_last):
            n, model = len(ss), ss[0].model
            T = np.array([f.shape[1] for f in fs], dtype=np.int32)
            hs, fp, first, last = _handle_array(ss), _ptr_array(fs), _flag_array(firsts), _flag_array(lasts)
            cap = int(T.max()) + 4 * int(model.desc.context) + 2048
            while True:
                probs = torch.empty((n, cap, model.n_labels), dtype=torch.float32, device=fs[0].device)
                tout = np.zeros(n, dtype=np.int32)
                rc = lib().dsmi_stream_forward_many(hs, n, fp, _np_ptr(T), _np_ptr(first), _np_ptr(last), probs.data_ptr(), cap,
                                                    _np_ptr(tout), _stream(model.device))
                if rc == DSMI_ERR_CAPACITY and cap < (1 << 24):
                    cap *= 4               # refused before any state changed
                    continue
                NativeStream._check_thread(rc)
                break
            outs += [probs[i, :int(tout[i])].unsqueeze(0) if tout[i] > 0 else None for i in range(n)]
        return outs

    def reset(self):
        self._check(lib().dsmi_stream_reset(self._h))


def _sizes_ptr(sizes):
    """Optional int32 sizes -> what a native call takes for them."""
    return None if sizes is None else _np_ptr(np.ascontiguousarray(sizes, dtype=np.int32))


def _greedy_arrays(B, T):
    """What a greedy decode of [B,T] fills: (ids [B,T], offsets [B,T], counts [B])."""
    return np.empty((B, T), dtype=np.int32), np.empty((B, T), dtype=np.int32), np.empty(B, dtype=np.int32)


def _greedy_results(ids, offs, n):
    return [(ids[b, :n[b]].copy(), offs[b, :n[b]].copy()) for b in range(len(n))]


class NativeDecoder(_Handle):
    """Owns one dsmi_decoder handle: greedy and beam-search CTC decoding on one GPU."""
    _destroy, _last_error = "dsmi_decoder_destroy", "dsmi_decoder_last_error"

    def __init__(self, labels, blank_index=0, device=0):
        self.labels = labels
        self.device = device
        arr = (C.c_char_p * len(labels))(*[c.encode("utf-8") for c in labels])
        self._create("dsmi_decoder_create", device, arr, len(labels), int(blank_index))

    def set_lm(self, lm_path, alpha, beta):
        self._check(lib().dsmi_decoder_set_lm(self._h, lm_path.encode() if lm_path else None, float(alpha), float(beta)))

    def greedy(self, probs, sizes=None):
        """probs: CUDA [B,T,C] -> list of (ids, offsets) int32 arrays per utterance."""
        B, T = probs.shape[0], probs.shape[1]
        ids, offs, n = _greedy_arrays(B, T)
        self._check(lib().dsmi_greedy(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, _np_ptr(ids), _np_ptr(offs), _np_ptr(n),
                                      _stream(self.device)))
        return _greedy_results(ids, offs, n)

    def greedy_enqueue(self, probs, sizes=None):
        """Launch the greedy decode and the copies of its results on the current stream and return at once."""
        B, T = probs.shape[0], probs.shape[1]
        self._check(lib().dsmi_greedy_enqueue(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, _stream(self.device)))
        self._greedy_pending = (probs, B, T)                     # keeps the probabilities alive until the collect

    def greedy_collect(self):
        _, B, T = self._greedy_pending
        self._greedy_pending = None
        ids, offs, n = _greedy_arrays(B, T)
        self._check(lib().dsmi_greedy_collect(self._h, _np_ptr(ids), _np_ptr(offs), _np_ptr(n)))
        return _greedy_results(ids, offs, n)

    def beam(self, probs, sizes=None, beam_width=64, cutoff_top_n=40, cutoff_prob=1.0):
        """probs: CUDA [B,T,C] -> (tokens [B,beam,T], timesteps [B,beam,T], lens [B,beam], scores [B,beam])."""
        self.beam_enqueue(probs, sizes, beam_width, cutoff_top_n, cutoff_prob)
        return self.beam_collect()

    def beam_enqueue(self, probs, sizes=None, beam_width=64, cutoff_top_n=40, cutoff_prob=1.0):
        """Launch the search on the current stream and return at once; ``beam_collect`` waits and returns the arrays."""
        B, T = probs.shape[0], probs.shape[1]
        self._check(lib().dsmi_beam_enqueue(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, int(beam_width),
                                            int(cutoff_top_n), float(cutoff_prob), _stream(self.device)))
        self._beam_pending = (probs, B, T, int(beam_width))        # keeps the probabilities alive until the collect

    def beam_collect(self):
        _, B, T, beam_width = self._beam_pending
        self._beam_pending = None
        tok = np.zeros((B, beam_width, T), dtype=np.int32)
        ts = np.zeros((B, beam_width, T), dtype=np.int32)
        ln = np.zeros((B, beam_width), dtype=np.int32)
        sc = np.zeros((B, beam_width), dtype=np.float32)
        self._check(lib().dsmi_beam_collect(self._h, _np_ptr(tok), _np_ptr(ts), _np_ptr(ln), _np_ptr(sc)))
        return tok, ts, ln, sc

    def beam_stamps(self):
        """[64, 8] uint64: 100 MHz phase-boundary stamps of the last collected search (dsmi_debug_beam_stamps)."""
        st = np.zeros((64, 8), dtype=np.uint64)
        self._check(lib().dsmi_debug_beam_stamps(self._h, _np_ptr(st), st.size))
        return st

    def beam_stats(self):
        """Of the last collected search: {revivals, walk_hops, list_rankings, full_rankings} (dsmi_decoder_beam_stats)."""
        c = np.zeros(4, dtype=np.int32)
        self._check(lib().dsmi_decoder_beam_stats(self._h, _np_ptr(c)))
        return dict(zip(("revivals", "walk_hops", "list_rankings", "full_rankings"), (int(v) for v in c)))

    def align(self, probs, sizes, targets, target_lens=None):
        """CTC forced alignment (``dsmi_align``).  probs: CUDA [B,T,C]; sizes: [B] frames or None (= T); targets: [B, L_stride]
        int array with ``target_lens`` [B], or a list of B id sequences (``target_lens`` None).  Returns numpy arrays
        (spans int32 [B,L_stride,2], token_probs float32 [B,L_stride], path_logp float32 [B], status int32 [B]: 1 = infeasible)."""
        B, T = probs.shape[0], probs.shape[1]
        tg, target_lens = _padded_ids(targets, target_lens, B, 0, "align: %d target sequences for a batch of %d")
        Ls = tg.shape[1]
        spans = np.zeros((B, Ls, 2), dtype=np.int32)
        tp = np.zeros((B, Ls), dtype=np.float32)
        lp = np.zeros(B, dtype=np.float32)
        st = np.zeros(B, dtype=np.int32)
        self._check(lib().dsmi_align(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, _np_ptr(tg),
                                     _np_ptr(target_lens), Ls, _np_ptr(spans), _np_ptr(tp), _np_ptr(lp), _np_ptr(st),
                                     _stream(self.device)))
        return spans, tp, lp, st

    def align_long(self, probs, targets, lead_free=True, tail_free=True):
        """Long-form CTC forced alignment (``dsmi_align_long``) of one recording.  probs: CUDA [T,C], the softmax rows of the
        recording's phrases in time order; targets: the whole transcript as label ids; ``lead_free`` / ``tail_free``: the
        frames before the first and after the last token cost nothing.  Returns (spans int32 [L,2], token_probs float32 [L],
        path_logp float, status int: 1 = infeasible)."""
        if probs.dim() != 2:
            raise ValueError("align_long: probs must be [T, C]")
        T = probs.shape[0]
        tg = np.ascontiguousarray(targets, dtype=np.int32).reshape(-1)
        L = len(tg)
        spans = np.zeros((L, 2), dtype=np.int32)
        tp = np.zeros(L, dtype=np.float32)
        lp = np.zeros(1, dtype=np.float32)
        st = np.zeros(1, dtype=np.int32)
        self._check(lib().dsmi_align_long(self._h, probs.data_ptr(), T, _np_ptr(tg) if L else None, L, int(lead_free), int(tail_free),
                                          _np_ptr(spans) if L else None, _np_ptr(tp) if L else None, _np_ptr(lp), _np_ptr(st),
                                          _stream(self.device)))
        return spans, tp, float(lp[0]), int(st[0])

    def spot(self, probs, sizes, phrases, max_hits, min_mean_logp, tracks=False):
        """CTC phrase search (``dsmi_spot``): every phrase in every clip.  probs: CUDA [B,T,C]; sizes: [B] frames or None (= T);
        phrases: a list of K label-id sequences.  Returns numpy arrays (hits int32 [B,K,max_hits,2] frames [start, end), scores
        float32 [B,K,max_hits] natural-log probabilities, counts int32 [B,K]; rows past the count are 0), best hit first; with
        ``tracks`` also the end scores float32 [B,K,T] and the start frames int32 [B,K,T] behind them."""
        B, T = probs.shape[0], probs.shape[1]
        ph, lens = _padded_ids(phrases, None, None, 1, None)
        K, M = len(lens), int(max_hits)
        rows = max(M, 0)
        hits = np.zeros((B, K, rows, 2), dtype=np.int32)
        scores = np.zeros((B, K, rows), dtype=np.float32)
        counts = np.zeros((B, K), dtype=np.int32)
        E = np.zeros((B, K, T), dtype=np.float32) if tracks else None
        ST = np.zeros((B, K, T), dtype=np.int32) if tracks else None
        self._check(lib().dsmi_spot(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, _np_ptr(ph), _np_ptr(lens), K, ph.shape[1],
                                    M, float(min_mean_logp), _np_ptr(hits), _np_ptr(scores), _np_ptr(counts),
                                    _np_ptr(E) if tracks else None, _np_ptr(ST) if tracks else None, _stream(self.device)))
        return (hits, scores, counts, E, ST) if tracks else (hits, scores, counts)

    def score(self, probs, sizes, cand_clip, targets, target_lens=None):
        """CTC transcript scoring (``dsmi_score``): the exact float64 log likelihood of candidate transcripts, summed over
        every alignment.  probs: CUDA [B,T,C]; sizes: [B] frames or None (= T); cand_clip: [N] the clip of each candidate;
        targets: [N, L_stride] int array with ``target_lens`` [N], or a list of N id sequences (``target_lens`` None).
        Returns numpy arrays (logp float64 [N], status int32 [N]: 1 = infeasible, logp = -inf)."""
        B, T = probs.shape[0], probs.shape[1]
        clip = np.ascontiguousarray(cand_clip, dtype=np.int32).reshape(-1)
        N = len(clip)
        tg, target_lens = _padded_ids(targets, target_lens, N, 0, "score: %d target sequences for %d candidates")
        lp = np.zeros(N, dtype=np.float64)
        st = np.zeros(N, dtype=np.int32)
        self._check(lib().dsmi_score(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, _np_ptr(clip), _np_ptr(tg),
                                     _np_ptr(target_lens), N, tg.shape[1], _np_ptr(lp), _np_ptr(st), _stream(self.device)))
        return lp, st

    def alternatives(self, probs, sizes, cand_clip, targets, target_lens=None):
        """CTC token confidence (``dsmi_alternatives``): for every token of every candidate, the exact float64 log likelihood
        of the candidate with that token replaced by each label, or deleted (the blank's column).  Arguments as ``score``.
        Returns numpy arrays (logp float64 [N], alt float64 [N, L_stride, C], status int32 [N]: 1 = infeasible, all -inf);
        rows past a candidate's length are -inf."""
        B, T = probs.shape[0], probs.shape[1]
        clip = np.ascontiguousarray(cand_clip, dtype=np.int32).reshape(-1)
        N = len(clip)
        tg, target_lens = _padded_ids(targets, target_lens, N, 0, "alternatives: %d target sequences for %d candidates")
        lp = np.zeros(N, dtype=np.float64)
        alt = np.zeros((N, tg.shape[1], probs.shape[2]), dtype=np.float64)
        st = np.zeros(N, dtype=np.int32)
        self._check(lib().dsmi_alternatives(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, _np_ptr(clip), _np_ptr(tg),
                                            _np_ptr(target_lens), N, tg.shape[1], _np_ptr(lp), _np_ptr(alt), _np_ptr(st),
                                            _stream(self.device)))
        return lp, alt, st

    def occupancy(self, probs, sizes, cand_clip, targets, target_lens=None, want_occ=True, want_tok=True):
        """CTC occupancy (``dsmi_occupancy``): for every candidate the posterior, given the transcript, that frame t carries
        label c (``occ``) or is emitted by token k (``tok``).  Arguments as ``score``.  Returns ``(logp, occ, tok, status)``:
        logp float64 [N] and status int32 [N] (1 = infeasible, logp = -inf) are numpy; occ [N, T, C] and tok [N, T, L_stride]
        are CUDA float64 tensors written in full (zeros past a clip's frames, past a transcript's length and for an
        infeasible candidate), or None where ``want_occ`` / ``want_tok`` is false."""
        import torch
        B, T = probs.shape[0], probs.shape[1]
        clip = np.ascontiguousarray(cand_clip, dtype=np.int32).reshape(-1)
        N = len(clip)
        tg, target_lens = _padded_ids(targets, target_lens, N, 0, "occupancy: %d target sequences for %d candidates")
        lp = np.zeros(N, dtype=np.float64)
        st = np.zeros(N, dtype=np.int32)
        occ = torch.empty((N, T, probs.shape[2]), dtype=torch.float64, device=probs.device) if want_occ else None
        tok = torch.empty((N, T, tg.shape[1]), dtype=torch.float64, device=probs.device) if want_tok else None
        self._check(lib().dsmi_occupancy(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, _np_ptr(clip), _np_ptr(tg),
                                         _np_ptr(target_lens), N, tg.shape[1], _np_ptr(lp), occ.data_ptr() if want_occ else None,
                                         tok.data_ptr() if want_tok and tok.numel() else None, _np_ptr(st), _stream(self.device)))
        return lp, occ, tok, st

    def grammar(self, probs, sizes, graphs, clip_graph=None):
        """CTC grammar decoding (``dsmi_grammar``): the best CTC path of any sentence a token graph accepts.  probs: CUDA
        [B,T,C]; sizes: [B] frames or None (= T); graphs: one graph or a list of K -- a ``grammar.Grammar`` or anything with its
        arrays ``labels``, ``weights``, ``flags``, ``arc_off``, ``arc_pred`` and ``empty_ok``; clip_graph: [B] the graph of each
        clip or None (= graph 0).  Returns numpy arrays (path_lens int32 [B], path_nodes int32 [B,T], path_spans int32 [B,T,2],
        token_probs float32 [B,T], path_logp float32 [B], status int32 [B]: 1 = no accepted sentence fits)."""
        B, T = probs.shape[0], probs.shape[1]
        pool, keep = grammar_pool(graphs)
        cg = None if clip_graph is None else np.ascontiguousarray(clip_graph, dtype=np.int32).reshape(-1)
        if cg is not None and len(cg) != B:
            raise ValueError("grammar: %d graph indices for a batch of %d" % (len(cg), B))
        lens = np.zeros(B, dtype=np.int32)
        nodes = np.zeros((B, T), dtype=np.int32)
        spans = np.zeros((B, T, 2), dtype=np.int32)
        tp = np.zeros((B, T), dtype=np.float32)
        lp = np.zeros(B, dtype=np.float32)
        st = np.zeros(B, dtype=np.int32)
        self._check(lib().dsmi_grammar(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, C.byref(pool), None if cg is None else _np_ptr(cg),
                                       _np_ptr(lens), _np_ptr(nodes), _np_ptr(spans), _np_ptr(tp), _np_ptr(lp), _np_ptr(st),
                                       _stream(self.device)))
        del keep
        return lens, nodes, spans, tp, lp, st

    def grammar_posterior(self, probs, sizes, graphs, clip_graph=None, want_visits=True, want_occ=True):
        """CTC grammar posterior (``dsmi_grammar_posterior``): the summed probability of every path a token graph accepts.
        Arguments as ``grammar``.  Returns ``(logp, visits, occ, status)``: logp float64 [B] and status int32 [B] (1 = no
        accepted sentence fits, logp = -inf) are numpy; visits float64 [B, N] numpy (N the most nodes of a graph: each node's
        expected number of entries, zeros past a graph's nodes) and occ [B, T, C] a CUDA float64 tensor written in full (the
        per-frame label posteriors given the grammar), or None where ``want_visits`` / ``want_occ`` is false."""
        import torch
        B, T = probs.shape[0], probs.shape[1]
        pool, keep = grammar_pool(graphs)
        cg = None if clip_graph is None else np.ascontiguousarray(clip_graph, dtype=np.int32).reshape(-1)
        if cg is not None and len(cg) != B:
            raise ValueError("grammar: %d graph indices for a batch of %d" % (len(cg), B))
        N = int(np.diff(keep[0]).max()) if pool.K else 0
        lp = np.zeros(B, dtype=np.float64)
        st = np.zeros(B, dtype=np.int32)
        visits = np.zeros((B, N), dtype=np.float64) if want_visits else None
        occ = torch.empty((B, T, probs.shape[2]), dtype=torch.float64, device=probs.device) if want_occ else None
        self._check(lib().dsmi_grammar_posterior(self._h, probs.data_ptr(), _sizes_ptr(sizes), B, T, C.byref(pool),
                                                 None if cg is None else _np_ptr(cg), N, _np_ptr(lp),
                                                 _np_ptr(visits) if want_visits and visits.size else None,
                                                 occ.data_ptr() if want_occ else None, _np_ptr(st), _stream(self.device)))
        del keep
        return lp, visits, occ, st

    def edit_distance(self, seqs, pairs, seq_lens=None):
        """Batched edit distance (``dsmi_edit_distance``).  seqs: the pool, an int array [M, L_stride] with ``seq_lens`` [M],
        or a list of M id sequences (``seq_lens`` None); tokens are any int32.  pairs: int [N, 2], row n = (a, b) compares
        pool sequence a (the reference) with pool sequence b (the hypothesis).  Returns int32 [N, 4]: distance,
        substitutions, deletions, insertions of the minimum-distance alignment with the fewest substitutions."""
        if seq_lens is not None and np.size(seqs) == 0:        # (a pool of empty sequences: no column to infer the rows from)
            pool, seq_lens = np.zeros((len(seq_lens), 0), dtype=np.int32), np.ascontiguousarray(seq_lens, dtype=np.int32)
        else:
            pool, seq_lens = _padded_ids(seqs, seq_lens, None if seq_lens is None else len(seq_lens), 0, None)
        pr =np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        pa, pb = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        counts = np.zeros((len(pr), 4), dtype=np.int32)
        self._check(lib().dsmi_edit_distance(self._h, _np_ptr(pool) if pool.size else None, _np_ptr(seq_lens), pool.shape[0], pool.shape[1],
                                             _np_ptr(pa), _np_ptr(pb), len(pr), _np_ptr(counts), _stream(self.device)))
        return counts

    def lm_score(self, ids, lens=None, want_terms=False):
        """LM sentence scoring (``dsmi_lm_score``) with the language model of ``set_lm``.  ids: the pool, an int array
        [M, L_stride] of label ids with ``lens`` [M], or a list of M id sequences (``lens`` None).  Returns numpy arrays
        (lm_ln float64 [M] natural log, n_words int32 [M], n_oov int32 [M]) and, with ``want_terms``, a list of M float64
        arrays: the n_words + 1 window terms of each sentence (2 for no words), whose sum in order is lm_ln."""
        if lens is not None and np.size(ids) == 0:             # (a pool of empty sequences: no column to infer the rows from)
            pool, lens = np.zeros((len(lens), 0), dtype=np.int32), np.ascontiguousarray(lens, dtype=np.int32)
        else:
            pool, lens = _padded_ids(ids, lens, None if lens is None else len(lens), 0, None)
        M = pool.shape[0]
        W = pool.shape[1] // 2 + 2 if want_terms else 0       # words are at least a space apart: n_terms <= L_stride // 2 + 2
        lm_ln = np.zeros(M, dtype=np.float64)
        n_words, n_oov, n_terms = (np.zeros(M, dtype=np.int32) for _ in range(3))
        terms = np.zeros((M, W), dtype=np.float64) if want_terms else None
        self._check(lib().dsmi_lm_score(self._h, _np_ptr(pool) if pool.size else None, _np_ptr(lens), M, pool.shape[1], _np_ptr(lm_ln),
                                        _np_ptr(n_words), _np_ptr(n_oov), _np_ptr(n_terms), _np_ptr(terms) if want_terms else None, W,
                                        _stream(self.device)))
        if want_terms:
            return lm_ln, n_words, n_oov, [terms[m, :n_terms[m]].copy() for m in range(M)]
        return lm_ln, n_words, n_oov


def lm_score_plan(ids, lens=None, space=-2):
    """dsmi_lm_score_plan (host only): the words dsmi_lm_score finds in rows of label ids -- (n_words int32 [M], word_first
    int32 [M, W], word_len int32 [M, W]) with ``space`` the space label's id and W the largest n_words."""
    if lens is not None and np.size(ids) == 0:
        pool, lens = np.zeros((len(lens), 0), dtype=np.int32), np.ascontiguousarray(lens, dtype=np.int32)
    else:
        pool, lens = _padded_ids(ids, lens, None if lens is None else len(lens), 0, None)
    M, W = pool.shape[0], (pool.shape[1] + 1) // 2
    n_words = np.zeros(M, dtype=np.int32)
    first, length = np.zeros((M, W), dtype=np.int32), np.zeros((M, W), dtype=np.int32)
    rc = lib().dsmi_lm_score_plan(_np_ptr(pool) if pool.size else None, _np_ptr(lens), M, pool.shape[1], int(space), _np_ptr(n_words),
                                  _np_ptr(first) if W else None, _np_ptr(length) if W else None, W)
    if rc < 0:
        raise DsmiError(rc, "dsmi_lm_score_plan: at least one row, every length within 0 .. L_stride")
    return n_words, first[:, :rc].copy(), length[:, :rc].copy()


def _padded_ids(rows, lens, count, min_width, mismatch):
    """The token rows of dsmi_align / dsmi_spot / dsmi_score as a contiguous int32 [count, L_stride] array and its int32 lens:
    from an array with ``lens``, or (``lens`` None) from a list of ``count`` id sequences (None: as many as there are),
    zero-padded to the longest (at least ``min_width`` columns).  ``mismatch`` is the ValueError's text for another number of
    sequences (% (given, count))."""
    if lens is not None:
        return (np.ascontiguousarray(rows, dtype=np.int32).reshape(count, -1), np.ascontiguousarray(lens, dtype=np.int32))
    seqs = [np.asarray(t, dtype=np.int32).reshape(-1) for t in rows]
    if count is None:
        count = len(seqs)
    if len(seqs) != count:
        raise ValueError(mismatch % (len(seqs), count))
    lens = np.array([len(t) for t in seqs], dtype=np.int32)
    ids = np.zeros((count, max(min_width, int(lens.max()) if count else 0)), dtype=np.int32)
    for i, t in enumerate(seqs):
        ids[i, :len(t)] = t
    return ids, lens


def grammar_pool(graphs):
    """The dsmi_grammar_pool of one graph or a list of graphs (objects with the arrays ``labels``, ``weights`` (or None),
    ``flags``, ``arc_off``, ``arc_pred`` and the flag ``empty_ok``): (the ctypes structure, the arrays it points into -- keep them
    alive for as long as the structure is used)."""
    if hasattr(graphs, "arc_off"):
        graphs = [graphs]
    graphs = list(graphs)
    i32 = lambda rows: np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.int32).reshape(-1) for r in rows]) if rows else [], dtype=np.int32)
    node_off = np.zeros(len(graphs) + 1, dtype=np.int32)
    node_off[1:] = np.cumsum([len(g.labels) for g in graphs])
    labels, flags = i32([g.labels for g in graphs]), i32([g.flags for g in graphs])
    arc_pred = i32([g.arc_pred for g in graphs])
    arc_off, base = [np.zeros(1, dtype=np.int32)], 0
    for g in graphs:
        off = np.asarray(g.arc_off, dtype=np.int64).reshape(-1)
        if len(off) != len(g.labels) + 1:
            raise ValueError("grammar: arc_off must have one entry more than there are nodes")
        arc_off.append((off[1:] + base).astype(np.int32))
        base += int(off[-1])
    arc_off = np.ascontiguousarray(np.concatenate(arc_off), dtype=np.int32)
    weights = None
    if any(getattr(g, "weights", None) is not None for g in graphs):
        weights = np.ascontiguousarray(np.concatenate([np.zeros(len(g.labels), dtype=np.float32) if getattr(g, "weights", None) is None
                                                       else np.asarray(g.weights, dtype=np.float32).reshape(-1) for g in graphs]), dtype=np.float32)
    empty_ok = np.array([1 if g.empty_ok else 0 for g in graphs], dtype=np.int32)
    keep = (node_off, labels, weights, flags, arc_off, arc_pred, empty_ok)
    ptr = lambda a: None if a is None else a.ctypes.data
    pool = GrammarPool(len(graphs), ptr(node_off), ptr(labels), ptr(weights), ptr(flags), ptr(arc_off), ptr(arc_pred), ptr(empty_ok))
    return pool, keep


def grammar_plan(B, T_out, n_nodes, n_arcs):
    """dsmi_grammar_plan (host only): the geometry of a dsmi_grammar call of B clips of T_out frames whose largest graph has
    n_nodes nodes and n_arcs arcs, as a dict; DsmiError with the code dsmi_grammar would refuse these numbers with."""
    info = np.zeros(3, dtype=np.int64)
    rc = lib().dsmi_grammar_plan(int(B), int(T_out), int(n_nodes), int(n_arcs), info.ctypes.data_as(_i64p))
    if rc < 0:
        raise DsmiError(rc, "dsmi_grammar_plan: B and T_out positive, 0 .. %d nodes, 0 .. %d arcs, at most 2^31 bytes of backpointers"
                        % (GRAMMAR_MAX_NODES, GRAMMAR_MAX_ARCS))
    return dict(zip(("node_stride", "lds_bytes", "bp_bytes"), (int(v) for v in info)))


def grammar_posterior_plan(B, T_out, n_nodes, n_arcs):
    """dsmi_grammar_posterior_plan (host only): the geometry of a dsmi_grammar_posterior call of B clips of T_out frames whose
    largest graph has n_nodes nodes and n_arcs arcs, as a dict; DsmiError with the code the call would refuse these numbers with."""
    info = np.zeros(3, dtype=np.int64)
    rc = lib().dsmi_grammar_posterior_plan(int(B), int(T_out), int(n_nodes), int(n_arcs), info.ctypes.data_as(_i64p))
    if rc < 0:
        raise DsmiError(rc, "dsmi_grammar_posterior_plan: B and T_out positive, 0 .. %d nodes, 0 .. %d arcs, at most 2^30 bytes of stored trellises"
                        % (GRAMMAR_MAX_NODES, GRAMMAR_MAX_ARCS))
    return dict(zip(("node_stride", "lds_bytes", "ws_bytes"), (int(v) for v in info)))


def grammar_stream_plan(n_nodes, n_arcs, n_labels, max_frames):
    """dsmi_grammar_stream_plan (host only): the geometry of one dsmi_grammar_stream over a graph of n_nodes nodes and n_arcs arcs
    with n_labels labels and room for max_frames frames, as a dict; DsmiError with the code a create would refuse these numbers with."""
    info = np.zeros(3, dtype=np.int64)
    rc = lib().dsmi_grammar_stream_plan(int(n_nodes), int(n_arcs), int(n_labels), int(max_frames), info.ctypes.data_as(_i64p))
    if rc < 0:
        raise DsmiError(rc, "dsmi_grammar_stream_plan: 1 .. %d frames, 0 .. %d nodes, 0 .. %d arcs, 1 .. 128 labels, at most 2^31 bytes"
                        % (GRAMMAR_STREAM_MAX_FRAMES, GRAMMAR_MAX_NODES, GRAMMAR_MAX_ARCS))
    return dict(zip(("node_stride", "lds_bytes", "block_bytes"), (int(v) for v in info)))


def spot_plan(phrase_lens):
    """dsmi_spot_plan (host only): (n_groups, group_of, first_state) of phrases with these token counts, as dsmi_spot packs them."""
    lens = np.ascontiguousarray(phrase_lens, dtype=np.int32).reshape(-1)
    group_of = np.zeros(len(lens), dtype=np.int32)
    first_state = np.zeros(len(lens), dtype=np.int32)
    rc = lib().dsmi_spot_plan(_np_ptr(lens) if len(lens) else None, len(lens), _np_ptr(group_of), _np_ptr(first_state))
    if rc < 0:
        raise DsmiError(rc, "dsmi_spot_plan: 1 .. %d phrases of 1 .. %d tokens" % (SPOT_MAX_PHRASES, SPOT_MAX_TOKENS))
    return rc, group_of, first_state


def align_long_plan(T, L):
    """dsmi_align_long_plan (host only): the geometry dsmi_align_long uses for T frames and L tokens, as a dict."""
    info = np.zeros(6, dtype=np.int64)
    rc = lib().dsmi_align_long_plan(int(T), int(L), info.ctypes.data_as(_i64p))
    if rc < 0:
        raise DsmiError(rc, "dsmi_align_long_plan: 1 .. %d frames, 0 .. %d tokens, checkpoint rows of at most 4 GiB"
                        % (ALIGN_LONG_MAX_FRAMES, ALIGN_LONG_MAX_TOKENS))
    return dict(zip(("W", "F", "state_tiles", "frame_tiles", "rows", "bytes"), (int(v) for v in info)))


def score_plan(cand_clip, cand_frames, target_lens):
    """dsmi_score_plan (host only): the order in which dsmi_score launches candidates with these clips, frames of their clips
    and token counts -- order[i] = the candidate of workgroup i."""
    clip = np.ascontiguousarray(cand_clip, dtype=np.int32).reshape(-1)
    frames = np.ascontiguousarray(cand_frames, dtype=np.int32).reshape(-1)
    lens = np.ascontiguousarray(target_lens, dtype=np.int32).reshape(-1)
    if not (len(clip) == len(frames) == len(lens)):
        raise ValueError("score_plan: one clip, frame count and token count per candidate")
    order = np.zeros(len(clip), dtype=np.int32)
    rc = lib().dsmi_score_plan(_np_ptr(clip), _np_ptr(frames), _np_ptr(lens), len(clip), _np_ptr(order))
    if rc < 0:
        raise DsmiError(rc, "dsmi_score_plan: at least one candidate, no negative entry")
    return order


def edit_plan(len_a, len_b):
    """dsmi_edit_plan (host only): (order, seg) for pairs of these token counts -- seg[n] the lane segment (16, 32 or 64) of
    pair n, order the launch order of the pairs with both lengths > 0, as dsmi_edit_distance launches them."""
    la = np.ascontiguousarray(len_a, dtype=np.int32).reshape(-1)
    lb = np.ascontiguousarray(len_b, dtype=np.int32).reshape(-1)
    if len(la) != len(lb):
        raise ValueError("edit_plan: one length of a and one of b per pair")
    order = np.zeros(len(la), dtype=np.int32)
    seg = np.zeros(len(la), dtype=np.int32)
    rc = lib().dsmi_edit_plan(_np_ptr(la), _np_ptr(lb), len(la), _np_ptr(order), _np_ptr(seg))
    if rc < 0:
        raise DsmiError(rc, "dsmi_edit_plan: at least one pair, no negative length")
    return order[:rc].copy(), seg


class NativeBeamStream(_Handle):
    """Owns one dsmi_beam_stream handle: one utterance's beam search carried from chunk to chunk, with the language model,
    alpha and beta of ``decoder`` (a ``NativeDecoder``, kept alive by the stream)."""
    _destroy, _last_error = "dsmi_beam_stream_destroy", "dsmi_beam_stream_last_error"

    def __init__(self, decoder, beam_width=64, cutoff_top_n=40, cutoff_prob=1.0):
        self.decoder = decoder
        self.beam_width = int(beam_width)
        self._create("dsmi_beam_stream_create", decoder._h, self.beam_width, int(cutoff_top_n), float(cutoff_prob))

    @property
    def frames(self):
        f = C.c_int64()
        if lib().dsmi_beam_stream_frames(self._h, C.byref(f)) != 0:
            raise DsmiError(DSMI_ERR_INVALID, "closed beam stream")
        return int(f.value)

    @staticmethod
    def advance_many(streams, probs_list, n_best=0):
        """dsmi_beam_stream_advance_many: advance distinct ``NativeBeamStream`` of one decoder in one launch, stream i by the
        frames of ``probs_list[i]`` (CUDA float32 [T,C] or [1,T,C]; None or T = 0: no frames).  n_best = 0 -> None; else a
        list with, per stream, (tokens [n_best,T], timesteps [n_best,T], lens [n_best], scores [n_best]) over all its frames so
        far, T = its frame count: what ``NativeDecoder.beam`` returns first for the concatenated probabilities.  Longer lists
        than BEAM_STREAM_MANY_MAX run as several launches."""
        import torch
        if len(probs_list) != len(streams):
            raise ValueError("streams and probs_list must have one entry per stream")
        probs, new = [], []
        for p in probs_list:
            t = 0
            if p is not None:
                t = p.shape[-2]
                p = p.reshape(t, p.shape[-1]).contiguous()
                assert p.is_cuda and p.dtype == torch.float32
            probs.append(p if t > 0 else None)
            new.append(t)
        outs = []
        for ss, ps, ts in _cut(BEAM_STREAM_MANY_MAX, streams, probs, new):
            n, hs = len(ss), _handle_array(ss)
            fr = np.array(ts, dtype=np.int32)
            NativeBeamStream._check_thread(lib().dsmi_beam_stream_advance_many(hs, n, _ptr_array(ps), _np_ptr(fr), int(n_best),
                                                                               _stream(ss[0].decoder.device)))
            if not n_best:
                continue
            frames = [max(1, s.frames) for s in ss]
            T = max(frames)
            tok = np.zeros((n, n_best, T), dtype=np.int32)
            ts = np.zeros((n, n_best, T), dtype=np.int32)
            ln = np.zeros((n, n_best), dtype=np.int32)
            sc = np.zeros((n, n_best), dtype=np.float32)
            cnt = np.zeros(n, dtype=np.int32)
            NativeBeamStream._check_thread(lib().dsmi_beam_stream_collect_many(hs, n, int(n_best), T, _np_ptr(tok), _np_ptr(ts), _np_ptr(ln),
                                                                               _np_ptr(sc), _np_ptr(cnt)))
            outs += [(tok[i, :, :t], ts[i, :, :t], ln[i], sc[i]) for i, t in enumerate(frames)]
        return outs if n_best else None

    def advance(self, probs, n_best=0):
        r = NativeBeamStream.advance_many([self], [probs], n_best)
        return None if r is None else r[0]

    def reset(self):
        if lib().dsmi_beam_stream_reset(self._h) != 0:
            raise DsmiError(DSMI_ERR_INVALID, "closed beam stream")


class SpotPickState(C.Structure):
    """dsmi_spot_pick_state: the online picking rule's state of one (stream, phrase); ``SpotPickState.fresh()`` starts an utterance."""
    _fields_ = [("pending", C.c_int32), ("ps", C.c_int32), ("pe", C.c_int32), ("last_end", C.c_int32), ("pv", C.c_float)]

    @classmethod
    def fresh(cls):
        return cls(0, 0, 0, -1, 0.0)


def spot_watch_pick(E, ST, t0, flush, min_mean_logp, settle_frames, state, max_events=SPOT_MAX_HITS):
    """dsmi_spot_watch_pick (host only): the online picking rule of the streaming phrase watch over the tracks of one phrase,
    frames t0 .. t0 + len(E) - 1; ``state`` (a ``SpotPickState``) is carried from call to call, ``flush`` ends the utterance.
    -> (count, [(start, end, logp, fired), ...] the first min(count, max_events) events, frames [start, end))."""
    E = np.ascontiguousarray(E, dtype=np.float32).reshape(-1)
    ST = np.ascontiguousarray(ST, dtype=np.int32).reshape(-1)
    if len(E) != len(ST):
        raise ValueError("spot_watch_pick: one start frame per end score")
    M = int(max_events)
    hits = np.zeros((max(M, 0), 2), dtype=np.int32)
    scores = np.zeros(max(M, 0), dtype=np.float32)
    fired = np.zeros(max(M, 0), dtype=np.int32)
    rc = lib().dsmi_spot_watch_pick(_np_ptr(E) if len(E) else None, _np_ptr(ST) if len(E) else None, len(E), int(t0), int(bool(flush)),
                                    float(min_mean_logp), int(settle_frames), C.byref(state), M, _np_ptr(hits) if M > 0 else None,
                                    _np_ptr(scores) if M > 0 else None, _np_ptr(fired) if M > 0 else None)
    if rc < 0:
        raise DsmiError(rc, "dsmi_spot_watch_pick: frames from t0 >= 0 within 2^31 - 1, settle_frames >= 1, max_events >= 0, no NaN floor")
    return rc, [(int(hits[i, 0]), int(hits[i, 1]), float(scores[i]), int(fired[i])) for i in range(min(rc, M))]


class NativeSpotWatch(_Handle):
    """Owns one dsmi_spot_watch handle: a phrase list (label-id sequences) packed and uploaded once for ``decoder`` (a
    ``NativeDecoder``, kept alive by the watch), with the picking parameters of the streaming phrase watch."""
    _destroy, _last_error = "dsmi_spot_watch_destroy", "dsmi_spot_watch_last_error"

    def __init__(self, decoder, phrases, min_mean_logp, settle_frames):
        self.decoder = decoder
        ph, lens = _padded_ids(phrases, None, None, 1, None)
        self.min_mean_logp, self.settle_frames = float(min_mean_logp), int(settle_frames)
        self._create("dsmi_spot_watch_create", decoder._h, _np_ptr(ph), _np_ptr(lens) if len(lens) else None, len(lens), ph.shape[1],
                     self.min_mean_logp, self.settle_frames)
        K, G, S = C.c_int(), C.c_int(), C.c_int()
        self._check(lib().dsmi_spot_watch_info(self._h, C.byref(K), C.byref(G), C.byref(S)))
        self.K, self.n_groups = K.value, G.value
        assert S.value == self.settle_frames


class NativeSpotStream(_Handle):
    """Owns one dsmi_spot_stream handle: one live utterance's phrase search over ``watch`` (a ``NativeSpotWatch``, kept alive by
    the stream), carried from chunk to chunk."""
    _destroy, _last_error = "dsmi_spot_stream_destroy", "dsmi_spot_stream_last_error"

    def __init__(self, watch):
        self.watch = watch
        self._create("dsmi_spot_stream_create", watch._h)

    def close(self):
        if getattr(self.watch, "_h", None):      # (the handle points into its watch: after the watch has gone there is nothing to free safely)
            super().close()
        self._h = None

    def frames(self):
        f = C.c_int64()
        if lib().dsmi_spot_stream_frames(self._h, C.byref(f)) != 0:
            raise DsmiError(DSMI_ERR_INVALID, "closed spot stream")
        return int(f.value)

    def reset(self):
        if lib().dsmi_spot_stream_reset(self._h) != 0:
            raise DsmiError(DSMI_ERR_INVALID, "closed spot stream")

    @staticmethod
    def advance_many(streams, probs_list, flush, max_events=4, tracks=False):
        """dsmi_spot_stream_advance_many: advance distinct ``NativeSpotStream`` of one watch in one launch, stream i by the
        frames of ``probs_list[i]`` (CUDA float32 [T,C] or [1,T,C]; None or T = 0: no frames); ``flush[i]``: its utterance ends
        with them.  -> per stream the events fired in this call, ``(phrase_index, start, end, logp, fired)`` with frames
        [start, end) counted from the utterance's first frame, sorted by (fired, phrase_index); with ``tracks`` a tuple
        (events, E float32 [K,T], ST int32 [K,T]) of this call's frames.  A (stream, phrase) that fired more than
        ``max_events`` events in one call raises ``DsmiError`` (DSMI_ERR_CAPACITY) after every stream has advanced: use
        ``advance_many_counts`` to be told instead.  Longer lists than SPOT_STREAM_MANY_MAX run as several launches."""
        outs, counts = NativeSpotStream.advance_many_counts(streams, probs_list, flush, max_events, tracks)
        for i, c in enumerate(counts):
            if c.max(initial=0) > int(max_events):
                raise DsmiError(DSMI_ERR_CAPACITY, "spot stream %d: %d events of one phrase in one call, max_events = %d" % (i, int(c.max()), int(max_events)))
        return outs

    @staticmethod
    def advance_many_counts(streams, probs_list, flush, max_events=4, tracks=False):
        """``advance_many`` with, per stream, the int32 [K] counts of the events fired beside what was stored (the first
        ``max_events`` of each phrase): -> (outs, counts)."""
        import torch
        if not (len(probs_list) == len(flush) == len(streams)):
            raise ValueError("streams, probs_list and flush must have one entry per stream")
        probs, new = [], []
        for p in probs_list:
            t = 0
            if p is not None:
                t = p.shape[-2]
                p = p.reshape(t, p.shape[-1]).contiguous()
                assert p.is_cuda and p.dtype == torch.float32
            probs.append(p if t > 0 else None)
            new.append(t)
        outs, all_counts = [], []
        M = int(max_events)
        for ss, ps, ts, fl in _cut(SPOT_STREAM_MANY_MAX, streams, probs, new, list(flush)):
            n, K = len(ss), ss[0].watch.K
            fr = np.array(ts, dtype=np.int32)
            F = max(ts) if tracks else 0
            rows = max(M, 0)
            hits = np.zeros((n, K, rows, 2), dtype=np.int32)
            scores = np.zeros((n, K, rows), dtype=np.float32)
            fired = np.zeros((n, K, rows), dtype=np.int32)
            counts = np.zeros((n, K), dtype=np.int32)
            E = np.zeros((n, K, F), dtype=np.float32) if tracks else None
            ST = np.zeros((n, K, F), dtype=np.int32) if tracks else None
            NativeSpotStream._check_thread(lib().dsmi_spot_stream_advance_many(
                _handle_array(ss), n, _ptr_array(ps), _np_ptr(fr), _np_ptr(_flag_array(fl)), M, _np_ptr(hits), _np_ptr(scores), _np_ptr(fired),
                _np_ptr(counts), _np_ptr(E) if tracks else None, _np_ptr(ST) if tracks else None, F, _stream(ss[0].watch.decoder.device)))
            for i in range(n):
                ev = [(k, int(hits[i, k, e, 0]), int(hits[i, k, e, 1]), float(scores[i, k, e]), int(fired[i, k, e]))
                      for k in range(K) for e in range(min(int(counts[i, k]), M))]
                ev.sort(key=lambda h: (h[4], h[0]))
                outs.append((ev, E[i, :, :ts[i]].copy(), ST[i, :, :ts[i]].copy()) if tracks else ev)
                all_counts.append(counts[i].copy())
        return outs, all_counts

    def advance(self, probs, flush=False, max_events=4, tracks=False):
        return NativeSpotStream.advance_many([self], [probs], [flush], max_events, tracks)[0]


class NativeGrammarNet(_Handle):
    """Owns one dsmi_grammar_net handle: one graph or a list of K (as ``NativeDecoder.grammar`` takes them) checked, packed and
    uploaded once for ``decoder`` (a ``NativeDecoder``, kept alive by the net)."""
    _destroy, _last_error = "dsmi_grammar_net_destroy", "dsmi_grammar_net_last_error"

    def __init__(self, decoder, graphs):
        self.decoder = decoder
        pool, keep = grammar_pool(graphs)
        self._create("dsmi_grammar_net_create", decoder._h, C.byref(pool))
        del keep
        K, N, A = C.c_int(), C.c_int(), C.c_int()
        self._check(lib().dsmi_grammar_net_info(self._h, C.byref(K), C.byref(N), C.byref(A)))
        self.K, self.max_nodes, self.max_arcs = K.value, N.value, A.value


class NativeGrammarStream(_Handle):
    """Owns one dsmi_grammar_stream handle: one live utterance's search over graph ``graph`` of ``net`` (a ``NativeGrammarNet``,
    kept alive by the stream), carried from chunk to chunk for at most ``max_frames`` frames."""
    _destroy, _last_error = "dsmi_grammar_stream_destroy", "dsmi_grammar_stream_last_error"

    def __init__(self, net, graph=0, max_frames=1500):
        self.net, self.graph, self.max_frames = net, int(graph), int(max_frames)
        self._create("dsmi_grammar_stream_create", net._h, self.graph, self.max_frames)

    def close(self):
        if getattr(self.net, "_h", None):        # (the handle points into its net: after the net has gone there is nothing to free safely)
            super().close()
        self._h = None

    def frames(self):
        f = C.c_int64()
        if lib().dsmi_grammar_stream_frames(self._h, C.byref(f)) != 0:
            raise DsmiError(DSMI_ERR_INVALID, "closed grammar stream")
        return int(f.value)

    def reset(self):
        if lib().dsmi_grammar_stream_reset(self._h) != 0:
            raise DsmiError(DSMI_ERR_INVALID, "closed grammar stream")

    @staticmethod
    def advance_many(streams, rows, modes):
        """dsmi_grammar_stream_advance_many: advance distinct ``NativeGrammarStream`` of one net in one launch, stream i by the
        frames of ``rows[i]`` (CUDA float32 [T,C] or [1,T,C]; None or T = 0: no frames).  ``modes[i]``: 0 advance only, 1 then
        the partial result (the best path into any state), 2 then the final result (the utterance is over).  -> per stream
        None (mode 0) or (lens int, nodes int32 [F], spans int32 [F,2], token_probs float32 [F], logp float, status int,
        complete int) over the F frames of its utterance so far: what ``NativeDecoder.grammar`` gives for their concatenation.
        Longer lists than GRAMMAR_STREAM_MANY_MAX run as several launches."""
        import torch
        if not (len(rows) == len(modes) == len(streams)):
            raise ValueError("streams, rows and modes must have one entry per stream")
        probs, new = [], []
        for p in rows:
            t = 0
            if p is not None:
                t = p.shape[-2]
                p = p.reshape(t, p.shape[-1]).contiguous()
                assert p.is_cuda and p.dtype == torch.float32
            probs.append(p if t > 0 else None)
            new.append(t)
        outs = []
        for ss, ps, ts, md in _cut(GRAMMAR_STREAM_MANY_MAX, streams, probs, new, [int(m) for m in modes]):
            n = len(ss)
            fr, mo = np.array(ts, dtype=np.int32), np.array(md, dtype=np.int32)
            due = [i for i in range(n) if md[i] != 0]
            after = [ss[i].frames() + ts[i] for i in due]
            P = max(after, default=0)
            lens, lp, st, cp = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            nodes, spans, tp = np.zeros((n, P), dtype=np.int32), np.zeros((n, P, 2), dtype=np.int32), np.zeros((n, P), dtype=np.float32)
            NativeGrammarStream._check_thread(lib().dsmi_grammar_stream_advance_many(
                _handle_array(ss), n, _ptr_array(ps), _np_ptr(fr), _np_ptr(mo), P, _np_ptr(lens), _np_ptr(nodes), _np_ptr(spans), _np_ptr(tp),
                _np_ptr(lp), _np_ptr(st), _np_ptr(cp), _stream(ss[0].net.decoder.device)))
            res = [None] * n
            for i, F in zip(due, after):
                res[i] = (int(lens[i]), nodes[i, :F].copy(), spans[i, :F].copy(), tp[i, :F].copy(), float(lp[i]), int(st[i]), int(cp[i]))
            outs += res
        return outs

    def advance(self, rows, mode=0):
        return NativeGrammarStream.advance_many([self], [rows], [mode])[0]


class NativeLM(_Handle):
    """Host-only view of a language-model file through libdsmi.so's reader (``dsmi_lm_*``): no GPU needed."""
    _destroy, _last_error, _host_only = "dsmi_lm_close", "dsmi_lm_last_error", True
    KINDS = {0: "arpa", 1: "klm-probing", 2: "klm-trie"}

    def __init__(self, path):
        self._create("dsmi_lm_open", str(path).encode())
        o = C.c_int(); v = C.c_int64(); k = C.c_int()
        lib().dsmi_lm_info(self._h, C.byref(o), C.byref(v), C.byref(k))
        self.order, self.vocab_size, self.kind = o.value, v.value, self.KINDS[k.value]

    def word_index(self, word):
        return int(lib().dsmi_lm_word_index(self._h, word.encode("utf-8")))

    def lookup(self, ids):
        """(log10 prob, log10 backoff) of the n-gram, or None."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        lp = C.c_float(); bo = C.c_float()
        rc = lib().dsmi_lm_lookup(self._h, _np_ptr(a), len(a), C.byref(lp), C.byref(bo))
        if rc < 0:
            raise DsmiError(rc, "bad n-gram")
        return (lp.value, bo.value) if rc == 1 else None

    def cond_log10(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        return float(lib().dsmi_lm_cond_log10(self._h, _np_ptr(a), len(a)))

    def sentence_ln(self, word_ids):
        """(natural-log sentence score, its window terms float64 [n + 1], or [2] for no words) of a sentence of the file's own
        word ids, -1 = out of vocabulary (``dsmi_lm_sentence_ln``: ctcdecode ``Scorer.get_sent_log_prob``)."""
        a = np.ascontiguousarray(word_ids, dtype=np.int32).reshape(-1)
        terms = np.zeros(max(len(a) + 1, 2), dtype=np.float64)
        return float(lib().dsmi_lm_sentence_ln(self._h, _np_ptr(a) if len(a) else None, len(a), _np_ptr(terms), len(terms))), terms


def plan_shards(n_samples, world):
    """dsmi_plan_shards: (rank_of, slot_of) int32 arrays."""
    n = np.ascontiguousarray(n_samples, dtype=np.int64)
    rank_of = np.zeros(len(n), dtype=np.int32)
    slot_of = np.zeros(len(n), dtype=np.int32)
    rc = lib().dsmi_plan_shards(_np_ptr(n) if len(n) else None, len(n), int(world),
                                _np_ptr(rank_of) if len(n) else None, _np_ptr(slot_of) if len(n) else None)
    if rc != 0:
        raise DsmiError(rc, "dsmi_plan_shards")
    return rank_of, slot_of


class NativeSession(_Handle):
    """dsmi_session_*: the fused recognise call a host without the Python layer uses (tests drive it through ctypes).
    ``frontend`` / ``model`` / ``decoder``: NativeFrontend / NativeModel / NativeDecoder; they must outlive the session."""
    _destroy, _last_error = "dsmi_session_destroy", "dsmi_session_last_error"
    _finalise = False       # at interpreter exit the object may outlive the model (as a NativeComm may the RCCL runtime): close() only

    def __init__(self, frontend, model, decoder):
        self._keep = (frontend, model, decoder)
        self._create("dsmi_session_create", frontend._h, model._h, decoder._h)

    def enqueue(self, clips):
        clips = [np.ascontiguousarray(c) for c in clips]
        kinds = {c.dtype for c in clips}
        if len(kinds) != 1 or next(iter(kinds)) not in PCM_DTYPES:
            raise ValueError("clips of one sample type: int16, float32 or float64")
        n = np.array([len(c) for c in clips], dtype=np.int64)
        ptrs = (_vp * len(clips))(*[c.ctypes.data for c in clips])
        self._check(lib().dsmi_recognize_enqueue(self._h, ptrs, _np_ptr(n), _pcm_code(clips[0].dtype), len(clips)))
        self._count = len(clips)

    def enqueue_device(self, pcm_dev, n_samples, dtype_code):
        n = np.ascontiguousarray(n_samples, dtype=np.int64)
        ptr = pcm_dev.data_ptr() if hasattr(pcm_dev, "data_ptr") else int(pcm_dev)
        self._check(lib().dsmi_recognize_enqueue_device(self._h, ptr, _np_ptr(n), int(dtype_code), len(n)))
        self._count = len(n)
        self._keep_pcm = pcm_dev

    def collect(self, beam_width=0, cutoff_top_n=40, cutoff_prob=1.0, text_stride=4096, raw=False):
        B = self._count
        text = np.zeros((B, text_stride), dtype=np.uint8)
        nbytes = np.zeros(B, dtype=np.int32)
        scores = np.zeros(B, dtype=np.float32)
        rc = lib().dsmi_recognize_collect(self._h, int(beam_width), int(cutoff_top_n), float(cutoff_prob), text.ctypes.data, text_stride,
                                          _np_ptr(nbytes), _np_ptr(scores))
        if rc < 0:
            self._check(rc)
        self.last_status = rc
        if raw:
            return text, nbytes, scores
        return [bytes(text[b]).split(b"\0", 1)[0].decode("utf-8") for b in range(B)], nbytes, scores

    def recognize_batch(self, clips, **kw):
        self.enqueue(clips)
        return self.collect(**kw)


class NativeComm(_Handle):
    """dsmi_comm_*: scatter / gather over RCCL for hosts without torch.distributed."""
    _destroy, _last_error = "dsmi_comm_destroy", "dsmi_comm_last_error"
    _finalise = False       # (see NativeSession)

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * 128)()
        NativeComm._check_thread(lib().dsmi_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, unique_id, rank, world, device):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self._create("dsmi_comm_init", buf, int(rank), int(world), int(device))
        self.rank, self.world, self.device = rank, world, device

    def scatter(self, clips, root=0, cap=4096):
        """-> (device address of the shard, n_samples int64[count], positions int32[count], sample-type code, total)."""
        ptrs, n, code, count = None, None, 0, 0
        if self.rank == root:
            clips = [np.ascontiguousarray(c) for c in clips]
            code = _pcm_code(clips[0].dtype) if clips else 0
            n = np.array([len(c) for c in clips], dtype=np.int64)
            ptrs = (_vp * max(len(clips), 1))(*[c.ctypes.data for c in clips])
            count = len(clips)
        dev = _vp()
        sn = np.zeros(cap, dtype=np.int64)
        si = np.zeros(cap, dtype=np.int32)
        cnt, dt, tot = C.c_int(), C.c_int(), C.c_int()
        rc = lib().dsmi_comm_scatter(self._h, root, ptrs, _np_ptr(n) if n is not None and len(n) else None, code, count, C.byref(dev),
                                     _np_ptr(sn), _np_ptr(si), cap, C.byref(cnt), C.byref(dt), C.byref(tot), _stream(self.device))
        self._check(rc)
        return dev.value, sn[:cnt.value].copy(), si[:cnt.value].copy(), dt.value, tot.value

    def gather_text(self, text, positions, total, root=0):
        """text: uint8 [count][stride] (NativeSession.collect(raw=True)); -> list of str on the root, None elsewhere."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        stride = text.shape[1]
        pos = np.ascontiguousarray(positions, dtype=np.int32)
        out = np.zeros((max(total, 1), stride), dtype=np.uint8)
        rc = lib().dsmi_comm_gather_text(self._h, root, text.ctypes.data if len(pos) else None, stride, _np_ptr(pos) if len(pos) else None,
                                         len(pos), total, out.ctypes.data, _stream(self.device))
        self._check(rc)
        if self.rank != root:
            return None
        return [bytes(out[i]).split(b"\0", 1)[0].decode("utf-8") for i in range(total)]
