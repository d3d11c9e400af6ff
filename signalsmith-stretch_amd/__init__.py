"""signalsmith-stretch_amd -- MI355X (gfx950) implementation of the Signalsmith Stretch spectral hot path.

Python is plumbing only: this module binds the C ABI of ``libsmst_hip.so`` (``include/smst.h``) with ctypes and
mirrors the reference class' method names (``signalsmith-stretch.h:38-491``) so tests read like calls on the
reference.  All arithmetic runs in the hand-written HIP kernels under ``csrc/``; there is NO CPU fallback -- if
the shared library is missing or no GPU is visible, construction raises.

The directory name contains a hyphen (it follows the reference project's name), so import it with::

    import importlib; smst = importlib.import_module("signalsmith-stretch_amd")
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (The engine's three pipeline streams should not share a hardware queue: INTEGRATION.md "Hardware queues" asks the HOST APPLICATION to
# export GPU_MAX_HW_QUEUES=8 before the HIP runtime starts.  Importing this package does not touch the environment -- bench.py and tools/
# set the variable themselves; load_library() warns once when it finds the runtime already started with fewer queues.)
# SMST_LIBRARY: measurement hook of bench.py / tools/ -- another BUILD of the same library (an A/B variant, an instrumented trace
# build under variants/), never another implementation; unset in every product use, and announced on stderr when set.  A build that
# lacks entry points of include/smst.h is refused at load unless SMST_LIBRARY_ALLOW_MISSING=1 (A/B against an older revision).
LIBRARY_PATH = os.environ.get("SMST_LIBRARY") or os.path.join(_HERE, "libsmst_hip.so")
CSRC_DIR = os.path.join(_HERE, "csrc")

MEM_HOST, MEM_DEVICE = 0, 1
PCM_S16, PCM_F32, PCM_S24, PCM_S32, PCM_F16 = 1, 2, 4, 5, 6  # frame formats of the *_pcm calls (include/smst.h)
DITHER_NONE, DITHER_TPDF, DITHER_TPDF_HP = 0, 1, 2           # dither of the int16 / int24 output (StretchBatch.setPcmDither)
LEVEL_FIXED, LEVEL_PROTECT, LEVEL_NORMALISE = 0, 1, 2        # level of the frame output (StretchBatch.set_pcm_level)
LEVEL_LOUDNESS = 3                                           # ... to a LUFS target (StretchBatch.set_pcm_loudness)
RESAMPLE_MAX_TERM, RESAMPLE_MAX_RATIOS, RESAMPLE_TILE = 640, 8, 1024   # the limits of a resample ratio, and the frames a workgroup forms (SMST_RESAMPLE_*)
LOUDNESS_RANGE_TILE = 256                                   # short-term powers the range stage's workgroup takes at a time (SMST_LOUDNESS_RANGE_TILE)
LOUDNESS_CHUNK = 256                                         # frames one lane of the loudness passes filters (SMST_LOUDNESS_CHUNK)
TRUE_PEAK_TILE = 1024                                        # frames one workgroup of the true-peak pass measures (SMST_TRUE_PEAK_TILE)
LIMITER_TILE, LIMITER_MAX_LOOKAHEAD, LIMITER_DEFAULT_LOOKAHEAD = 1024, 1024, 72  # frames one workgroup of the limiter's passes takes; the lookahead's bound and default (SMST_LIMITER_*)
STREAM_LIMITER_TRUE_PEAK_DELAY = 6  # frames a stream with the stream limiter's true-peak flag is late beyond 2*lookahead (SMST_STREAM_LIMITER_TRUE_PEAK_DELAY)
_FRAME_DTYPES = {"int16": PCM_S16, "float32": PCM_F32, "int32": PCM_S32, "float16": PCM_F16}  # (packed int24 travels as uint8 [..., 3])
_FRAME_DTYPE_OF = {PCM_S16: "int16", PCM_F32: "float32", PCM_S32: "int32", PCM_F16: "float16", PCM_S24: "uint8"}
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)
_ll = C.c_longlong

# name -> (restype, argtypes); every symbol include/smst.h declares
_SIGNATURES = {
    "smst_last_error": (C.c_char_p, []),
    "smst_reference_version": (None, [_ip]),
    "smst_device_count": (C.c_int, []),
    # single-stream
    "smst_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_long, C.c_int]),
    "smst_destroy": (None, [C.c_void_p]),
    "smst_clone": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p]),
    "smst_default_device": (C.c_int, []),
    "smst_set_default_device": (C.c_int, [C.c_int]),
    "smst_preset_default": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int]),
    "smst_preset_cheaper": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int]),
    "smst_configure": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]),
    "smst_block_samples": (C.c_int, [C.c_void_p]),
    "smst_interval_samples": (C.c_int, [C.c_void_p]),
    "smst_input_latency": (C.c_int, [C.c_void_p]),
    "smst_output_latency": (C.c_int, [C.c_void_p]),
    "smst_split_computation": (C.c_int, [C.c_void_p]),
    "smst_block_steps": (C.c_int, [C.c_void_p]),
    "smst_blocks_started": (C.c_int, [C.c_void_p]),
    "smst_seek_length": (C.c_int, [C.c_void_p]),
    "smst_output_seek_length": (C.c_int, [C.c_void_p, C.c_float]),
    "smst_reset": (C.c_int, [C.c_void_p]),
    "smst_set_transpose_factor": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "smst_set_transpose_semitones": (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    "smst_set_formant_factor": (C.c_int, [C.c_void_p, C.c_float, C.c_int]),
    "smst_set_formant_semitones": (C.c_int, [C.c_void_p, C.c_float, C.c_int]),
    "smst_set_formant_base": (C.c_int, [C.c_void_p, C.c_float]),
    "smst_set_freq_map_table": (C.c_int, [C.c_void_p, _fp, C.c_int]),
    "smst_seek": (C.c_int, [C.c_void_p, C.POINTER(_fp), C.c_int, C.c_double]),
    "smst_process": (C.c_int, [C.c_void_p, C.POINTER(_fp), C.c_int, C.POINTER(_fp), C.c_int]),
    "smst_flush": (C.c_int, [C.c_void_p, C.POINTER(_fp), C.c_int, C.c_float]),
    "smst_output_seek": (C.c_int, [C.c_void_p, C.POINTER(_fp), C.c_int]),
    "smst_exact": (C.c_int, [C.c_void_p, C.POINTER(_fp), C.c_int, C.POINTER(_fp), C.c_int]),
    # pool (extension)
    "smst_pool_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "smst_pool_destroy": (None, [C.c_void_p]),
    "smst_pool_attach": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smst_pool_detach": (C.c_int, [C.c_void_p]),
    "smst_pool_members": (C.c_int, [C.c_void_p]),
    "smst_pool_pending": (C.c_int, [C.c_void_p]),
    "smst_pool_run": (C.c_int, [C.c_void_p]),
    "smst_process_begin": (C.c_int, [C.c_void_p, C.POINTER(_fp), C.c_int, C.POINTER(_fp), C.c_int]),
    "smst_process_end": (C.c_int, [C.c_void_p]),
    "smst_pool_debug_engine_calls": (_ll, [C.c_void_p]),
    "smst_pool_debug_allocation_events": (_ll, [C.c_void_p]),
    # batch
    "smst_batch_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long]),
    "smst_batch_create_preset": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_long]),
    "smst_batch_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_uint]),
    "smst_batch_create_preset_ex": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_long, C.c_uint]),
    "smst_batch_destroy": (None, [C.c_void_p]),
    "smst_batch_streams": (C.c_int, [C.c_void_p]),
    "smst_batch_channels": (C.c_int, [C.c_void_p]),
    "smst_batch_block_samples": (C.c_int, [C.c_void_p]),
    "smst_batch_interval_samples": (C.c_int, [C.c_void_p]),
    "smst_batch_fft_samples": (C.c_int, [C.c_void_p]),
    "smst_batch_bands": (C.c_int, [C.c_void_p]),
    "smst_batch_input_latency": (C.c_int, [C.c_void_p]),
    "smst_batch_output_latency": (C.c_int, [C.c_void_p]),
    "smst_batch_seek_length": (C.c_int, [C.c_void_p]),
    "smst_batch_half_state": (C.c_int, [C.c_void_p]),
    "smst_batch_output_seek_length": (C.c_int, [C.c_void_p, C.c_float]),
    "smst_batch_workspace_bytes": (_ll, [C.c_void_p]),
    "smst_batch_reset": (C.c_int, [C.c_void_p]),
    "smst_batch_set_transpose_factor": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "smst_batch_set_transpose_semitones": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_float]),
    "smst_batch_set_formant_factor": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int]),
    "smst_batch_set_formant_semitones": (C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_int]),
    "smst_batch_set_formant_base": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "smst_batch_set_freq_map_table": (C.c_int, [C.c_void_p, C.c_int, _fp, C.c_int]),
    "smst_batch_seek": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, _dp, C.c_int]),
    "smst_batch_process": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, C.c_void_p, _ll, _ll, _ip, C.c_int]),
    "smst_batch_flush": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, _fp, C.c_int]),
    "smst_batch_output_seek": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, C.c_int]),
    "smst_batch_exact": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, C.c_void_p, _ll, _ll, _ip, _ip, C.c_int]),
    "smst_batch_exact_pcm": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, C.c_void_p, _ll, _ll, _ip, _ip, C.c_int, C.c_int]),
    "smst_debug_clip_copy": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, C.c_void_p, _ll, _ll, C.POINTER(_ll), C.POINTER(_ll)]),
    "smst_batch_process_pcm": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, C.c_void_p, _ll, _ll, _ip, C.c_int, C.c_int]),
    "smst_batch_seek_pcm": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, _dp, C.c_int, C.c_int]),
    "smst_batch_flush_pcm": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, _fp, C.c_int, C.c_int]),
    "smst_batch_output_seek_pcm": (C.c_int, [C.c_void_p, C.c_void_p, _ll, _ll, _ip, C.c_int, C.c_int]),
    "smst_debug_pcm_convert": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, C.c_void_p, _ll, _ll]),
    "smst_debug_pcm_convert_counted": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, C.c_void_p, _ll, _ll, C.POINTER(_ll), C.POINTER(_ll)]),
    "smst_batch_take_pcm_overs": (C.c_int, [C.c_void_p, C.POINTER(_ll), C.POINTER(_ll)]),
    "smst_batch_set_pcm_dither": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ll]),
    "smst_batch_pcm_dither": (C.c_int, [C.c_void_p, C.c_int, _ip, C.POINTER(_ll), C.POINTER(_ll)]),
    "smst_debug_pcm_convert_dithered": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, C.c_void_p, _ll, _ll, _ip, C.POINTER(_ll), C.POINTER(_ll),
                                                  C.POINTER(_ll), C.POINTER(_ll)]),
    "smst_batch_set_pcm_level": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float]),
    "smst_batch_pcm_level": (C.c_int, [C.c_void_p, C.c_int, _ip, _fp, _fp]),
    "smst_batch_take_pcm_peaks": (C.c_int, [C.c_void_p, _fp, _fp]),
    "smst_debug_pcm_convert_levelled": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, C.c_void_p, _ll, _ll, _ip, C.POINTER(_ll), C.POINTER(_ll),
                                                  _fp, C.POINTER(_ll), C.POINTER(_ll), _fp]),
    "smst_debug_clip_copy_levelled": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, C.c_void_p, _ll, _ll, _ip, _fp, _fp, _ip, C.POINTER(_ll),
                                                C.POINTER(_ll), C.POINTER(_ll), _fp, _fp]),
    "smst_batch_set_pcm_loudness": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_float, C.c_double]),
    "smst_batch_pcm_loudness": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "smst_batch_set_pcm_loudness_weights": (C.c_int, [C.c_void_p, _fp]),
    "smst_batch_take_pcm_loudness": (C.c_int, [C.c_void_p, _dp, _ip, _ip]),
    "smst_debug_clip_loudness": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, _dp, _fp, C.c_double, _dp, _ip, _ip, _fp, _dp, C.c_int]),
    "smst_batch_set_pcm_true_peak": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "smst_batch_pcm_true_peak": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "smst_batch_take_pcm_true_peaks": (C.c_int, [C.c_void_p, _fp]),
    "smst_debug_clip_true_peak": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, _fp, _fp, _ip]),
    "smst_debug_true_peak_taps": (C.c_int, [_fp]),
    "smst_batch_set_pcm_limiter": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "smst_batch_pcm_limiter": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "smst_batch_set_pcm_limiter_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "smst_batch_pcm_limiter_lookahead": (C.c_int, [C.c_void_p, _ip]),
    "smst_batch_take_pcm_limiter": (C.c_int, [C.c_void_p, _fp, C.POINTER(_ll)]),
    "smst_debug_clip_limit": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, _fp, _fp, _ip, C.c_int, _fp, _fp, C.c_int, _fp, C.POINTER(_ll)]),
    "smst_debug_limiter_window": (C.c_int, [C.c_int, _fp]),
    "smst_batch_set_pcm_stream_limiter": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float]),
    "smst_batch_pcm_stream_limiter": (C.c_int, [C.c_void_p, C.c_int, _ip, _fp]),
    "smst_batch_pcm_stream_limiter_latency": (C.c_int, [C.c_void_p, _ip]),
    "smst_batch_set_pcm_stream_limiter_true_peak": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "smst_batch_pcm_stream_limiter_true_peak": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "smst_batch_pcm_stream_limiter_latency_of": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "smst_batch_take_pcm_stream_limiter": (C.c_int, [C.c_void_p, _fp, C.POINTER(_ll)]),
    "smst_debug_pcm_stream_limit": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, _fp, _fp, _ip, C.c_int, _fp, _fp, C.c_int, _fp, C.POINTER(_ll)]),
    "smst_batch_set_pcm_loudness_range": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double]),
    "smst_batch_pcm_loudness_range": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp]),
    "smst_batch_set_pcm_loudness_caps": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double]),
    "smst_batch_pcm_loudness_caps": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp]),
    "smst_batch_take_pcm_loudness_range": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _ip, _ip]),
    "smst_debug_clip_loudness_range": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, C.c_void_p, _ll, _ll, _dp, _fp, C.c_double, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _fp, _dp, C.c_int]),
    "smst_batch_set_pcm_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "smst_batch_pcm_resample": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip]),
    "smst_batch_resampled_length": (_ll, [C.c_void_p, C.c_int, _ll]),
    "smst_resample_ratio": (C.c_int, [C.c_double, C.c_double, _ip, _ip]),
    "smst_debug_resample_taps": (C.c_int, [C.c_int, C.c_int, _fp, _ip]),
    "smst_debug_clip_resample": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_void_p, _ll, _ll, _ip, C.c_void_p, _ll, _ll]),
    "smst_batch_set_pcm_out_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "smst_batch_pcm_out_resample": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip]),
    "smst_batch_pcm_out_render_length": (_ll, [C.c_void_p, C.c_int, _ll]),
    "smst_debug_clip_resample_out": (C.c_int, [C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_void_p, _ll, _ll, _ip, _ip, C.c_void_p, _ll, _ll]),
    "smst_batch_set_pcm_stream_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "smst_batch_pcm_stream_resample": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip]),
    "smst_batch_pcm_stream_resample_latency": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "smst_batch_pcm_stream_resample_frames": (_ll, [C.c_void_p, C.c_int, _ll, C.c_int]),
    "smst_batch_pcm_stream_resample_need": (_ll, [C.c_void_p, C.c_int, _ll, C.c_int]),
    "smst_debug_pcm_stream_resample": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, C.POINTER(_ll), C.c_void_p, _ll, _ll, C.c_void_p, _ll, _ll, C.c_int, C.POINTER(_ll)]),
    "smst_batch_set_pcm_stream_meter": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int]),
    "smst_batch_pcm_stream_meter": (C.c_int, [C.c_void_p, C.c_int, _ip, _dp, _ip]),
    "smst_batch_pcm_stream_meter_frames": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(_ll), C.POINTER(_ll)]),
    "smst_batch_take_pcm_stream_meter": (C.c_int, [C.c_void_p, _dp, _ip, _ip, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _fp, _fp]),
    "smst_debug_pcm_stream_meter": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, C.c_int, C.c_void_p, _ll, _ll, _dp, _fp, _ip, C.c_int,
                                              _dp, _ip, _ip, _dp, _dp, _dp, _dp, _ip, _ip, _fp, _fp, C.POINTER(_ll), _dp, _dp, C.c_int]),
    "smst_batch_set_pcm_stream_out_resample": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "smst_batch_pcm_stream_out_resample": (C.c_int, [C.c_void_p, C.c_int, _ip, _ip]),
    "smst_batch_pcm_stream_out_resample_latency": (C.c_int, [C.c_void_p, C.c_int, _ip]),
    "smst_batch_pcm_stream_out_resample_render": (_ll, [C.c_void_p, C.c_int, _ll, C.c_int]),
    "smst_debug_pcm_stream_resample_out": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, C.POINTER(_ll), C.c_void_p, _ll, _ll, C.c_void_p, _ll, _ll, C.c_int, C.POINTER(_ll)]),
    "smst_batch_synchronize": (C.c_int, [C.c_void_p]),
    "smst_batch_hip_stream": (C.c_void_p, [C.c_void_p]),
    "smst_batch_enable_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "smst_batch_take_timings": (C.c_int, [C.c_void_p, _dp, C.POINTER(_ll)]),
    "smst_batch_take_host_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(_ll)]),
    "smst_batch_debug_get_state": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _fp]),
    "smst_batch_debug_get_carry": (C.c_int, [C.c_void_p, C.c_int, _fp, _fp]),
    "smst_batch_debug_set_state": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _fp]),
    "smst_batch_debug_set_carry": (C.c_int, [C.c_void_p, C.c_int, _fp, _fp]),
    "smst_batch_debug_get_map": (C.c_int, [C.c_void_p, C.c_int, _fp]),
    "smst_batch_debug_get_formants": (C.c_int, [C.c_void_p, C.c_int, _fp, _fp, _fp]),
    "smst_batch_debug_allocation_events": (_ll, [C.c_void_p]),
    "smst_batch_wait_for_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smst_batch_signal_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "smst_debug_complex_selftest": (C.c_int, [C.c_int, _fp, _fp, C.c_int]),
    "smst_debug_fft_complex_selftest": (C.c_int, [C.c_int, _fp, _fp, C.c_int]),
    "smst_debug_launch_count": (_ll, [C.c_char_p]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


class StretchError(RuntimeError):
    pass


def bind(cdll):
    """Attach the include/smst.h prototypes to a loaded library object."""
    missing = [name for name in _SIGNATURES if not hasattr(cdll, name)]
    if missing and not (os.environ.get("SMST_LIBRARY") and os.environ.get("SMST_LIBRARY_ALLOW_MISSING") == "1"):
        raise StretchError("the library lacks entry points of include/smst.h: %s (a stale build? rebuild with __graft_entry__.build(); "
                           "an A/B build of an older revision needs SMST_LIBRARY_ALLOW_MISSING=1)" % ", ".join(missing))
    for name, (res, args) in _SIGNATURES.items():
        if name in missing:
            continue
        f = getattr(cdll, name)
        f.restype = res
        f.argtypes = args
    return cdll


def library_path():
    return LIBRARY_PATH


def load_library():
    """Load libsmst_hip.so (built by ``__graft_entry__.build()`` / ``csrc/Makefile``).  Raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBRARY_PATH):
            raise StretchError(
                "libsmst_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % LIBRARY_PATH)
        # PyTorch ships its own HIP runtime; when both live in one process it has to be the first one loaded
        # (torch is the plumbing for device tensors/streams here, so load it first whenever it is installed).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        import sys
        try:  # advisory only: with 4 hardware queues (HIP's default) a step of the pipelined engine takes ~12 % longer next to an RCCL communicator
            queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
        except ValueError:
            queues = 4
        torch_mod = sys.modules.get("torch")
        if queues < 8 and torch_mod is not None and torch_mod.cuda.is_available() and torch_mod.cuda.is_initialized():
            print("signalsmith-stretch_amd: the HIP runtime is already running with GPU_MAX_HW_QUEUES=%d; export GPU_MAX_HW_QUEUES=8 before the "
                  "first HIP call so that the engine's pipeline streams get hardware queues of their own (INTEGRATION.md)" % queues, file=sys.stderr)
        if os.environ.get("SMST_LIBRARY"):
            print("signalsmith-stretch_amd: SMST_LIBRARY is set -- loading %s instead of the in-tree library (measurement hook)" % LIBRARY_PATH, file=sys.stderr)
        _lib = bind(C.CDLL(LIBRARY_PATH))
    return _lib


def build(verbose=False):
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess
    res = subprocess.run(["make", "-C", CSRC_DIR], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
        print(res.stderr)
    if res.returncode != 0:
        raise StretchError("hipcc build failed")
    return LIBRARY_PATH


def _check(lib, rc):
    if rc != 0:
        raise StretchError("smst error %d: %s" % (rc, (lib.smst_last_error() or b"").decode()))


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _int_array(values, n):
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.int32), (n,)))
    return a, a.ctypes.data_as(_ip)


def complex_selftest(values, device=0, lib=None):
    """values: [n, 7] float32 (a, b, c complex + a fraction) -> [n, 8] (a*b, a*conj(b), a*b + c, lerp) from the device helpers."""
    lib = lib if lib is not None else load_library()
    v = np.ascontiguousarray(values, np.float32).reshape(-1, 7)
    out = np.zeros((v.shape[0], 8), np.float32)
    _check(lib, lib.smst_debug_complex_selftest(device, v.ctypes.data_as(_fp), out.ctypes.data_as(_fp), v.shape[0]))
    return out


def fft_complex_selftest(values, device=0, lib=None):
    """values: [n, 4] float32 (a, b complex) -> [n, 20]: a*b, a*conj(b) (twiddle form), a*conj(b) (window form), a + i b, a - i b, a + b, a - b,
    conj(a) (store), conj(a) (load), a -- from the FFT kernels' helpers (csrc/smst_fft_complex.h)."""
    lib = lib if lib is not None else load_library()
    v = np.ascontiguousarray(values, np.float32).reshape(-1, 4)
    out = np.zeros((v.shape[0], 20), np.float32)
    _check(lib, lib.smst_debug_fft_complex_selftest(device, v.ctypes.data_as(_fp), out.ctypes.data_as(_fp), v.shape[0]))
    return out


def _level_arrays(n, *columns):
    """per-stream columns of the levelled debug hooks -> contiguous arrays (int32 / float32 / int64 by the column's kind) and their pointers"""
    kinds = {"i": (np.int32, _ip), "f": (np.float32, _fp), "l": (np.int64, C.POINTER(_ll))}
    arrays = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, kinds[k][0]), (n,))) for k, v in columns]
    return arrays, [a.ctypes.data_as(kinds[k][1]) for a, (k, _) in zip(arrays, columns)]


def debug_pcm_convert_levelled(fmt, counts, channels, src, src_ss, src_cs, dst, dst_ss, dst_fs, modes, seeds, firsts, gains, device=0, lib=None):
    """smst_debug_pcm_convert_levelled on numpy buffers (src planar float32, dst the frames' bytes or elements; strides in elements)
    -> (clamped, nans int64 [S], peaks float32 [S])"""
    lib = lib if lib is not None else load_library()
    S = len(counts)
    keep, (pc, pm, ps, pf, pg) = _level_arrays(S, ("i", counts), ("i", modes), ("l", seeds), ("l", firsts), ("f", gains))
    clamped, nans, peaks = np.full(S, -1, np.int64), np.full(S, -1, np.int64), np.full(S, -1, np.float32)
    _check(lib, lib.smst_debug_pcm_convert_levelled(device, fmt, S, channels, pc, C.c_void_p(src.ctypes.data), src_ss, src_cs, C.c_void_p(dst.ctypes.data), dst_ss, dst_fs,
                                                    pm, ps, pf, pg, clamped.ctypes.data_as(C.POINTER(_ll)), nans.ctypes.data_as(C.POINTER(_ll)), peaks.ctypes.data_as(_fp)))
    return clamped, nans, peaks


def debug_clip_copy_levelled(fmt, segments, channels, src, src_ss, src_cs, dst, dst_ss, dst_fs, level_modes, gains, ceilings, dither_modes, seeds, device=0, lib=None):
    """smst_debug_clip_copy_levelled on numpy buffers (src the planar float32 image, dst the frames; segments int [S, 2, 4])
    -> (clamped, nans int64 [S], peaks, applied float32 [S])"""
    lib = lib if lib is not None else load_library()
    seg = np.ascontiguousarray(segments, np.int32)
    S = seg.shape[0]
    keep, (pl, pg, pc, pd, ps) = _level_arrays(S, ("i", level_modes), ("f", gains), ("f", ceilings), ("i", dither_modes), ("l", seeds))
    clamped, nans = np.full(S, -1, np.int64), np.full(S, -1, np.int64)
    peaks, applied = np.full(S, -1, np.float32), np.full(S, -1, np.float32)
    _check(lib, lib.smst_debug_clip_copy_levelled(device, fmt, S, channels, seg.ctypes.data_as(_ip), C.c_void_p(src.ctypes.data), src_ss, src_cs, C.c_void_p(dst.ctypes.data), dst_ss, dst_fs,
                                                  pl, pg, pc, pd, ps, clamped.ctypes.data_as(C.POINTER(_ll)), nans.ctypes.data_as(C.POINTER(_ll)),
                                                  peaks.ctypes.data_as(_fp), applied.ctypes.data_as(_fp)))
    return clamped, nans, peaks, applied


def debug_clip_loudness(segments, channels, image, image_ss, image_cs, sample_rates, weights=None, target=-23.0, max_blocks=0, device=0, lib=None):
    """smst_debug_clip_loudness on a numpy image (planar float32; segments int [S, 2, 4]; strides in floats)
    -> (Z float64 [S], blocks, gated int32 [S], gains float32 [S], block powers float64 [S, max_blocks], NaN behind a stream's last block)"""
    lib = lib if lib is not None else load_library()
    seg = np.ascontiguousarray(segments, np.int32)
    S = seg.shape[0]
    rates = np.ascontiguousarray(np.broadcast_to(np.asarray(sample_rates, np.float64), (S,)))
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    assert w is None or w.shape == (channels,)
    Z, blocks, gated, gains = np.full(S, -1.0), np.full(S, -1, np.int32), np.full(S, -1, np.int32), np.full(S, -1, np.float32)
    powers = np.full((S, max(max_blocks, 1)), np.nan)
    _check(lib, lib.smst_debug_clip_loudness(device, S, channels, seg.ctypes.data_as(_ip), C.c_void_p(image.ctypes.data), image_ss, image_cs, rates.ctypes.data_as(_dp),
                                             None if w is None else w.ctypes.data_as(_fp), float(target), Z.ctypes.data_as(_dp), blocks.ctypes.data_as(_ip),
                                             gated.ctypes.data_as(_ip), gains.ctypes.data_as(_fp), powers.ctypes.data_as(_dp), max_blocks))
    return Z, blocks, gated, gains, powers[:, :max_blocks]


def debug_clip_loudness_range(segments, channels, image, image_ss, image_cs, sample_rates, weights=None, target=-23.0, caps=None, max_blocks=0, device=0, lib=None):
    """smst_debug_clip_loudness_range on a numpy image (as debug_clip_loudness; caps: [S, 2] in LUFS -- momentary, short-term; inf: none --, None:
    none) -> (M, ST, lo, hi: powers, float64 [S]; ns, n: int32 [S]; gains float32 [S]; short-term powers float64 [S, max_blocks], NaN behind
    a stream's last one)"""
    lib = lib if lib is not None else load_library()
    seg = np.ascontiguousarray(segments, np.int32)
    S = seg.shape[0]
    rates = np.ascontiguousarray(np.broadcast_to(np.asarray(sample_rates, np.float64), (S,)))
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    assert w is None or w.shape == (channels,)
    k = None if caps is None else np.ascontiguousarray(caps, np.float64)
    assert k is None or k.shape == (S, 2)
    M, ST, lo, hi = (np.full(S, -1.0) for _ in range(4))
    ns, n, gains = np.full(S, -1, np.int32), np.full(S, -1, np.int32), np.full(S, -1, np.float32)
    powers = np.full((S, max(max_blocks, 1)), np.nan)
    _check(lib, lib.smst_debug_clip_loudness_range(device, S, channels, seg.ctypes.data_as(_ip), C.c_void_p(image.ctypes.data), image_ss, image_cs, rates.ctypes.data_as(_dp),
                                                   None if w is None else w.ctypes.data_as(_fp), float(target), None if k is None else k.ctypes.data_as(_dp),
                                                   M.ctypes.data_as(_dp), ST.ctypes.data_as(_dp), lo.ctypes.data_as(_dp), hi.ctypes.data_as(_dp), ns.ctypes.data_as(_ip),
                                                   n.ctypes.data_as(_ip), gains.ctypes.data_as(_fp), powers.ctypes.data_as(_dp), max_blocks))
    return M, ST, lo, hi, ns, n, gains, powers[:, :max_blocks]


def debug_clip_true_peak(segments, channels, image, image_ss, image_cs, flags=None, device=0, lib=None):
    """smst_debug_clip_true_peak on a numpy image (planar float32; segments int [S, 2, 4]; strides in floats; flags: [S], None: every stream)
    -> (true peaks, sample peaks), float32 [S]"""
    lib = lib if lib is not None else load_library()
    seg = np.ascontiguousarray(segments, np.int32)
    S = seg.shape[0]
    on = None if flags is None else np.ascontiguousarray(flags, np.int32)
    assert on is None or on.shape == (S,)
    true_peaks, sample_peaks = np.full(S, -1, np.float32), np.full(S, -1, np.float32)
    _check(lib, lib.smst_debug_clip_true_peak(device, S, channels, seg.ctypes.data_as(_ip), C.c_void_p(image.ctypes.data), image_ss, image_cs,
                                              true_peaks.ctypes.data_as(_fp), sample_peaks.ctypes.data_as(_fp), None if on is None else on.ctypes.data_as(_ip)))
    return true_peaks, sample_peaks


def debug_true_peak_taps(lib=None):
    """smst_debug_true_peak_taps -> float32 [3, 12]: the library's taps of the phases 1, 2, 3"""
    lib = lib if lib is not None else load_library()
    taps = np.zeros((3, 12), np.float32)
    _check(lib, lib.smst_debug_true_peak_taps(taps.ctypes.data_as(_fp)))
    return taps


def debug_clip_limit(segments, channels, image, image_ss, image_cs, gains, ceilings, flags, lookahead, max_frames, device=0, lib=None):
    """smst_debug_clip_limit on a numpy image (planar float32; segments int [S, 2, 4]; strides in floats; gains, ceilings, flags: [S], flags
    with bit 0 true peak and bit 1 limiter) -> (need, r: float32 [S, max_frames]; min gain: float32 [S]; limited frames: int64 [S])"""
    lib = lib if lib is not None else load_library()
    seg = np.ascontiguousarray(segments, np.int32)
    S = seg.shape[0]
    g, c, f = np.ascontiguousarray(gains, np.float32), np.ascontiguousarray(ceilings, np.float32), np.ascontiguousarray(flags, np.int32)
    assert g.shape == c.shape == f.shape == (S,)
    need, r = np.full((S, max_frames), -1, np.float32), np.full((S, max_frames), -1, np.float32)
    low, frames = np.full(S, -1, np.float32), np.full(S, -1, np.int64)
    _check(lib, lib.smst_debug_clip_limit(device, S, channels, seg.ctypes.data_as(_ip), C.c_void_p(image.ctypes.data), image_ss, image_cs,
                                          g.ctypes.data_as(_fp), c.ctypes.data_as(_fp), f.ctypes.data_as(_ip), int(lookahead),
                                          need.ctypes.data_as(_fp), r.ctypes.data_as(_fp), int(max_frames), low.ctypes.data_as(_fp),
                                          frames.ctypes.data_as(C.POINTER(_ll))))
    return need, r, low, frames


def debug_limiter_window(lookahead, lib=None):
    """smst_debug_limiter_window -> float32 [2*lookahead + 1]: the library's smoothing window"""
    lib = lib if lib is not None else load_library()
    win = np.zeros(2*int(lookahead) + 1, np.float32)
    _check(lib, lib.smst_debug_limiter_window(int(lookahead), win.ctypes.data_as(_fp)))
    return win


def debug_pcm_stream_limit(counts, channels, image, image_ss, image_cs, gains, ceilings, flags, lookahead, max_frames, device=0, lib=None):
    """smst_debug_pcm_stream_limit on a numpy image (planar float32 that holds each stream's frames in order; strides in floats; counts int
    [calls, S], negative: the stream takes no part in that call; gains, ceilings, flags: [S], flags 1 = the setting on, 3 = with the true-peak
    detector, 2H + 6 frames late) -> (r: float32
    [S, max_frames] as written; frames: float32 [S, max_frames, channels], the F32 output; min gain: float32 [S]; limited frames: int64 [S])"""
    lib = lib if lib is not None else load_library()
    g, c, f = np.ascontiguousarray(gains, np.float32), np.ascontiguousarray(ceilings, np.float32), np.ascontiguousarray(flags, np.int32)
    S = g.shape[0]
    n = np.ascontiguousarray(counts, np.int32).reshape(-1, S)
    assert g.shape == c.shape == f.shape == (S,)
    r, frames = np.full((S, max_frames), -1, np.float32), np.full((S, max_frames, channels), -1, np.float32)
    low, limited = np.full(S, -1, np.float32), np.full(S, -1, np.int64)
    _check(lib, lib.smst_debug_pcm_stream_limit(device, S, channels, n.shape[0], n.ctypes.data_as(_ip), C.c_void_p(image.ctypes.data), image_ss, image_cs,
                                                g.ctypes.data_as(_fp), c.ctypes.data_as(_fp), f.ctypes.data_as(_ip), int(lookahead),
                                                r.ctypes.data_as(_fp), frames.ctypes.data_as(_fp), int(max_frames), low.ctypes.data_as(_fp),
                                                limited.ctypes.data_as(C.POINTER(_ll))))
    return r, frames, low, limited


def debug_pcm_stream_meter(counts, channels, image, image_ss, image_cs, sample_rates, max_sub_blocks, weights=None, flags=None, read_after=None, form=0,
                           max_blocks=0, device=0, lib=None):
    """smst_debug_pcm_stream_meter on a numpy image (planar float32 that holds each stream's frames in order; strides in floats; counts int
    [calls, S], negative: the stream takes no part in that call; read_after: [calls] or None -- a reading after the last call only)
    -> a dict of arrays, reading-major [R, S]: Z, M, ST, lo, hi (powers, float64), blocks, gated, ns, n (int32), true_peaks, sample_peaks
    (float32), metered (int64); block_powers, short_powers: float64 [S, max_blocks] of the LAST reading, NaN behind a stream's last one"""
    lib = lib if lib is not None else load_library()
    rates = np.ascontiguousarray(np.asarray(sample_rates, np.float64).reshape(-1))
    S = rates.shape[0]
    n = np.ascontiguousarray(counts, np.int32).reshape(-1, S)
    calls = n.shape[0]
    after = None if read_after is None else np.ascontiguousarray(read_after, np.int32)
    assert after is None or after.shape == (calls,)
    R = 1 if after is None else int(np.count_nonzero(after))
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    assert w is None or w.shape == (channels,)
    on = None if flags is None else np.ascontiguousarray(flags, np.int32)
    assert on is None or on.shape == (S,)
    f64 = {k: np.full((max(R, 1), S), -1.0) for k in ("Z", "M", "ST", "lo", "hi")}
    i32 = {k: np.full((max(R, 1), S), -1, np.int32) for k in ("blocks", "gated", "ns", "n")}
    f32 = {k: np.full((max(R, 1), S), -1, np.float32) for k in ("true_peaks", "sample_peaks")}
    metered = np.full((max(R, 1), S), -1, np.int64)
    block_powers, short_powers = np.full((S, max(max_blocks, 1)), np.nan), np.full((S, max(max_blocks, 1)), np.nan)
    d, i, f = (lambda a: a.ctypes.data_as(_dp)), (lambda a: a.ctypes.data_as(_ip)), (lambda a: a.ctypes.data_as(_fp))
    _check(lib, lib.smst_debug_pcm_stream_meter(device, S, channels, calls, i(n), None if after is None else i(after), int(form), C.c_void_p(image.ctypes.data), image_ss, image_cs,
                                                d(rates), None if w is None else f(w), None if on is None else i(on), int(max_sub_blocks),
                                                d(f64["Z"]), i(i32["blocks"]), i(i32["gated"]), d(f64["M"]), d(f64["ST"]), d(f64["lo"]), d(f64["hi"]), i(i32["ns"]), i(i32["n"]),
                                                f(f32["true_peaks"]), f(f32["sample_peaks"]), metered.ctypes.data_as(C.POINTER(_ll)), d(block_powers), d(short_powers), int(max_blocks)))
    out = dict(f64, **i32, **f32)
    out = {k: v[:R] for k, v in out.items()}
    out.update(metered=metered[:R], block_powers=block_powers[:, :max_blocks], short_powers=short_powers[:, :max_blocks])
    return out


def resample_ratio(from_rate, to_rate, lib=None):
    """smst_resample_ratio -> (up, down): the reduced ratio to_rate/from_rate of two integer-valued sample rates"""
    lib = lib if lib is not None else load_library()
    up, down = C.c_int(0), C.c_int(0)
    _check(lib, lib.smst_resample_ratio(float(from_rate), float(to_rate), C.byref(up), C.byref(down)))
    return up.value, down.value


def debug_resample_taps(up, down, lib=None):
    """smst_debug_resample_taps -> float32 [L, T]: the library's table of the (reduced) ratio up/down, phase-major"""
    lib = lib if lib is not None else load_library()
    g = math.gcd(int(up), int(down)) if int(up) > 0 and int(down) > 0 else 1
    taps = C.c_int(0)
    _check(lib, lib.smst_debug_resample_taps(int(up), int(down), None, C.byref(taps)))
    table = np.zeros((int(up)//g, taps.value), np.float32)
    _check(lib, lib.smst_debug_resample_taps(int(up), int(down), table.ctypes.data_as(_fp), C.byref(taps)))
    return table


def debug_pcm_stream_resample(counts, ratios, channels, image, image_ss, image_cs, out, out_ss, out_cs, max_frames, fed0=None, device=0, lib=None):
    """smst_debug_pcm_stream_resample on numpy buffers (planar float32, 1-d views whose first element is the first stream's first row; strides
    in floats).  counts: int [calls, S], negative = no part; ratios: [S] of (up, down); fed0: [S] int64 or None.  ``out`` is written in
    place -> made, int64 [S]: the frames written per stream"""
    lib = lib or load_library()
    n = np.ascontiguousarray(np.asarray(counts, np.int32))
    calls, S = n.shape
    r = np.ascontiguousarray(np.asarray(ratios, np.int32).reshape(S, 2))
    start = None if fed0 is None else np.ascontiguousarray(np.asarray(fed0, np.int64).reshape(S))
    made = np.zeros(S, np.int64)
    _check(lib, lib.smst_debug_pcm_stream_resample(device, S, channels, calls, n.ctypes.data_as(_ip), r.ctypes.data_as(_ip),
                                                   None if start is None else start.ctypes.data_as(C.POINTER(_ll)), C.c_void_p(image.ctypes.data), image_ss, image_cs,
                                                   C.c_void_p(out.ctypes.data), out_ss, out_cs, int(max_frames), made.ctypes.data_as(C.POINTER(_ll))))
    return made


def debug_pcm_stream_resample_out(counts, ratios, channels, image, image_ss, image_cs, out, out_ss, out_cs, max_frames, delivered0=None, device=0, lib=None):
    """smst_debug_pcm_stream_resample_out on numpy buffers (planar float32, 1-d views whose first element is the first stream's first row;
    strides in floats).  counts: int [calls, S] delivered frames, negative = no part; ratios: [S] of (up, down); delivered0: [S] int64 or
    None.  ``out`` is written in place -> rendered, int64 [S]: the frames of ``image`` consumed per stream"""
    lib = lib or load_library()
    n = np.ascontiguousarray(np.asarray(counts, np.int32))
    calls, S = n.shape
    r = np.ascontiguousarray(np.asarray(ratios, np.int32).reshape(S, 2))
    start = None if delivered0 is None else np.ascontiguousarray(np.asarray(delivered0, np.int64).reshape(S))
    rendered = np.zeros(S, np.int64)
    _check(lib, lib.smst_debug_pcm_stream_resample_out(device, S, channels, calls, n.ctypes.data_as(_ip), r.ctypes.data_as(_ip),
                                                       None if start is None else start.ctypes.data_as(C.POINTER(_ll)), C.c_void_p(image.ctypes.data), image_ss, image_cs,
                                                       C.c_void_p(out.ctypes.data), out_ss, out_cs, int(max_frames), rendered.ctypes.data_as(C.POINTER(_ll))))
    return rendered


def debug_clip_resample(counts, ratios, channels, image, image_ss, image_cs, segments, out, out_ss, out_cs, device=0, lib=None):
    """smst_debug_clip_resample on numpy buffers (planar float32, 1-d views whose first element is the first stream's first row; strides in
    floats; counts int [S]; ratios int [S, 2]; segments int [S, 2, 4], the destination).  ``out`` is written in place and returned."""
    lib = lib if lib is not None else load_library()
    n, r, seg = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(ratios, np.int32), np.ascontiguousarray(segments, np.int32)
    S = n.shape[0]
    assert r.shape == (S, 2) and seg.shape == (S, 2, 4)
    assert image.dtype == np.float32 and out.dtype == np.float32 and image.ndim == 1 and out.ndim == 1 and image.strides[0] == 4 and out.strides[0] == 4
    assert image.size >= (S - 1)*image_ss + (channels - 1)*image_cs + int(n.max(initial=0))
    assert out.size >= (S - 1)*out_ss + (channels - 1)*out_cs + int((seg[:, :, 1] + seg[:, :, 2]).max(initial=0))
    _check(lib, lib.smst_debug_clip_resample(device, S, channels, n.ctypes.data_as(_ip), r.ctypes.data_as(_ip), C.c_void_p(image.ctypes.data), image_ss, image_cs,
                                             seg.ctypes.data_as(_ip), C.c_void_p(out.ctypes.data), out_ss, out_cs))
    return out


def debug_clip_resample_out(counts, ratios, channels, image, image_ss, image_cs, src_segments, dst_segments, out, out_ss, out_cs, device=0, lib=None):
    """smst_debug_clip_resample_out on numpy buffers (planar float32, 1-d views whose first element is the first stream's first row; strides
    in floats; counts int [S], the delivered frames Nd; ratios int [S, 2]; src_segments int [S, 2, 4], where the E rendered frames lie in
    ``image``; dst_segments int [S, 2, 4], the destination).  ``out`` is written in place and returned."""
    lib = lib if lib is not None else load_library()
    n, r = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(ratios, np.int32)
    src, dst = np.ascontiguousarray(src_segments, np.int32), np.ascontiguousarray(dst_segments, np.int32)
    S = n.shape[0]
    assert r.shape == (S, 2) and src.shape == (S, 2, 4) and dst.shape == (S, 2, 4)
    assert image.dtype == np.float32 and out.dtype == np.float32 and image.ndim == 1 and out.ndim == 1 and image.strides[0] == 4 and out.strides[0] == 4
    assert image.size >= (S - 1)*image_ss + (channels - 1)*image_cs + int((src[:, :, 0] + src[:, :, 2]).max(initial=0))
    assert out.size >= (S - 1)*out_ss + (channels - 1)*out_cs + int((dst[:, :, 1] + dst[:, :, 2]).max(initial=0))
    _check(lib, lib.smst_debug_clip_resample_out(device, S, channels, n.ctypes.data_as(_ip), r.ctypes.data_as(_ip), C.c_void_p(image.ctypes.data), image_ss, image_cs,
                                                 src.ctypes.data_as(_ip), dst.ctypes.data_as(_ip), C.c_void_p(out.ctypes.data), out_ss, out_cs))
    return out


def launch_count(name, lib=None):
    """Launches of one kernel variant since the library was loaded (test hook, smst_debug_launch_count)."""
    lib = lib if lib is not None else load_library()
    return int(lib.smst_debug_launch_count(name.encode()))


class StretchBatch:
    """S independent streams with one configuration on one GPU (C ABI group 2 of include/smst.h).

    Buffers are [S, C, n] float32: numpy arrays (host memory, staged by the library) or CUDA/HIP torch tensors
    (device memory, zero-copy).  Each stream behaves like one reference ``SignalsmithStretch<float>`` instance.
    """

    def __init__(self, streams, channels, block=None, interval=None, split=None, preset=None, sample_rate=None,
                 device=0, seed=0, lib=None, half_state=False):
        """half_state: store the carried per-bin state and the overlap-add sums in fp16 (SMST_FLAG_HALF_STATE, include/smst.h)."""
        self.lib = lib if lib is not None else load_library()
        h = C.c_void_p()
        flags = 1 if half_state else 0
        if preset is not None:
            code = {"default": 0, "cheaper": 1}[preset]
            rc = self.lib.smst_batch_create_preset_ex(C.byref(h), streams, channels, code, float(sample_rate),
                                                      -1 if split is None else int(split), device, seed, flags)
        else:
            rc = self.lib.smst_batch_create_ex(C.byref(h), streams, channels, int(block), int(interval), int(bool(split)), device, seed, flags)
        _check(self.lib, rc)
        self.h = h
        self.streams, self.channels, self.device = streams, channels, device

    def close(self):
        if getattr(self, "h", None):
            self.lib.smst_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- queries (reference names)
    def blockSamples(self): return self.lib.smst_batch_block_samples(self.h)
    def intervalSamples(self): return self.lib.smst_batch_interval_samples(self.h)
    def fftSamples(self): return self.lib.smst_batch_fft_samples(self.h)
    def bands(self): return self.lib.smst_batch_bands(self.h)
    def inputLatency(self): return self.lib.smst_batch_input_latency(self.h)
    def outputLatency(self): return self.lib.smst_batch_output_latency(self.h)
    def seekLength(self): return self.lib.smst_batch_seek_length(self.h)
    def outputSeekLength(self, rate): return self.lib.smst_batch_output_seek_length(self.h, rate)
    def workspaceBytes(self): return self.lib.smst_batch_workspace_bytes(self.h)

    def reset(self): _check(self.lib, self.lib.smst_batch_reset(self.h))
    def setTransposeFactor(self, m, tonality=0.0, stream=-1): _check(self.lib, self.lib.smst_batch_set_transpose_factor(self.h, stream, m, tonality))
    def setTransposeSemitones(self, s, tonality=0.0, stream=-1): _check(self.lib, self.lib.smst_batch_set_transpose_semitones(self.h, stream, s, tonality))
    def setFormantFactor(self, m, comp=False, stream=-1): _check(self.lib, self.lib.smst_batch_set_formant_factor(self.h, stream, m, int(comp)))
    def setFormantSemitones(self, s, comp=False, stream=-1): _check(self.lib, self.lib.smst_batch_set_formant_semitones(self.h, stream, s, int(comp)))
    def setFormantBase(self, f=0.0, stream=-1): _check(self.lib, self.lib.smst_batch_set_formant_base(self.h, stream, f))

    def setFreqMapTable(self, table, stream=-1):
        if table is None:
            _check(self.lib, self.lib.smst_batch_set_freq_map_table(self.h, stream, None, 0))
        else:
            t = np.ascontiguousarray(table, np.float32)
            _check(self.lib, self.lib.smst_batch_set_freq_map_table(self.h, stream, t.ctypes.data_as(_fp), len(t)))

    def synchronize(self):
        _check(self.lib, self.lib.smst_batch_synchronize(self.h))
        self._inflight = []

    def _order_after_torch(self, *tensors, wait=True):
        """Device-memory calls are asynchronous on the batch's own HIP streams.  Order them after the producer (torch's
        current stream) with an event -- no host synchronisation -- and keep the tensors referenced until the batch's
        stream has drained, so torch's caching allocator cannot recycle their memory while our kernels still use it."""
        import torch
        if wait:
            _check(self.lib, self.lib.smst_batch_wait_for_stream(self.h, C.c_void_p(torch.cuda.current_stream(tensors[0].device).cuda_stream)))
        inflight = getattr(self, "_inflight", [])
        if len(inflight) >= 16:
            self.synchronize()
            inflight = []
        inflight.append(tensors)
        self._inflight = inflight

    def enableProfiling(self, mode=1): _check(self.lib, self.lib.smst_batch_enable_profiling(self.h, int(mode)))

    def takeHostTimes(self):
        """Host time of process() since the last take: dict(call_ms, wait_tables_ms, wait_gate_ms, work_ms, calls) -- see include/smst.h"""
        ms = (C.c_double*3)()
        n = _ll(0)
        _check(self.lib, self.lib.smst_batch_take_host_times(self.h, ms, C.byref(n)))
        return dict(call_ms=ms[0], wait_tables_ms=ms[1], wait_gate_ms=ms[2], work_ms=ms[0] - ms[1] - ms[2], calls=int(n.value))

    def takeTimings(self):
        ms = (C.c_double*8)()
        n = (_ll*6)()
        _check(self.lib, self.lib.smst_batch_take_timings(self.h, ms, n))
        keys = ["analyse", "feed", "predict", "chain", "synth", "emit", "other", "chain_live"]
        lk = ["analyse", "predict", "chain", "synth", "emit", "chain_live"]
        return dict(zip(keys, list(ms))), dict(zip(lk, list(n)))

    # --- buffers
    def _describe(self, x, what):
        """-> (pointer, streamStride, channelStride, length, memory, keepalive)"""
        if _is_torch(x):
            if x.dim() != 3 or x.shape[0] != self.streams or x.shape[1] != self.channels:
                raise StretchError("%s must be [S, C, n]" % what)
            if str(x.dtype) != "torch.float32" or not x.is_cuda or x.stride(2) != 1:
                raise StretchError("%s: need a float32 GPU tensor with contiguous samples" % what)
            return C.c_void_p(x.data_ptr()), x.stride(0), x.stride(1), x.shape[2], MEM_DEVICE, x
        a = np.asarray(x, dtype=np.float32)
        if a.ndim != 3 or a.shape[0] != self.streams or a.shape[1] != self.channels:
            raise StretchError("%s must be [S, C, n]" % what)
        a = np.ascontiguousarray(a)
        return C.c_void_p(a.ctypes.data), a.shape[1]*a.shape[2], a.shape[2], a.shape[2], MEM_HOST, a

    # --- interleaved PCM frames (smst_batch_*_pcm): [S, n, C] of int16, int32, float16 or float32, or packed int24 as uint8 [S, n, C, 3];
    # the same dtype and layout back
    def _describe_frames(self, x, what):
        """-> (pointer, streamStride, frameStride, frames, format, memory, keepalive); strides in elements.

        Frames are [S, n, C] of int16, int32, float16 or float32, or -- packed 24-bit, SMST_PCM_S24 -- uint8 of shape [S, n, C, 3]: three
        little-endian bytes per sample.  numpy arrays are host memory, torch GPU tensors device memory.  The channels of a frame (and the
        bytes of a 24-bit sample) must be contiguous; the stream and frame strides are free -- whole elements, so multiples of 3 bytes
        for packed int24, which needs no alignment beyond the byte."""
        torch_x = _is_torch(x)
        a = x if torch_x else np.asarray(x)
        name = str(a.dtype).replace("torch.", "")
        ndim = a.dim() if torch_x else a.ndim
        s24 = name == "uint8" and ndim == 4 and a.shape[3] == 3
        fmt = PCM_S24 if s24 else _FRAME_DTYPES.get(name)
        if fmt is None:
            raise StretchError("%s: frames are int16, int32, float16 or float32 [S, n, C], or uint8 [S, n, C, 3] (packed int24)" % what)
        if ndim != (4 if s24 else 3) or a.shape[0] != self.streams or a.shape[2] != self.channels:
            raise StretchError("%s must be [S, n, C]%s" % (what, " x 3 bytes" if s24 else ""))
        if torch_x:
            if not x.is_cuda or x.stride(ndim - 1) != 1 or (s24 and x.stride(2) != 3):
                raise StretchError("%s: need a GPU tensor with contiguous channels" % what)
            if s24 and (x.stride(0) % 3 or x.stride(1) % 3):
                raise StretchError("%s: the stream and frame strides of packed int24 frames must be multiples of 3 bytes" % what)
            unit = 3 if s24 else 1
            return C.c_void_p(x.data_ptr()), x.stride(0)//unit, x.stride(1)//unit, x.shape[1], fmt, MEM_DEVICE, x
        if s24:
            if a.size and (a.strides[3] != 1 or a.strides[2] != 3):
                a = np.ascontiguousarray(a)
            if a.size and (a.strides[0] % 3 or a.strides[1] % 3 or a.strides[0] < 0 or a.strides[1] < 3*a.shape[2]):
                raise StretchError("%s: the stream and frame strides of packed int24 frames must be multiples of 3 bytes" % what)
            if a.size == 0:
                return C.c_void_p(a.ctypes.data), a.shape[1]*a.shape[2], a.shape[2], a.shape[1], fmt, MEM_HOST, a
            return C.c_void_p(a.ctypes.data), a.strides[0]//3, a.strides[1]//3, a.shape[1], fmt, MEM_HOST, a
        if a.size and (a.strides[2] != a.itemsize or a.strides[0] % a.itemsize or a.strides[1] % a.itemsize or a.strides[0] < 0 or a.strides[1] < a.itemsize*a.shape[2]):
            a = np.ascontiguousarray(a)
        if a.size == 0:  # (numpy gives an empty array zero strides)
            return C.c_void_p(a.ctypes.data), a.shape[1]*a.shape[2], a.shape[2], a.shape[1], fmt, MEM_HOST, a
        return C.c_void_p(a.ctypes.data), a.strides[0]//a.itemsize, a.strides[1]//a.itemsize, a.shape[1], fmt, MEM_HOST, a

    def _new_frames(self, frames, fmt, like):
        shape = (self.streams, frames, self.channels) + ((3,) if fmt == PCM_S24 else ())
        if like is not None and _is_torch(like):
            import torch
            return torch.zeros(shape, dtype=getattr(torch, _FRAME_DTYPE_OF[fmt]), device=like.device)
        return np.zeros(shape, _FRAME_DTYPE_OF[fmt])

    # --- the calls: each on planar buffers (frames False, format None) or on frames -- the same body, _describe against _describe_frames and
    # smst_batch_<name> against smst_batch_<name>_pcm
    def _describe_any(self, frames, x, what):
        """-> (pointer, streamStride, channelStride | frameStride, length, format | None, memory, keepalive)"""
        if frames:
            return self._describe_frames(x, what)
        ptr, ss, cs, n, mem, keep = self._describe(x, what)
        return ptr, ss, cs, n, None, mem, keep

    def _new_out(self, n, fmt, like):
        """zeros for n samples per stream: frames of format fmt, planar float32 [S, C, n] for None; a torch tensor beside ``like`` if that is one"""
        if fmt is not None:
            return self._new_frames(n, fmt, like)
        if like is not None and _is_torch(like):
            import torch
            return torch.zeros((self.streams, self.channels, n), dtype=torch.float32, device=like.device)
        return np.zeros((self.streams, self.channels, n), np.float32)

    def _batch_call(self, name, fmt, mem, *args):
        fn = getattr(self.lib, "smst_batch_" + name + ("" if fmt is None else "_pcm"))
        _check(self.lib, fn(self.h, *args, mem) if fmt is None else fn(self.h, *args, fmt, mem))

    def _signal_torch(self, out):
        """torch ops on ``out`` issued from here on are ordered after our kernels (no host sync either)"""
        import torch
        _check(self.lib, self.lib.smst_batch_signal_stream(self.h, C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)))

    def _process(self, frames, x, out_samples, in_samples, out, ordered):
        S = self.streams
        ptr, ss, inner, n, fmt, mem, keep = self._describe_any(frames, x, "input")
        nin, pin = _int_array(n if in_samples is None else in_samples, S)
        nout, pout = _int_array(out_samples, S)
        max_out = max(int(nout.max()), 1)
        if out is None:
            out = self._new_out(max_out, fmt, x if mem == MEM_DEVICE else None)
        optr, oss, oinner, on, ofmt, omem, okeep = self._describe_any(frames, out, "output")
        if frames:
            if omem != mem or ofmt != fmt:
                raise StretchError("input and output must have the same format and live in the same memory space")
            if omem == MEM_HOST and okeep is not out:
                raise StretchError("output: need an array the library can write in place")
        elif omem != mem:
            raise StretchError("input and output must live in the same memory space")
        if on < max_out or int(nin.max()) > n:
            raise StretchError("buffer shorter than the requested sample count")
        if mem == MEM_DEVICE and ordered:
            self._order_after_torch(x, out)
        # (ordered=False: the caller's contract -- inputs complete, outputs untouched and both tensors ALIVE until it synchronises the batch -- so
        # nothing is tracked here.  Until round 6 the tensors were still put on the in-flight list, whose every 17th entry synchronises the batch:
        # one pipeline drain per 16 calls, 2.4 ms of the bench's 17th step -- bench.py's per-step periods showed it, roofline.step_ms.in_order)
        self._batch_call("process", fmt, mem, ptr, ss, inner, pin, optr, oss, oinner, pout)
        if mem == MEM_DEVICE and ordered:
            self._signal_torch(out)
        return out

    def _seek(self, name, frames, x, counts, *rates):
        """seek (rates: the double array) and outputSeek (none)"""
        ptr, ss, inner, n, fmt, mem, keep = self._describe_any(frames, x, "input")
        nin, pin = _int_array(n if counts is None else counts, self.streams)
        if mem == MEM_DEVICE:
            self._order_after_torch(x)
        self._batch_call(name, fmt, mem, ptr, ss, inner, pin, *rates)

    def _rates(self, rates, dtype, pointer):
        """one rate per stream (a scalar: the same for all) -> the pointer (which keeps the array alive)"""
        return np.ascontiguousarray(np.broadcast_to(np.asarray(rates, dtype=dtype), (self.streams,))).ctypes.data_as(pointer)

    def _flush(self, fmt, out_samples, rates, like):
        nout, pout = _int_array(out_samples, self.streams)
        out = self._new_out(max(int(nout.max()), 1), fmt, like)
        optr, oss, oinner, on, ofmt, omem, okeep = self._describe_any(fmt is not None, out, "output")
        self._batch_call("flush", fmt, omem, optr, oss, oinner, pout, self._rates(rates, np.float32, _fp))
        if omem == MEM_DEVICE:
            self.synchronize()
        return out

    def process(self, x, out_samples, in_samples=None, out=None, ordered=True):
        """process(inputs, inputSamples, outputs, outputSamples) for every stream (signalsmith-stretch.h:210).

        Device tensors: with ``ordered`` (default) the call is ordered after torch's current stream (the producer of ``x``) and
        torch's current stream is ordered after it (consumers of the result) -- by events, without a host synchronisation.
        That makes consecutive calls wait for each other through torch's stream.  A caller whose inputs are already
        complete and who synchronises the batch itself before touching the outputs (``bench.py``) passes
        ``ordered=False`` and keeps the overlap of call n+1's host scheduling with call n's kernels."""
        return self._process(False, x, out_samples, in_samples, out, ordered)

    def seek(self, x, rates, in_samples=None):
        self._seek("seek", False, x, in_samples, self._rates(rates, np.float64, _dp))

    def flush(self, out_samples, rates=0.0, like=None):
        """flush() of every stream with a non-negative count; a negative count leaves that stream alone (include/smst.h)"""
        return self._flush(None, out_samples, rates, like)

    def outputSeek(self, x, input_lengths=None):
        self._seek("output_seek", False, x, input_lengths)

    def processFrames(self, x, out_samples, in_samples=None, out=None, ordered=True):
        """process() on interleaved frames: x is [S, n, C] int16 (full scale 32768), int32 (2^31), float16 or float32, or uint8
        [S, n, C, 3] for packed int24 (8388608), numpy (host memory) or a torch GPU tensor (_describe_frames has the layout rules); the
        result has the same dtype and shape convention.  Integer output is round-to-nearest, ties away from zero, clamped, no dither
        unless setPcmDither() turned it on (int16 / int24);
        NaN -> 0.  int32 input above 2^24 is rounded to float32.  float16 output is round-to-nearest-even: subnormals kept, 65520 and
        above +-inf, NaN stays NaN (include/smst.h).  What was clamped: takePcmOvers().  ``ordered`` as in process()."""
        return self._process(True, x, out_samples, in_samples, out, ordered)

    def seekFrames(self, x, rates, in_samples=None):
        self._seek("seek", True, x, in_samples, self._rates(rates, np.float64, _dp))

    def flushFrames(self, out_samples, rates=0.0, like=None, dtype=np.int16):
        """flush() into [S, n, C] frames of ``dtype`` (int16, int32, float16 or float32), or with dtype="s24" into uint8 [S, n, C, 3]
        (packed int24); a negative count leaves that stream alone"""
        fmt = PCM_S24 if isinstance(dtype, str) and dtype.lower() == "s24" else _FRAME_DTYPES.get(np.dtype(dtype).name)
        if fmt is None:
            raise StretchError("frames are int16, int32, float16, float32 or \"s24\"")
        return self._flush(fmt, out_samples, rates, like)

    def outputSeekFrames(self, x, input_lengths=None):
        self._seek("output_seek", True, x, input_lengths)

    # --- whole clips (smst_batch_exact / smst_batch_exact_pcm): S clips of S lengths and S rates in one call
    def _exact(self, frames, x, out_samples, in_samples, out, ordered):
        S = self.streams
        ptr, ss, inner, n, fmt, mem, keep = self._describe_any(frames, x, "input")
        nin, pin = _int_array(n if in_samples is None else in_samples, S)
        nout, pout = _int_array(out_samples, S)
        max_out = max(int(nout.max()), 1)
        if out is None:
            out = self._new_out(max_out, fmt, x if mem == MEM_DEVICE else None)
        optr, oss, oinner, on, ofmt, omem, okeep = self._describe_any(frames, out, "output")
        if omem != mem or ofmt != fmt:
            raise StretchError("input and output must have the same format and live in the same memory space")
        if omem == MEM_HOST and okeep is not out:
            raise StretchError("output: need an array the library can write in place")
        if on < max_out or int(nin[nout >= 0].max(initial=0)) > n:
            raise StretchError("buffer shorter than the requested sample count")
        status = np.full(S, 1, np.int32)                        # (a stream that is left out keeps the 1)
        if mem == MEM_DEVICE and ordered:
            self._order_after_torch(x, out)
        self._batch_call("exact", fmt, mem, ptr, ss, inner, pin, optr, oss, oinner, pout, status.ctypes.data_as(_ip))
        if mem == MEM_DEVICE and ordered:
            self._signal_torch(out)
        return out, status == 0

    def exact(self, x, out_samples, in_samples=None, out=None, ordered=True):
        """exact() of every stream (signalsmith-stretch.h:468-491): stream s, a fresh run of instance seed+s, turns its whole clip
        x[s, :, :in_samples[s]] into exactly out_samples[s] samples -- lengths and rates are each stream's own, one call for all.
        -> (out [S, C, max(out_samples)], ok bool [S]); ok[s] is False for a stream whose clip is shorter than outputSeekLength(rate_s)
        (its output is zeros, its state untouched) and for one left out of the call by a NEGATIVE out_samples[s] (nothing of it is
        touched).  numpy arrays are host memory, torch GPU tensors device memory; ``ordered`` as in process()."""
        return self._exact(False, x, out_samples, in_samples, out, ordered)

    def exactFrames(self, x, out_samples, in_samples=None, out=None, ordered=True):
        """exact() on interleaved frames ([S, n, C] of a frame dtype, or uint8 [S, n, C, 3]: processFrames has the rules) -> (out, ok)"""
        return self._exact(True, x, out_samples, in_samples, out, ordered)

    def setPcmDither(self, mode, seed=0, stream=-1):
        """TPDF dither of the int16 / int24 output of processFrames, flushFrames and exactFrames (include/smst.h, "Dither"): DITHER_NONE,
        DITHER_TPDF (white) or DITHER_TPDF_HP (lag-1 correlation -1/2).  stream = -1: every stream, stream s with seed + s.  The frame
        counter of the stream(s) restarts at 0; the other formats are not affected."""
        _check(self.lib, self.lib.smst_batch_set_pcm_dither(self.h, int(stream), int(mode), int(seed)))

    def pcmDither(self, stream):
        """-> (mode, seed, frames): the stream's dither mode, its seed and its frame counter"""
        mode, seed, frames = C.c_int(0), _ll(0), _ll(0)
        _check(self.lib, self.lib.smst_batch_pcm_dither(self.h, int(stream), C.byref(mode), C.byref(seed), C.byref(frames)))
        return mode.value, seed.value, frames.value

    def takePcmOvers(self):
        """-> (clamped, nans), int64 [S]: per stream, the output elements of processFrames / flushFrames since the last take whose code
        the clamp set (integer formats) or that became +-inf from a finite value (float16), and those whose input was NaN (every
        format).  Synchronises the batch and clears the counters."""
        clamped, nans = np.zeros(self.streams, np.int64), np.zeros(self.streams, np.int64)
        _check(self.lib, self.lib.smst_batch_take_pcm_overs(self.h, clamped.ctypes.data_as(C.POINTER(_ll)), nans.ctypes.data_as(C.POINTER(_ll))))
        self._inflight = []
        return clamped, nans

    def set_pcm_level(self, mode, gain=1.0, ceiling=1.0, stream=-1):
        """Level of the frame output (include/smst.h, "Level"): LEVEL_FIXED (w = v*gain in processFrames, flushFrames and exactFrames) or, for
        exactFrames only, LEVEL_PROTECT (the gain, lowered to ceiling/peak where the clip would exceed the ceiling) and LEVEL_NORMALISE
        (ceiling/peak), peak being the clip's own.  stream = -1: every stream.  The batch uses the levelled kernels from the first call on."""
        _check(self.lib, self.lib.smst_batch_set_pcm_level(self.h, int(stream), int(mode), float(gain), float(ceiling)))

    def pcm_level(self, stream):
        """-> (mode, gain, ceiling) of the stream"""
        mode, gain, ceiling = C.c_int(0), C.c_float(0), C.c_float(0)
        _check(self.lib, self.lib.smst_batch_pcm_level(self.h, int(stream), C.byref(mode), C.byref(gain), C.byref(ceiling)))
        return mode.value, gain.value, ceiling.value

    def take_pcm_peaks(self):
        """-> (peaks, gains), float32 [S]: per stream, the largest |v| the levelled frame conversions met before the gain since the last take
        (NaN skipped; 0 if none) and the gain the newest one applied (1 before any).  Synchronises the batch and clears the peaks."""
        peaks, gains = np.zeros(self.streams, np.float32), np.zeros(self.streams, np.float32)
        _check(self.lib, self.lib.smst_batch_take_pcm_peaks(self.h, peaks.ctypes.data_as(_fp), gains.ctypes.data_as(_fp)))
        self._inflight = []
        return peaks, gains

    def set_pcm_loudness(self, target_lufs, ceiling=float("inf"), sample_rate=48000.0, stream=-1):
        """LEVEL_LOUDNESS (include/smst.h, "Loudness"), exactFrames only: the clip's ITU-R BS.1770-4 integrated loudness is measured on the
        device at ``sample_rate`` -- the rate of the OUTPUT clip -- and the clip brought to ``target_lufs``, the gain lowered to ceiling/peak
        where the clip would exceed the ceiling (inf: no limit).  stream = -1: every stream."""
        _check(self.lib, self.lib.smst_batch_set_pcm_loudness(self.h, int(stream), float(target_lufs), float(ceiling), float(sample_rate)))

    def pcm_loudness(self, stream):
        """-> (target, sample_rate) of a stream in LEVEL_LOUDNESS"""
        target, rate = C.c_double(0), C.c_double(0)
        _check(self.lib, self.lib.smst_batch_pcm_loudness(self.h, int(stream), C.byref(target), C.byref(rate)))
        return target.value, rate.value

    def set_pcm_loudness_weights(self, weights=None):
        """the channel weights of the loudness measurement, [C] (None: 1 on every channel)"""
        if weights is None:
            _check(self.lib, self.lib.smst_batch_set_pcm_loudness_weights(self.h, None))
            return
        w = np.ascontiguousarray(weights, np.float32)
        if w.shape != (self.channels,):
            raise StretchError("one weight per channel")
        _check(self.lib, self.lib.smst_batch_set_pcm_loudness_weights(self.h, w.ctypes.data_as(_fp)))

    def set_pcm_loudness_range(self, on=True, sample_rate=48000.0, stream=-1):
        """The meter flag (include/smst.h, "Loudness range"), exactFrames only: the stream's maximum momentary and short-term loudness and its
        loudness range (EBU Tech 3341 / 3342) are measured on the device, whatever its level mode.  sample_rate is the OUTPUT clip's rate, used
        where the stream is not in LEVEL_LOUDNESS (which has a rate of its own).  stream = -1: every stream."""
        _check(self.lib, self.lib.smst_batch_set_pcm_loudness_range(self.h, int(stream), 1 if on else 0, float(sample_rate)))

    def pcm_loudness_range(self, stream):
        """-> (on, sample_rate) of a stream's meter flag"""
        on, rate = C.c_int(), C.c_double()
        _check(self.lib, self.lib.smst_batch_pcm_loudness_range(self.h, int(stream), C.byref(on), C.byref(rate)))
        return bool(on.value), rate.value

    def set_pcm_loudness_caps(self, max_momentary=float("inf"), max_short_term=float("inf"), stream=-1):
        """Caps in LUFS on the maximum momentary and short-term loudness of a LEVEL_LOUDNESS stream's clip (EBU R 128 s1): the gain is the
        lowest of the target's and the caps'.  inf: none.  A finite cap implies the meter; outside LEVEL_LOUDNESS a cap is inert."""
        _check(self.lib, self.lib.smst_batch_set_pcm_loudness_caps(self.h, int(stream), float(max_momentary), float(max_short_term)))

    def pcm_loudness_caps(self, stream):
        """-> (max_momentary, max_short_term) in LUFS, inf: none"""
        m, t = C.c_double(), C.c_double()
        _check(self.lib, self.lib.smst_batch_pcm_loudness_caps(self.h, int(stream), C.byref(m), C.byref(t)))
        return m.value, t.value

    def take_pcm_loudness_range(self):
        """-> (momentary_max, short_term_max in LUFS, range in LU, low, high in LUFS: float64 [S]; short_blocks, range_blocks: int32 [S]) of the
        newest exactFrames that metered (-inf, 0 and no blocks where the stream was not metered).  Synchronises; resets nothing."""
        S = self.streams
        m, t, lra, lo, hi = (np.zeros(S, np.float64) for _ in range(5))
        ns, n = np.zeros(S, np.int32), np.zeros(S, np.int32)
        _check(self.lib, self.lib.smst_batch_take_pcm_loudness_range(self.h, m.ctypes.data_as(_dp), t.ctypes.data_as(_dp), lra.ctypes.data_as(_dp), lo.ctypes.data_as(_dp),
                                                                     hi.ctypes.data_as(_dp), ns.ctypes.data_as(_ip), n.ctypes.data_as(_ip)))
        self._inflight = []
        return m, t, lra, lo, hi, ns, n

    def take_pcm_loudness(self):
        """-> (lufs float64 [S], blocks, gated int32 [S]) of the newest exactFrames that measured: the loudness (-inf where it was undefined or
        the stream was not measured), the blocks that passed the absolute gate and those that passed both.  Synchronises the batch."""
        lufs, blocks, gated = np.zeros(self.streams), np.zeros(self.streams, np.int32), np.zeros(self.streams, np.int32)
        _check(self.lib, self.lib.smst_batch_take_pcm_loudness(self.h, lufs.ctypes.data_as(_dp), blocks.ctypes.data_as(_ip), gated.ctypes.data_as(_ip)))
        self._inflight = []
        return lufs, blocks, gated

    def set_pcm_true_peak(self, on=True, stream=-1):
        """The true-peak flag (include/smst.h, "True peak"), exactFrames only: the clip's true peak -- a 4x interpolation between the samples,
        and the samples themselves -- is measured on the device, and the stream's whole-clip modes (LEVEL_PROTECT, LEVEL_NORMALISE,
        LEVEL_LOUDNESS) form ceiling/peak from it: their ceilings are then true-peak ceilings.  A LEVEL_FIXED stream is metered only.
        stream = -1: every stream.  set_pcm_level and set_pcm_loudness leave the flag as it is."""
        _check(self.lib, self.lib.smst_batch_set_pcm_true_peak(self.h, int(stream), 1 if on else 0))

    def pcm_true_peak(self, stream):
        """-> whether the stream has the true-peak flag"""
        on = C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_true_peak(self.h, int(stream), C.byref(on)))
        return bool(on.value)

    def take_pcm_true_peaks(self):
        """-> float32 [S]: the true peaks, before the gain, of the newest exactFrames that measured (0 for a stream it did not measure).
        Synchronises the batch; resets nothing."""
        peaks = np.zeros(self.streams, np.float32)
        _check(self.lib, self.lib.smst_batch_take_pcm_true_peaks(self.h, peaks.ctypes.data_as(_fp)))
        self._inflight = []
        return peaks

    def set_pcm_limiter(self, on=True, stream=-1):
        """The limiter flag (include/smst.h, "Limiter"), exactFrames only: a stream in LEVEL_PROTECT or LEVEL_LOUDNESS keeps its whole-clip
        gain -- the clip reaches its LUFS target -- and a lookahead limiter, on the device, brings the frames that would exceed the ceiling
        down to it (with the true-peak flag: the frames whose inter-sample values would).  Inert in the other two modes.  stream = -1: every
        stream.  set_pcm_level and set_pcm_loudness leave the flag as it is."""
        _check(self.lib, self.lib.smst_batch_set_pcm_limiter(self.h, int(stream), 1 if on else 0))

    def pcm_limiter(self, stream):
        """-> whether the stream has the limiter flag"""
        on = C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_limiter(self.h, int(stream), C.byref(on)))
        return bool(on.value)

    def set_pcm_limiter_lookahead(self, frames):
        """The batch's lookahead in frames, 1 ... LIMITER_MAX_LOOKAHEAD (default 72: 1.5 ms at 48 kHz)"""
        _check(self.lib, self.lib.smst_batch_set_pcm_limiter_lookahead(self.h, int(frames)))

    def pcm_limiter_lookahead(self):
        frames = C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_limiter_lookahead(self.h, C.byref(frames)))
        return frames.value

    def take_pcm_limiter(self):
        """-> (float32 [S]: the lowest r, int64 [S]: the frames with r < 1) of the newest exactFrames that limited; 1 and 0 for a stream it
        did not limit.  Synchronises the batch; resets nothing."""
        low, frames = np.ones(self.streams, np.float32), np.zeros(self.streams, np.int64)
        _check(self.lib, self.lib.smst_batch_take_pcm_limiter(self.h, low.ctypes.data_as(_fp), frames.ctypes.data_as(C.POINTER(_ll))))
        self._inflight = []
        return low, frames

    def set_pcm_stream_limiter(self, on=True, ceiling=1.0, stream=-1):
        """The stream limiter (include/smst.h, "Stream limiter"), processFrames and flushFrames only: a LEVEL_FIXED stream's output comes
        2*lookahead frames late and is brought down to ``ceiling`` (inf: no limit) by the clip limiter's curve, whatever the cuts between
        calls.  A setting of its own beside set_pcm_limiter's flag.  Clears the stream's line; stream = -1: every stream."""
        _check(self.lib, self.lib.smst_batch_set_pcm_stream_limiter(self.h, int(stream), 1 if on else 0, float(ceiling)))

    def pcm_stream_limiter(self, stream):
        """-> (on, ceiling) of the stream's setting"""
        on, ceiling = C.c_int(0), C.c_float(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_limiter(self.h, int(stream), C.byref(on), C.byref(ceiling)))
        return bool(on.value), ceiling.value

    def pcm_stream_limiter_latency(self):
        """-> 2*lookahead: the frames by which a limited stream's output is late"""
        frames = C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_limiter_latency(self.h, C.byref(frames)))
        return frames.value

    def set_pcm_stream_limiter_true_peak(self, on=True, stream=-1):
        """The stream limiter's true-peak flag (include/smst.h, "Stream limiter"): the detector sees the three inter-sample phases of "True
        peak" as well, the output comes 2*lookahead + 6 frames late, and the stream is, bit for bit, the clip limiter with its true-peak
        flag.  Inert while the stream's setting is off.  Clears the stream's line; stream = -1: every stream."""
        _check(self.lib, self.lib.smst_batch_set_pcm_stream_limiter_true_peak(self.h, int(stream), 1 if on else 0))

    def pcm_stream_limiter_true_peak(self, stream):
        on = C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_limiter_true_peak(self.h, int(stream), C.byref(on)))
        return bool(on.value)

    def pcm_stream_limiter_latency_of(self, stream):
        """-> the frames by which the stream's output is late: 0 with the setting off, 2*lookahead with it on, 6 more with the flag"""
        frames = C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_limiter_latency_of(self.h, int(stream), C.byref(frames)))
        return frames.value

    def take_pcm_stream_limiter(self):
        """-> (float32 [S]: the lowest r written, int64 [S]: the frames written with r < 1) over the calls since the last take; 1 and 0 where
        nothing was limited.  Synchronises the batch and clears the meters."""
        low, frames = np.ones(self.streams, np.float32), np.zeros(self.streams, np.int64)
        _check(self.lib, self.lib.smst_batch_take_pcm_stream_limiter(self.h, low.ctypes.data_as(_fp), frames.ctypes.data_as(C.POINTER(_ll))))
        self._inflight = []
        return low, frames

    def set_pcm_stream_meter(self, on=True, sample_rate=48000.0, max_sub_blocks=36000, stream=-1):
        """The stream meter (include/smst.h, "Stream meter"), processFrames and flushFrames only: every frame written for the stream is
        measured on the device -- R 128 loudness, loudness range, true peak --, before the gain, with readings equal to the clip meters'
        of the frames so far, whatever the cuts between calls.  ``max_sub_blocks`` 100-ms sub-blocks size the history (an hour: 36000); a
        full meter freezes.  Clears the stream's meter; stream = -1: every stream."""
        _check(self.lib, self.lib.smst_batch_set_pcm_stream_meter(self.h, int(stream), 1 if on else 0, float(sample_rate), int(max_sub_blocks)))

    def pcm_stream_meter(self, stream):
        """-> (on, sample_rate, max_sub_blocks) of the stream's setting"""
        on, rate, blocks = C.c_int(0), C.c_double(0), C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_meter(self.h, int(stream), C.byref(on), C.byref(rate), C.byref(blocks)))
        return bool(on.value), rate.value, blocks.value

    def pcm_stream_meter_frames(self, stream):
        """-> (frames emitted for the stream since its meter was cleared, frames metered): host counters, no synchronisation"""
        frames, metered = _ll(0), _ll(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_meter_frames(self.h, int(stream), C.byref(frames), C.byref(metered)))
        return frames.value, metered.value

    def take_pcm_stream_meter(self):
        """-> a dict of arrays [S] over the frames metered so far: lufs, momentary, short_term, momentary_max, short_term_max, low, high (LUFS,
        float64; -inf where undefined), range (LU), blocks, gated, short_blocks, range_blocks (int32), true_peaks, sample_peaks (float32,
        before the gain).  Synchronises the batch; resets nothing: metering goes on."""
        S = self.streams
        f64 = {k: np.zeros(S, np.float64) for k in ("lufs", "momentary", "short_term", "momentary_max", "short_term_max", "range", "low", "high")}
        i32 = {k: np.zeros(S, np.int32) for k in ("blocks", "gated", "short_blocks", "range_blocks")}
        f32 = {k: np.zeros(S, np.float32) for k in ("true_peaks", "sample_peaks")}
        d, i, f = (lambda k: f64[k].ctypes.data_as(_dp)), (lambda k: i32[k].ctypes.data_as(_ip)), (lambda k: f32[k].ctypes.data_as(_fp))
        _check(self.lib, self.lib.smst_batch_take_pcm_stream_meter(self.h, d("lufs"), i("blocks"), i("gated"), d("momentary"), d("short_term"), d("momentary_max"), d("short_term_max"),
                                                                   d("range"), d("low"), d("high"), i("short_blocks"), i("range_blocks"), f("true_peaks"), f("sample_peaks")))
        self._inflight = []
        return dict(f64, **i32, **f32)

    # --- test hooks
    def set_pcm_resample(self, up, down, stream=-1):
        """Resample in front of exactFrames (include/smst.h, "Resample"): the stream's clips are at down/up of the batch's rate and are
        resampled on the device, by the ratio up/down, before the engine sees them.  1/1 turns it off; stream = -1: every stream."""
        _check(self.lib, self.lib.smst_batch_set_pcm_resample(self.h, int(stream), int(up), int(down)))

    def set_pcm_stream_resample(self, up, down, stream=-1):
        """Resample in front of processFrames / seekFrames (include/smst.h, "Stream resample"): the stream's frames are at down/up of the
        batch's rate and are resampled on the device, by the ratio up/down, with the last T - 1 frames carried from call to call; the engine
        gets them H frames late.  1/1 turns it off; stream = -1: every stream.  Clears the stream's line."""
        _check(self.lib, self.lib.smst_batch_set_pcm_stream_resample(self.h, int(stream), int(up), int(down)))

    def pcm_stream_resample(self, stream):
        """-> (up, down), the stream's reduced streaming ratio; (1, 1): none"""
        up, down = C.c_int(0), C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_resample(self.h, int(stream), C.byref(up), C.byref(down)))
        return up.value, down.value

    def stream_resample_latency(self, stream):
        """-> H, the frames at the stream's own rate by which its input is late (0 without the setting)"""
        frames = C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_resample_latency(self.h, int(stream), C.byref(frames)))
        return frames.value

    def stream_resample_frames(self, stream, in_samples, fresh=False):
        """-> k, the frames the engine gets from the stream's next call if it hands in_samples frames (fresh: as after a clear)"""
        k = int(self.lib.smst_batch_pcm_stream_resample_frames(self.h, int(stream), int(in_samples), 1 if fresh else 0))
        if k < 0:
            _check(self.lib, k)
        return k

    def stream_resample_need(self, stream, frames, fresh=False):
        """-> the smallest n whose call gives the engine at least ``frames`` frames of the stream (fresh: as after a clear)"""
        n = int(self.lib.smst_batch_pcm_stream_resample_need(self.h, int(stream), int(frames), 1 if fresh else 0))
        if n < 0:
            _check(self.lib, n)
        return n

    def set_pcm_stream_out_resample(self, up, down, stream=-1):
        """Resample behind processFrames / flushFrames (include/smst.h, "Stream output resample"): the stream's frames are delivered at
        up/down of the batch's rate, resampled on the device in front of the stream limiter, the stream meter, gain and dither, with the
        last rendered frames carried from call to call; they come ceil(H*up/down) delivered frames late.  1/1 turns it off; stream = -1:
        every stream.  Clears the stream's line."""
        _check(self.lib, self.lib.smst_batch_set_pcm_stream_out_resample(self.h, int(stream), int(up), int(down)))

    def pcm_stream_out_resample(self, stream):
        """-> (up, down), the stream's reduced streaming output ratio; (1, 1): none"""
        up, down = C.c_int(0), C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_out_resample(self.h, int(stream), C.byref(up), C.byref(down)))
        return up.value, down.value

    def stream_out_resample_latency(self, stream):
        """-> Dl, the delivered frames by which the stream's output is late (0 without the setting)"""
        frames = C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_stream_out_resample_latency(self.h, int(stream), C.byref(frames)))
        return frames.value

    def stream_out_resample_render(self, stream, out_samples, fresh=False):
        """-> E, the frames the engine renders in the stream's next call if it delivers out_samples frames (fresh: as after a clear)"""
        E = int(self.lib.smst_batch_pcm_stream_out_resample_render(self.h, int(stream), int(out_samples), 1 if fresh else 0))
        if E < 0:
            _check(self.lib, E)
        return E

    def pcm_resample(self, stream):
        """-> (up, down), the stream's reduced ratio; (1, 1): not resampled"""
        up, down = C.c_int(0), C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_resample(self.h, int(stream), C.byref(up), C.byref(down)))
        return up.value, down.value

    def resampled_length(self, stream, in_samples):
        """-> Nr = ceil(in_samples*up/down) of the stream's ratio: the clip's length at the batch's rate, what out_samples derives from"""
        n = int(self.lib.smst_batch_resampled_length(self.h, int(stream), int(in_samples)))
        if n < 0:
            _check(self.lib, n)
        return n

    def set_pcm_out_resample(self, up, down, stream=-1):
        """Resample behind the engine in exactFrames (include/smst.h, "Output resample"): the stream's clips are delivered at up/down of the
        batch's rate -- out_samples counts delivered frames, and the level stages, dither and conversion run on them.  1/1 turns it off;
        stream = -1: every stream."""
        _check(self.lib, self.lib.smst_batch_set_pcm_out_resample(self.h, int(stream), int(up), int(down)))

    def pcm_out_resample(self, stream):
        """-> (up, down), the stream's reduced output ratio; (1, 1): delivered at the batch's rate"""
        up, down = C.c_int(0), C.c_int(0)
        _check(self.lib, self.lib.smst_batch_pcm_out_resample(self.h, int(stream), C.byref(up), C.byref(down)))
        return up.value, down.value

    def out_render_length(self, stream, out_samples):
        """-> E = (out_samples - 1)*down//up + 1 of the stream's output ratio: the frames the engine renders for out_samples delivered ones"""
        n = int(self.lib.smst_batch_pcm_out_render_length(self.h, int(stream), int(out_samples)))
        if n < 0:
            _check(self.lib, n)
        return n

    def debug_state(self, stream, which):
        Cn, M = self.channels, self.bands()
        if which == 3:
            a = np.zeros((Cn, M), np.float32)
            _check(self.lib, self.lib.smst_batch_debug_get_state(self.h, stream, which, a.ctypes.data_as(_fp)))
            return a
        a = np.zeros((Cn, M, 2), np.float32)
        _check(self.lib, self.lib.smst_batch_debug_get_state(self.h, stream, which, a.ctypes.data_as(_fp)))
        return a[..., 0] + 1j*a[..., 1]

    def debug_set_state(self, stream, which, values):
        """Teacher forcing: overwrite Band.input / .prevInput / .output (complex [C, M]) or Prediction.energy ([C, M])."""
        Cn, M = self.channels, self.bands()
        if which == 3:
            a = np.ascontiguousarray(np.asarray(values, np.float32).reshape(Cn, M))
        else:
            v = np.asarray(values).reshape(Cn, M)
            a = np.ascontiguousarray(np.stack([v.real, v.imag], axis=-1).astype(np.float32))
        _check(self.lib, self.lib.smst_batch_debug_set_state(self.h, stream, which, a.ctypes.data_as(_fp)))

    def debug_set_carry(self, stream, sums, products):
        n = self.blockSamples() + self.intervalSamples()
        s = np.ascontiguousarray(np.asarray(sums, np.float32).reshape(self.channels, n))
        p = np.ascontiguousarray(np.asarray(products, np.float32).reshape(n))
        _check(self.lib, self.lib.smst_batch_debug_set_carry(self.h, stream, s.ctypes.data_as(_fp), p.ctypes.data_as(_fp)))

    def debug_map(self, stream):
        """(inputBin, freqGrad) per bin of the stream's newest hop, or None if that hop had no frequency map."""
        a = np.zeros((self.bands(), 2), np.float32)
        rc = self.lib.smst_batch_debug_get_map(self.h, stream, a.ctypes.data_as(_fp))
        if rc < 0:
            _check(self.lib, rc)
        return a if rc == 1 else None

    def debug_formants(self, stream):
        """(ratio[bands], envelope[bands], freqEstimate in bins) of the stream's newest hop, or None (no formant processing in that hop, or a
        batch that was not created with SMST_NO_FEED_FUSION=1)."""
        ratio, env, fe = np.zeros(self.bands(), np.float32), np.zeros(self.bands(), np.float32), np.zeros(1, np.float32)
        rc = self.lib.smst_batch_debug_get_formants(self.h, stream, ratio.ctypes.data_as(_fp), env.ctypes.data_as(_fp), fe.ctypes.data_as(_fp))
        if rc < 0:
            _check(self.lib, rc)
        return (ratio, env, float(fe[0])) if rc == 1 else None

    def allocation_events(self):
        return int(self.lib.smst_batch_debug_allocation_events(self.h))

    def debug_carry(self, stream):
        n = self.blockSamples() + self.intervalSamples()
        s = np.zeros((self.channels, n), np.float32)
        p = np.zeros(n, np.float32)
        _check(self.lib, self.lib.smst_batch_debug_get_carry(self.h, stream, s.ctypes.data_as(_fp), p.ctypes.data_as(_fp)))
        return s, p


class SignalsmithStretch:
    """Single-stream mirror of ``signalsmith::stretch::SignalsmithStretch<float>`` (same method names;
    buffers are [C, n] float32 numpy arrays) over the single-stream C ABI (group 1 of include/smst.h)."""

    def __init__(self, seed=0, device=0, lib=None):
        self.lib = lib if lib is not None else load_library()
        h = C.c_void_p()
        _check(self.lib, self.lib.smst_create(C.byref(h), seed, device))
        self.h = h
        self.channels = 0

    def close(self):
        if getattr(self, "h", None):
            self.lib.smst_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clone(self):
        """A copy of the object as the reference's (implicit) copy constructor makes one: configuration, parameters and the
        complete processing state; both continue identically and independently (smst_clone)."""
        other = SignalsmithStretch.__new__(SignalsmithStretch)
        other.lib, other.channels = self.lib, self.channels
        h = C.c_void_p()
        _check(self.lib, self.lib.smst_clone(C.byref(h), self.h))
        other.h = h
        return other

    def presetDefault(self, channels, sample_rate, split=False):
        self.channels = channels
        _check(self.lib, self.lib.smst_preset_default(self.h, channels, sample_rate, int(split)))

    def presetCheaper(self, channels, sample_rate, split=True):
        self.channels = channels
        _check(self.lib, self.lib.smst_preset_cheaper(self.h, channels, sample_rate, int(split)))

    def configure(self, channels, block, interval, split=False):
        self.channels = channels
        _check(self.lib, self.lib.smst_configure(self.h, channels, block, interval, int(split)))

    def blockSamples(self): return self.lib.smst_block_samples(self.h)
    def intervalSamples(self): return self.lib.smst_interval_samples(self.h)
    def inputLatency(self): return self.lib.smst_input_latency(self.h)
    def outputLatency(self): return self.lib.smst_output_latency(self.h)
    def splitComputation(self): return bool(self.lib.smst_split_computation(self.h))
    def seekLength(self): return self.lib.smst_seek_length(self.h)
    def outputSeekLength(self, rate): return self.lib.smst_output_seek_length(self.h, rate)
    def reset(self): _check(self.lib, self.lib.smst_reset(self.h))
    def setTransposeFactor(self, m, tonality=0.0): _check(self.lib, self.lib.smst_set_transpose_factor(self.h, m, tonality))
    def setTransposeSemitones(self, s, tonality=0.0): _check(self.lib, self.lib.smst_set_transpose_semitones(self.h, s, tonality))
    def setFormantFactor(self, m, comp=False): _check(self.lib, self.lib.smst_set_formant_factor(self.h, m, int(comp)))
    def setFormantSemitones(self, s, comp=False): _check(self.lib, self.lib.smst_set_formant_semitones(self.h, s, int(comp)))
    def setFormantBase(self, f=0.0): _check(self.lib, self.lib.smst_set_formant_base(self.h, f))

    def setFreqMapTable(self, table):
        if table is None:
            _check(self.lib, self.lib.smst_set_freq_map_table(self.h, None, 0))
        else:
            t = np.ascontiguousarray(table, np.float32)
            _check(self.lib, self.lib.smst_set_freq_map_table(self.h, t.ctypes.data_as(_fp), len(t)))

    def _planes(self, a):
        ptrs = (_fp*self.channels)()
        for c in range(self.channels):
            ptrs[c] = a[c].ctypes.data_as(_fp)
        return ptrs

    def _in(self, x):
        a = np.ascontiguousarray(np.asarray(x, np.float32).reshape(self.channels, -1))
        return a, self._planes(a)

    def seek(self, x, rate):
        a, p = self._in(x)
        _check(self.lib, self.lib.smst_seek(self.h, p, a.shape[1], rate))

    def process(self, x, out_samples):
        a, p = self._in(x)
        out = np.zeros((self.channels, max(out_samples, 1)), np.float32)
        _check(self.lib, self.lib.smst_process(self.h, p, a.shape[1], self._planes(out), out_samples))
        return out[:, :out_samples]

    def flush(self, out_samples, rate=0.0):
        out = np.zeros((self.channels, max(out_samples, 1)), np.float32)
        _check(self.lib, self.lib.smst_flush(self.h, self._planes(out), out_samples, rate))
        return out[:, :out_samples]

    def outputSeek(self, x):
        a, p = self._in(x)
        _check(self.lib, self.lib.smst_output_seek(self.h, p, a.shape[1]))

    # --- extension (include/smst.h group 3): the two halves of process() for an object in a StretchPool
    def processAsync(self, x, out_samples):
        """Records process(x, out_samples) with the object's pool; wait() returns the output.  The buffers are kept alive here until then.
        On an object that is in no pool this is process() itself, and wait() hands its result over."""
        a, p = self._in(x)
        out = np.zeros((self.channels, max(out_samples, 1)), np.float32)
        po = self._planes(out)
        self._request = (a, p, out, po, out_samples)
        _check(self.lib, self.lib.smst_process_begin(self.h, p, a.shape[1], po, out_samples))

    def wait(self):
        """Runs the pool if the request is still pending; -> the [C, out_samples] output of the newest processAsync()."""
        rc = self.lib.smst_process_end(self.h)
        request, self._request = getattr(self, "_request", None), None
        _check(self.lib, rc)
        if request is None:
            raise StretchError("wait() without processAsync()")
        return request[2][:, :request[4]]

    def exact(self, x, out_samples):
        a, p = self._in(x)
        out = np.zeros((self.channels, max(out_samples, 1)), np.float32)
        rc = self.lib.smst_exact(self.h, p, a.shape[1], self._planes(out), out_samples)
        if rc == -3:
            return out[:, :out_samples], False
        _check(self.lib, rc)
        return out[:, :out_samples], True


class StretchPool:
    """EXTENSION (the reference has nothing like it): SignalsmithStretch objects added to a pool record their process() calls with
    processAsync(); run() -- or the first wait() -- runs everything pending as ONE batched device submission per geometry.  Every
    object's output is bit for bit what it would be unpooled (include/smst.h, group 3)."""

    def __init__(self, device=0, lib=None):
        self.lib = lib if lib is not None else load_library()
        h = C.c_void_p()
        _check(self.lib, self.lib.smst_pool_create(C.byref(h), device))
        self.h = h

    def close(self):
        """Runs what is pending and detaches every member (they stay valid and keep their state)."""
        if getattr(self, "h", None):
            self.lib.smst_pool_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, stretch): _check(self.lib, self.lib.smst_pool_attach(self.h, stretch.h))
    def remove(self, stretch): _check(self.lib, self.lib.smst_pool_detach(stretch.h))
    def run(self): _check(self.lib, self.lib.smst_pool_run(self.h))
    def members(self): return int(self.lib.smst_pool_members(self.h))
    def pending(self): return int(self.lib.smst_pool_pending(self.h))
    def engine_calls(self): return int(self.lib.smst_pool_debug_engine_calls(self.h))
    def allocation_events(self): return int(self.lib.smst_pool_debug_allocation_events(self.h))
