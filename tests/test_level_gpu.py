"""Per-stream gain, peak meters and clip-safe whole-clip gains of the frame output, on the device: the levelled conversion kernel and the
clip pair (kClipPeak + the levelled kClipOut) against the numpy mirror -- the fp32 quotient of the whole-clip gain bit for bit --, the
ceiling table's worst cases, sessions and whole clips in host and in device memory against the mirror of the planar calls' output, the
opt-in, the steady state, the refusals and the command-line tool.  Every comparison with the mirror is exact (tests/level_cases.py); on a
library without the level entry points every test fails at its first call."""
import os

import pytest

import dither_cases as dc
import level_cases as lc
import pcm_format_cases as fc
from conftest import package

pytestmark = pytest.mark.gpu


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("fmt", lc.ALL_FORMATS)
def test_converter_against_mirror(hip, fmt, channels):
    lc.check_converter(hip, fmt, channels, (0, 1, 5) if fmt == fc.S24 else (0, fc.ELEM_BYTES[fmt]))


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", [fc.S16, fc.S24, fc.F32])
def test_clip_pair_against_mirror(hip, fmt, channels):
    lc.check_clip_pair(hip, fmt, channels)


@pytest.mark.parametrize("fmt,dithered", sorted(lc.CEILINGS))
def test_ceiling_worst_case_is_not_clamped(hip, fmt, dithered):
    lc.check_ceiling_on_device(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, False), (fc.S16, True), (fc.S24, True), (fc.F32, False)])
def test_session_equals_mirror_of_planar_host_memory(hip, fmt, dithered):
    lc.check_session(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, True), (fc.S24, False)])
def test_session_equals_mirror_of_planar_device_memory(hip, fmt, dithered):
    lc.check_session(hip, fmt, dithered, **_device_memory())


def test_session_cut_into_other_calls(hip):
    lc.check_recut(hip, fc.S16)


def test_whole_clip_mode_is_refused_in_streaming_calls_host_memory(hip):
    lc.check_whole_clip_mode_refused_in_streaming_calls(hip)


def test_whole_clip_mode_is_refused_in_streaming_calls_device_memory(hip):
    lc.check_whole_clip_mode_refused_in_streaming_calls(hip, **_device_memory())


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips_host_memory(hip, fmt):
    lc.check_clips(hip, fmt)


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips_device_memory(hip, fmt):
    lc.check_clips(hip, fmt, **_device_memory())


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips_wide_output_device_memory(hip, fmt):
    lc.check_clips(hip, fmt, wide=True, **_device_memory())


def test_whole_clips_wide_output_host_memory(hip):
    lc.check_clips(hip, fc.S16, wide=True)


@pytest.mark.parametrize("dithered", [False, True])
def test_opt_in_host_memory(hip, dithered):
    lc.check_opt_in(hip, dithered)


def test_opt_in_device_memory(hip):
    lc.check_opt_in(hip, False, **_device_memory())


def test_steady_state_host_memory(hip):
    lc.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    lc.check_steady_state(hip, _device_memory()["to_memory"])


def test_refusals(hip):
    lc.check_refusals(hip)


def test_cli_level_gpu(hip, tmp_path):
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    lc.check_cli(exe, tmp_path, hip)
