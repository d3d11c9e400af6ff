"""TPDF dither of the int16 / int24 output of the batch PCM calls, on the device: the dithered conversion kernel against the numpy mirror
of include/smst.h, sessions and whole clips in host and in device memory against the mirror of the planar calls' output, the counters, the
launch counters, the refusals and the command-line tool.  Every comparison with the mirror is exact (tests/dither_cases.py); on a library
without the dither entry points every test fails at its first call."""
import os

import pytest

import dither_cases as dc
import pcm_format_cases as fc
from conftest import package

pytestmark = pytest.mark.gpu


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_s16_converter_against_mirror(hip, channels):
    dc.check_converter(hip, fc.S16, channels, (0, 2))


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_s24_converter_against_mirror(hip, channels):
    dc.check_converter(hip, fc.S24, channels, range(16) if channels <= 3 else (0, 3))


def test_constant_below_one_lsb(hip):
    dc.check_constant_below_one_lsb(hip)


@pytest.mark.parametrize("mode", dc.MODES)
def test_statistics_of_the_specification(hip, mode):
    dc.check_statistics(hip, mode, -7)


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_session_equals_mirror_of_planar_host_memory(hip, fmt):
    dc.check_session(hip, fmt)


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_session_equals_mirror_of_planar_device_memory(hip, fmt):
    dc.check_session(hip, fmt, **_device_memory())


def test_session_cut_into_other_calls(hip):
    dc.check_recut(hip, fc.S16)


def test_set_dither_restarts_the_counter(hip):
    dc.check_restart(hip)


@pytest.mark.parametrize("fmt", [fc.S32, fc.F16, fc.F32])
def test_other_formats_are_unchanged(hip, fmt):
    dc.check_other_formats_unchanged(hip, fmt)


def test_other_formats_are_unchanged_device_memory(hip):
    dc.check_other_formats_unchanged(hip, fc.F16, **_device_memory())


def test_steady_state_and_launch_counters_host_memory(hip):
    dc.check_steady_state_and_launches(hip)


def test_steady_state_and_launch_counters_device_memory(hip):
    dc.check_steady_state_and_launches(hip, _device_memory()["to_memory"])


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips_host_memory(hip, fmt):
    dc.check_clips(hip, fmt)


def test_whole_clips_device_memory(hip):
    dc.check_clips(hip, fc.S24, **_device_memory())


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips_wide_output_host_memory(hip, fmt):
    dc.check_clips(hip, fmt, wide=True)


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips_wide_output_device_memory(hip, fmt):
    dc.check_clips(hip, fmt, wide=True, **_device_memory())


def test_refusals(hip):
    dc.check_refusals(hip)


def test_cli_dither_gpu(tmp_path):
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    dc.check_cli(exe, tmp_path)
