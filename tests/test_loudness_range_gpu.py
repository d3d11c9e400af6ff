"""The loudness-range meter of the frame output (include/smst.h, "Loudness range") on the device: the range stage against the numpy mirror,
the selection bit for bit, the content cases, the caps, whole clips through exactFrames in host and in device memory, the opt-in, the
steady state, the refusals and the command-line tool (tests/loudness_range_cases.py has the mirror and the checks).  On a library without
the new entry points every test fails at its first call.

Largest |p/p_mirror - 1| over the powers of this file's runs on an MI355X, and how many were compared: see EXPERIMENTS.md (the bound is 1e-9)."""
import os

import pytest

import loudness_cases as ld
import loudness_range_cases as lr
import pcm_format_cases as fc
from conftest import package

pytestmark = pytest.mark.gpu


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def _report():
    print("largest |p/p_mirror - 1| so far: %.3g over %d powers" % (ld.worst_seen["power"], lr.compared["powers"]))


@pytest.mark.parametrize("fs,channels", [(8000, 1), (8000, 2), (8000, 3), (8000, 16), (5120, 2)])
def test_stage_against_mirror(hip, fs, channels):
    lr.check_hook(hip, fs, channels)


def test_lowest_rate_where_the_hop_is_the_chunk(hip):
    lr.check_hook_lowest_rate(hip)


def test_selection_is_exact(hip):
    lr.check_selection(hip)


def test_gates_maxima_and_undefined_cases(hip):
    lr.check_content(hip)
    _report()


def test_caps(hip):
    lr.check_caps(hip)
    _report()


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, True), (fc.S16, False), (fc.S24, True), (fc.F32, False)])
def test_whole_clips_host_memory(hip, fmt, dithered):
    lr.check_clips(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, True), (fc.S16, False), (fc.S24, True), (fc.F32, False)])
def test_whole_clips_device_memory(hip, fmt, dithered):
    lr.check_clips(hip, fmt, dithered, **_device_memory())
    _report()


def test_two_runs_are_bit_identical(hip):
    lr.check_reproducible(hip)
    lr.check_two_runs(hip)


def test_opt_in_host_memory(hip):
    lr.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    lr.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    lr.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    lr.check_steady_state(hip, _device_memory()["to_memory"])


def test_refusals(hip):
    lr.check_refusals(hip)


def test_meter_and_caps_are_refused_in_streaming_calls(hip):
    lr.check_refused_in_streaming_calls(hip)
    lr.check_refused_in_streaming_calls(hip, **_device_memory())


def test_cli_loudness_range_gpu(hip, tmp_path):
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    lr.check_cli(exe, tmp_path)
