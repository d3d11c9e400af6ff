"""The loudness mode of the frame output (include/smst.h, "Loudness") on the device: the four passes against the numpy mirror, whole clips
through exactFrames in host and in device memory, the opt-in, the steady state, the refusals and the command-line tool
(tests/loudness_cases.py has the mirror and the checks).  On a library without the loudness entry points every test fails at its first call.

Largest |z/z_mirror - 1| over the block powers and Z of this file's runs on an MI355X: see EXPERIMENTS.md (the bound is 1e-9)."""
import os

import pytest

import loudness_cases as ld
import pcm_format_cases as fc
from conftest import package

pytestmark = pytest.mark.gpu


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("fs", [8000, 12000])
def test_passes_against_mirror(hip, fs, channels):
    ld.check_hook(hip, fs, channels)


def test_gates_and_undefined_cases(hip):
    ld.check_content(hip)
    print("largest |z/z_mirror - 1| so far: %.3g" % ld.worst_seen["power"])


def test_two_runs_are_bit_identical(hip):
    ld.check_reproducible(hip)
    ld.check_two_runs(hip)


@pytest.mark.parametrize("fs", [8000, 12000])
@pytest.mark.parametrize("fmt", [fc.S16, fc.S24, fc.F32])
def test_whole_clips_host_memory(hip, fmt, fs):
    ld.check_clips(hip, fmt, fs)


@pytest.mark.parametrize("fs", [8000, 12000])
@pytest.mark.parametrize("fmt", [fc.S16, fc.S24, fc.F32])
def test_whole_clips_device_memory(hip, fmt, fs):
    ld.check_clips(hip, fmt, fs, **_device_memory())
    print("largest |z/z_mirror - 1| so far: %.3g" % ld.worst_seen["power"])


def test_opt_in_host_memory(hip):
    ld.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    ld.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    ld.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    ld.check_steady_state(hip, _device_memory()["to_memory"])


def test_refusals(hip):
    ld.check_refusals(hip)


def test_loudness_mode_is_refused_in_streaming_calls(hip):
    ld.check_refused_in_streaming_calls(hip)
    ld.check_refused_in_streaming_calls(hip, **_device_memory())


def test_cli_loudness_gpu(hip, tmp_path):
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    ld.check_cli(exe, tmp_path)
