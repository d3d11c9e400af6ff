"""The true-peak flag of the frame output (include/smst.h, "True peak") on the device: the library's taps against the formula, the pass
against the numpy mirror bit for bit, NaN and inf, whole clips through exactFrames in host and in device memory, the opt-in, the steady
state, the refusals and the command-line tool (tests/true_peak_cases.py has the mirror and the checks).  On a library without the true-peak
entry points every test fails at its first call.

Every comparison of a true peak with the mirror is one of bit patterns; EXPERIMENTS.md has how many this file's runs made on an MI355X."""
import os

import pytest

import pcm_format_cases as fc
import true_peak_cases as tp
from conftest import package

pytestmark = pytest.mark.gpu


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def test_taps_against_formula(hip):
    tp.check_taps(hip)


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_pass_against_mirror(hip, channels):
    tp.check_hook(hip, channels)


def test_planted_inter_sample_peaks(hip):
    tp.check_planted(hip)


def test_nan_and_inf(hip):
    tp.check_nan_inf(hip)
    print("true peaks bit-identical to the mirror so far: %d" % tp.compared["peaks"])


def test_two_runs_are_bit_identical(hip):
    tp.check_reproducible(hip)
    tp.check_two_runs(hip)


@pytest.mark.parametrize("fmt", [fc.S16, fc.S24, fc.F32])
def test_whole_clips_host_memory(hip, fmt):
    tp.check_clips(hip, fmt)


@pytest.mark.parametrize("fmt", [fc.S16, fc.S24, fc.F32])
def test_whole_clips_device_memory(hip, fmt):
    tp.check_clips(hip, fmt, **_device_memory())
    print("true peaks bit-identical to the mirror so far: %d" % tp.compared["peaks"])


def test_opt_in_host_memory(hip):
    tp.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    tp.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    tp.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    tp.check_steady_state(hip, _device_memory()["to_memory"])


def test_refusals(hip):
    tp.check_refusals(hip)


def test_flag_is_refused_in_streaming_calls(hip):
    tp.check_refused_in_streaming_calls(hip)
    tp.check_refused_in_streaming_calls(hip, **_device_memory())


def test_cli_true_peak_gpu(hip, tmp_path):
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    tp.check_cli(exe, tmp_path, hip)
