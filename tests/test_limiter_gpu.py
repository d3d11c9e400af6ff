"""The limiter flag of the frame output (include/smst.h, "Limiter") on the device: the library's window against the formula, the two passes
against the numpy mirror bit for bit, NaN and inf, whole clips through exactFrames in host and in device memory, the opt-in, the steady
state, the refusals and the command-line tool (tests/limiter_cases.py has the mirror and the checks).  On a library without the limiter's
entry points every test fails at its first call.

Every comparison of need, r and the meters with the mirror is one of bit patterns; EXPERIMENTS.md has how many frames this file's runs
compared on an MI355X."""
import os

import pytest

import limiter_cases as lm
import pcm_format_cases as fc
from conftest import package

pytestmark = pytest.mark.gpu

FORMATS = [(fc.S16, False), (fc.S16, True), (fc.S24, False), (fc.S24, True), (fc.F32, False)]


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def test_window_against_formula(hip):
    lm.check_window(hip)


@pytest.mark.parametrize("lookahead", [1, 2, 72])
@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_passes_against_mirror(hip, channels, lookahead):
    lm.check_hook(hip, channels, lookahead)


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_passes_against_mirror_longest_lookahead(hip, channels):
    lm.check_hook(hip, channels, lm.MAX_H)


def test_mixed_batch(hip):
    lm.check_mixed(hip)


def test_nan_and_inf(hip):
    lm.check_nan_inf(hip)


def test_two_runs_are_bit_identical(hip):
    lm.check_reproducible(hip)
    lm.check_two_runs(hip)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_whole_clips_host_memory(hip, fmt, dithered):
    lm.check_clips(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_whole_clips_device_memory(hip, fmt, dithered):
    lm.check_clips(hip, fmt, dithered, **_device_memory())
    print("frames of r bit-identical to the mirror so far: %d" % lm.compared["frames"])


def test_opt_in_host_memory(hip):
    lm.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    lm.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    lm.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    lm.check_steady_state(hip, _device_memory()["to_memory"])


def test_refusals(hip):
    lm.check_refusals(hip)


def test_flag_is_refused_in_streaming_calls(hip):
    lm.check_refused_in_streaming_calls(hip)
    lm.check_refused_in_streaming_calls(hip, **_device_memory())


def test_cli_limit_gpu(hip, tmp_path):
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    lm.check_cli(exe, tmp_path, hip)
