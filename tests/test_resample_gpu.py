"""The sample-rate converter in front of smst_batch_exact_pcm (include/smst.h, "Resample") on the device: the library's table against the
formula; the kernel against the numpy mirror bit for bit; whole clips through exactFrames in host and in device memory against a twin batch
fed the mirror's frames; the opt-in, the steady state, the refusals and the command-line tool (tests/resample_cases.py has the mirror and
the checks).  On a library without the new entry points every test fails at its first call."""
import os

import pytest

import pcm_format_cases as fc
import resample_cases as rs
from conftest import package

pytestmark = pytest.mark.gpu

FORMATS = [(fc.S16, True), (fc.S24, True), (fc.S32, False), (fc.F16, False), (fc.F32, False)]


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("up,down", rs.TABLE_RATIOS)
def test_table_against_formula(hip, up, down):
    rs.check_table(hip, up, down)


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("up,down", rs.RATIOS)
def test_kernel_against_mirror(hip, up, down, channels):
    rs.check_kernel(hip, up, down, channels)


def test_eight_ratios_in_one_launch(hip):
    rs.check_mixed(hip)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_whole_clips_host_memory(hip, fmt, dithered):
    rs.check_clips(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_whole_clips_device_memory(hip, fmt, dithered):
    rs.check_clips(hip, fmt, dithered, **_device_memory())


def test_whole_clips_loudness_true_peak_limiter_host_memory(hip):
    rs.check_clips(hip, fc.F32, False, chain=True)


def test_whole_clips_loudness_true_peak_limiter_device_memory(hip):
    rs.check_clips(hip, fc.F32, False, chain=True, **_device_memory())


def test_opt_in_host_memory(hip):
    rs.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    rs.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    rs.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    rs.check_steady_state(hip, _device_memory()["to_memory"])


def test_two_runs_are_bit_identical(hip):
    rs.check_reproducible(hip)


def test_refusals(hip):
    rs.check_refusals(hip)
    rs.check_refusals(hip, _device_memory()["to_memory"])


def test_cli_resample_gpu(hip, tmp_path):
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    rs.check_cli(exe, tmp_path, hip)
