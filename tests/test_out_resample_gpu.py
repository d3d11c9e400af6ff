"""The sample-rate converter behind the engine in smst_batch_exact_pcm (include/smst.h, "Output resample") on the device: the library's
lengths; the kernel against the numpy mirror bit for bit, with the source's join in every position; whole clips through exactFrames in
host and in device memory against a twin batch that renders E frames; the level chain behind the converter against the existing hooks on
the mirror's image; the opt-in, the steady state, the refusals and the command-line tool (tests/out_resample_cases.py has the mirror and
the checks).  On a library without the new entry points every test fails at its first call."""
import os

import pytest

import out_resample_cases as oc
import pcm_format_cases as fc
import resample_cases as rs
from conftest import package

pytestmark = pytest.mark.gpu

FORMATS = [(fc.S16, True), (fc.S24, True), (fc.S32, False), (fc.F16, False), (fc.F32, False)]


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def test_render_length(hip):
    oc.check_lengths(hip)


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("up,down", rs.RATIOS)
def test_kernel_against_mirror(hip, up, down, channels):
    oc.check_kernel(hip, up, down, channels)


def test_eight_ratios_in_one_launch(hip):
    oc.check_mixed(hip)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_whole_clips_host_memory(hip, fmt, dithered):
    oc.check_clips(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_whole_clips_device_memory(hip, fmt, dithered):
    oc.check_clips(hip, fmt, dithered, **_device_memory())


def test_chain_runs_on_the_delivered_frames_host_memory(hip):
    oc.check_chain(hip)


def test_chain_runs_on_the_delivered_frames_device_memory(hip):
    oc.check_chain(hip, **_device_memory())


def test_opt_in_host_memory(hip):
    oc.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    oc.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    oc.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    oc.check_steady_state(hip, _device_memory()["to_memory"])


def test_two_runs_are_bit_identical(hip):
    oc.check_reproducible(hip)


def test_refusals(hip):
    oc.check_refusals(hip)
    oc.check_refusals(hip, _device_memory()["to_memory"])


def test_cli_out_resample_gpu(hip, tmp_path):
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    oc.check_cli(exe, tmp_path, hip)
