"""The sample-rate converter's streaming form behind smst_batch_process_pcm / _flush_pcm (include/smst.h, "Stream output resample") on the
device: the kernel hook against the numpy streaming model bit for bit, at 64-bit positions and with eight ratios in one sequence of calls;
processFrames and flushFrames in host and in device memory against a twin batch whose output the model resamples, with the stream limiter,
the stream meter, the input setting, and across reset and seek; the opt-in, the steady state and the refusals
(tests/stream_out_resample_cases.py has the model and the checks).  On a library without the new entry points every test fails at its
first call."""
import pytest

import pcm_format_cases as fc
import resample_cases as rs
import stream_out_resample_cases as so

pytestmark = pytest.mark.gpu

FORMATS = [(fc.S16, True), (fc.S24, True), (fc.S32, False), (fc.F16, False), (fc.F32, False)]


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("up,down", rs.RATIOS)
def test_hook_against_model(hip, up, down, channels):
    so.check_hook(hip, up, down, channels)


def test_hook_known_answers(hip):
    so.check_known_answers(hip)


def test_positions_beyond_32_bits(hip):
    so.check_far_positions(hip)


def test_eight_ratios_and_two_plain_streams(hip):
    so.check_mixed(hip)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_session_host_memory(hip, fmt, dithered):
    so.check_session(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_session_device_memory(hip, fmt, dithered):
    so.check_session(hip, fmt, dithered, **_device_memory())


def test_session_with_stream_limiter_host_memory(hip):
    so.check_session(hip, fc.F32, False, limiter=True)


def test_session_with_stream_limiter_device_memory(hip):
    so.check_session(hip, fc.F32, False, limiter=True, **_device_memory())


def test_session_with_stream_meter_host_memory(hip):
    so.check_session(hip, fc.F32, False, meter=True)


def test_session_with_stream_meter_device_memory(hip):
    so.check_session(hip, fc.F32, False, meter=True, **_device_memory())


def test_session_with_input_stream_resample_host_memory(hip):
    so.check_session(hip, fc.S16, True, resample_in=True)


def test_session_with_input_stream_resample_device_memory(hip):
    so.check_session(hip, fc.S16, True, resample_in=True, **_device_memory())


def test_reset_clears_the_line_and_seek_does_not_host_memory(hip):
    so.check_session(hip, fc.S16, True, seek=True)


def test_reset_clears_the_line_and_seek_does_not_device_memory(hip):
    so.check_session(hip, fc.S16, True, seek=True, **_device_memory())


def test_opt_in_host_memory(hip):
    so.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    so.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    so.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    so.check_steady_state(hip, _device_memory()["to_memory"])


def test_two_runs_are_bit_identical_and_getters(hip):
    so.check_reproducible(hip)


def test_refusals(hip):
    so.check_refusals(hip)
    so.check_refusals(hip, _device_memory()["to_memory"])
