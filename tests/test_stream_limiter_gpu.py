"""The stream limiter of the frame output (include/smst.h, "Stream limiter") on the device: the hook against the numpy mirror bit for bit,
cut invariance, NaN and inf, processFrames and flushFrames end to end in host and in device memory, two runs, the opt-in, the steady
state, the refusals and the clearing rules (tests/stream_limiter_cases.py has the mirror and the checks).  On a library without the stream
limiter's entry points every test fails at its first call.

Every comparison of r, the frames and the meters with the mirror is one of bit patterns."""
import pytest

import limiter_cases as lm
import pcm_format_cases as fc
import stream_limiter_cases as sl

pytestmark = pytest.mark.gpu

FORMATS = [(fc.S16, False), (fc.S16, True), (fc.S24, False), (fc.S24, True), (fc.F32, False)]


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def test_known_answers_through_the_hook(hip):
    sl.check_known_answers(hip)


@pytest.mark.parametrize("lookahead", [1, 2, 72])
@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_hook_against_mirror(hip, channels, lookahead):
    sl.check_hook(hip, channels, lookahead)


@pytest.mark.parametrize("channels", [1, 2])
def test_hook_against_mirror_longest_lookahead(hip, channels):
    sl.check_hook(hip, channels, lm.MAX_H, variants=(channels % 2,))


def test_cut_invariance(hip):
    sl.check_cut_invariance(hip)


def test_nan_and_inf(hip):
    sl.check_nan_inf(hip)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_process_and_flush_host_memory(hip, fmt, dithered):
    sl.check_session(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_process_and_flush_device_memory(hip, fmt, dithered):
    sl.check_session(hip, fmt, dithered, **_device_memory())
    print("frames of r bit-identical to the mirror so far: %d" % sl.compared["frames"])


def test_process_and_flush_short_lookahead(hip):
    sl.check_session(hip, fc.S16, True, H=3)


def test_two_runs_are_bit_identical(hip):
    sl.check_reproducible(hip)
    sl.check_two_runs(hip)
    sl.check_two_runs(hip, **_device_memory())


def test_opt_in_host_memory(hip):
    sl.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    sl.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    sl.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    sl.check_steady_state(hip, _device_memory()["to_memory"])


def test_refusals_and_getters(hip):
    sl.check_refusals(hip)
    sl.check_refusals(hip, **_device_memory())


@pytest.mark.parametrize("action", ["setter", "setter_one", "lookahead", "reset", "level"])
def test_clearing(hip, action):
    sl.check_clearing(hip, action)
