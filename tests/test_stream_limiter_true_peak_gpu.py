"""The stream limiter's true-peak flag (include/smst.h, "Stream limiter") on the device: the known answers, the hook against the numpy mirror
bit for bit, cut invariance, NaN and inf, processFrames and flushFrames end to end in host and in device memory, behind a stream output
resample, two runs, the opt-in, the steady state, the getters and refusals and the clearing rules
(tests/stream_limiter_true_peak_cases.py has the mirror and the checks).  On a library without the flag's entry points every test fails at
its first call.

Every comparison of r, the frames, the integer codes and the meters with the mirror is one of bit patterns."""
import pytest

import limiter_cases as lm
import pcm_format_cases as fc
import stream_limiter_true_peak_cases as st

pytestmark = pytest.mark.gpu

FORMATS = [(fc.S16, False), (fc.S16, True), (fc.S24, False), (fc.S24, True), (fc.F32, False)]


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def test_known_answers_through_the_hook(hip):
    st.check_known_answers(hip)


@pytest.mark.parametrize("lookahead", [1, 2, 3, 72])
@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_hook_against_mirror(hip, channels, lookahead):
    st.check_hook(hip, channels, lookahead, variants=(channels % 5, (channels + 2) % 5))


@pytest.mark.parametrize("channels", [1, 2])
def test_hook_against_mirror_longest_lookahead(hip, channels):
    st.check_hook(hip, channels, lm.MAX_H, variants=st.LONGEST_VARIANTS)


def test_cut_invariance(hip):
    st.check_cut_invariance(hip)


def test_nan_and_inf(hip):
    st.check_nan_inf(hip)


@pytest.mark.parametrize("lookahead", [lm.DEFAULT_H, 3])
@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_process_and_flush_host_memory(hip, fmt, dithered, lookahead):
    st.check_session(hip, fmt, dithered, H=lookahead)


@pytest.mark.parametrize("lookahead", [lm.DEFAULT_H, 3])
@pytest.mark.parametrize("fmt,dithered", FORMATS)
def test_process_and_flush_device_memory(hip, fmt, dithered, lookahead):
    st.check_session(hip, fmt, dithered, H=lookahead, **_device_memory())
    print("frames of r bit-identical to the mirror so far: %d" % st.compared["frames"])


def test_behind_a_stream_output_resample_host_memory(hip):
    st.check_behind_out_resample(hip)


def test_behind_a_stream_output_resample_device_memory(hip):
    st.check_behind_out_resample(hip, **_device_memory())


def test_two_runs_are_bit_identical(hip):
    st.check_reproducible(hip)
    st.check_two_runs(hip)
    st.check_two_runs(hip, **_device_memory())


def test_opt_in_host_memory(hip):
    st.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    st.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    st.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    st.check_steady_state(hip, _device_memory()["to_memory"])


def test_getters_and_refusals(hip):
    st.check_refusals(hip)
    st.check_refusals(hip, **_device_memory())


@pytest.mark.parametrize("action", ["flag_again", "flag_one", "flag_off", "setter", "lookahead", "reset", "level"])
def test_clearing(hip, action):
    st.check_clearing(hip, action)
