"""The sample-rate converter's streaming form behind smst_batch_process_pcm / _flush_pcm (include/smst.h, "Stream output resample") on the
CPU stand-in: the streaming model against the known answers, the clip mirror and the line bound; the kernel hook against the model bit for
bit, at 64-bit positions and with eight ratios in one sequence of calls; processFrames and flushFrames against a twin batch whose output the
model resamples, with the stream limiter, the stream meter, the input setting, and across reset and seek; the opt-in, the steady state and
the refusals (tests/stream_out_resample_cases.py has the model and the checks).  On a library without the new entry points every test but
the model's own fails at its first call."""
import pytest

import pcm_format_cases as fc
import resample_cases as rs
import stream_out_resample_cases as so


def test_model_known_answers_clip_mirror_and_line_bound():
    so.check_mirror()


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("up,down", rs.RATIOS)
def test_hook_against_model(emu, up, down, channels):
    so.check_hook(emu, up, down, channels)


def test_hook_known_answers(emu):
    so.check_known_answers(emu)


def test_positions_beyond_32_bits(emu):
    so.check_far_positions(emu)


def test_eight_ratios_and_two_plain_streams(emu):
    so.check_mixed(emu)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, True), (fc.S24, True), (fc.S32, False), (fc.F16, False), (fc.F32, False)])
def test_session_against_twin(emu, fmt, dithered):
    so.check_session(emu, fmt, dithered)


def test_session_with_stream_limiter(emu):
    so.check_session(emu, fc.F32, False, limiter=True)


def test_session_with_stream_meter(emu):
    so.check_session(emu, fc.F32, False, meter=True)


def test_session_with_input_stream_resample(emu):
    so.check_session(emu, fc.S16, True, resample_in=True)


def test_reset_clears_the_line_and_seek_does_not(emu):
    so.check_session(emu, fc.S16, True, seek=True)


def test_opt_in(emu):
    so.check_opt_in(emu)


def test_steady_state(emu):
    so.check_steady_state(emu)


def test_two_runs_are_bit_identical_and_getters(emu):
    so.check_reproducible(emu)


def test_refusals(emu):
    so.check_refusals(emu)
