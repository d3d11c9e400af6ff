"""The sample-rate converter's streaming form in front of smst_batch_process_pcm / _seek_pcm (include/smst.h, "Stream resample") on the CPU
stand-in: the streaming model against the known answers and the clip mirror; the kernel hook against the model bit for bit, at 64-bit
positions and with eight ratios in one sequence of calls; processFrames and seekFrames against a twin batch fed the model's frames; the
opt-in, the steady state and the refusals (tests/stream_resample_cases.py has the model and the checks).  On a library without the new
entry points every test but the model's own fails at its first call."""
import pytest

import pcm_format_cases as fc
import resample_cases as rs
import stream_resample_cases as sr


def test_model_known_answers_and_clip_mirror():
    sr.check_mirror()


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("up,down", rs.RATIOS)
def test_hook_against_model(emu, up, down, channels):
    sr.check_hook(emu, up, down, channels)


def test_positions_beyond_32_bits(emu):
    sr.check_far_positions(emu)


def test_eight_ratios_and_two_plain_streams(emu):
    sr.check_mixed(emu)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, True), (fc.S24, True), (fc.S32, False), (fc.F16, False), (fc.F32, False)])
def test_process_frames_against_twin(emu, fmt, dithered):
    sr.check_session(emu, fmt, dithered)


def test_process_frames_with_stream_limiter(emu):
    sr.check_session(emu, fc.F32, False, limiter=True)


def test_reset_and_seek_clear_the_line(emu):
    sr.check_session(emu, fc.S16, True, seek=True)


def test_opt_in(emu):
    sr.check_opt_in(emu)


def test_steady_state(emu):
    sr.check_steady_state(emu)


def test_two_runs_are_bit_identical_and_frames_need(emu):
    sr.check_reproducible(emu)


def test_refusals(emu):
    sr.check_refusals(emu)
