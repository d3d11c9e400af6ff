"""The loudness-range meter of the frame output (include/smst.h, "Loudness range") on the CPU stand-in: the numpy mirror against the known
answers, the range stage against the mirror, the selection bit for bit, the content cases, the caps, whole clips through exactFrames,
the opt-in, the steady state, the refusals and the command-line tool (tests/loudness_range_cases.py has the mirror and the checks).  On a
library without the new entry points every test but the mirror's own fails at its first call."""
import os
import subprocess

import pytest

import loudness_range_cases as lr
import pcm_format_cases as fc
from conftest import ROOT


def test_mirror_known_answers():
    lr.check_mirror()


@pytest.mark.parametrize("fs,channels", [(8000, 1), (8000, 2), (8000, 3), (8000, 16), (5120, 2)])
def test_stage_against_mirror(emu, fs, channels):
    lr.check_hook(emu, fs, channels)


def test_lowest_rate_where_the_hop_is_the_chunk(emu):
    lr.check_hook_lowest_rate(emu)


def test_selection_is_exact(emu):
    lr.check_selection(emu)


def test_gates_maxima_and_undefined_cases(emu):
    lr.check_content(emu)


def test_caps(emu):
    lr.check_caps(emu)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, True), (fc.S16, False), (fc.S24, True), (fc.F32, False)])
def test_whole_clips(emu, fmt, dithered):
    lr.check_clips(emu, fmt, dithered, calls=1)      # (the device tests call twice; test_steady_state repeats calls here)


def test_two_runs_are_bit_identical(emu):
    lr.check_reproducible(emu)
    lr.check_two_runs(emu)


def test_opt_in(emu):
    lr.check_opt_in(emu)


def test_steady_state(emu):
    lr.check_steady_state(emu)


def test_refusals(emu):
    lr.check_refusals(emu)


def test_meter_and_caps_are_refused_in_streaming_calls(emu):
    lr.check_refused_in_streaming_calls(emu)


def test_cli_loudness_range_emulated(emu, tmp_path):
    exe = str(tmp_path/"stretch_cli_emu")
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tools", "stretch_cli.cpp"), "-o", exe, "-L" + emu_dir,
                    "-l:libsmst_emu.so", "-Wl,-rpath," + emu_dir], check=True)
    lr.check_cli(exe, tmp_path)
