"""The sample-rate converter in front of smst_batch_exact_pcm (include/smst.h, "Resample") on the CPU stand-in: the numpy mirror against the
known answers, its frequency response and two sines; the library's table against the formula; the kernel against the mirror bit for bit;
whole clips through exactFrames against a twin batch fed the mirror's frames; the opt-in, the steady state, the refusals and the
command-line tool (tests/resample_cases.py has the mirror and the checks).  On a library without the new entry points every test but the
mirror's own fails at its first call."""
import os
import subprocess

import pytest

import pcm_format_cases as fc
import resample_cases as rs
from conftest import ROOT


def test_mirror_known_answers():
    rs.check_mirror()


def test_mirror_frequency_response():
    rs.check_response()


def test_mirror_sines():
    rs.check_sines()


@pytest.mark.parametrize("up,down", rs.TABLE_RATIOS)
def test_table_against_formula(emu, up, down):
    rs.check_table(emu, up, down)


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("up,down", rs.RATIOS)
def test_kernel_against_mirror(emu, up, down, channels):
    rs.check_kernel(emu, up, down, channels)


def test_eight_ratios_in_one_launch(emu):
    rs.check_mixed(emu)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, True), (fc.S24, True), (fc.S32, False), (fc.F16, False), (fc.F32, False)])
def test_whole_clips(emu, fmt, dithered):
    rs.check_clips(emu, fmt, dithered, calls=1)


def test_whole_clips_loudness_true_peak_limiter(emu):
    rs.check_clips(emu, fc.F32, False, chain=True, calls=1)


def test_opt_in(emu):
    rs.check_opt_in(emu)


def test_steady_state(emu):
    rs.check_steady_state(emu)


def test_two_runs_are_bit_identical(emu):
    rs.check_reproducible(emu)


def test_refusals(emu):
    rs.check_refusals(emu)


def test_cli_resample_emulated(emu, tmp_path):
    exe = str(tmp_path/"stretch_cli_emu")
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tools", "stretch_cli.cpp"), "-o", exe, "-L" + emu_dir,
                    "-l:libsmst_emu.so", "-Wl,-rpath," + emu_dir], check=True)
    rs.check_cli(exe, tmp_path, emu)
