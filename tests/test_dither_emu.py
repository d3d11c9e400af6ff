"""TPDF dither of the int16 / int24 output of the batch PCM calls, on the CPU stand-in: the numpy mirror of include/smst.h against the
header's known answers, the statistics the specification promises, the dithered conversion kernel against the mirror, sessions and whole
clips against the mirror of the planar calls' output, the refusals, and the command-line tool.  Every comparison with the mirror is exact
(tests/dither_cases.py); on a library without the dither entry points every test but the first fails at its first call."""
import os
import subprocess

import pytest

import dither_cases as dc
import pcm_format_cases as fc
from conftest import ROOT


def test_mirror_known_answers():
    dc.check_known_answers()


@pytest.mark.parametrize("seed", [0, 1, 12345, -7])
@pytest.mark.parametrize("mode", dc.MODES)
def test_statistics_of_the_specification(emu, mode, seed):
    dc.check_statistics(emu, mode, seed)


def test_constant_below_one_lsb(emu):
    dc.check_constant_below_one_lsb(emu)


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8, 16])
def test_s16_converter_against_mirror(emu, channels):
    dc.check_converter(emu, fc.S16, channels, (0, 2))


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8, 16])
def test_s24_converter_against_mirror(emu, channels):
    dc.check_converter(emu, fc.S24, channels, range(16) if channels <= 3 else (0, 3))


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_session_equals_mirror_of_planar(emu, fmt):
    dc.check_session(emu, fmt)


def test_session_cut_into_other_calls(emu):
    dc.check_recut(emu, fc.S16)


def test_set_dither_restarts_the_counter(emu):
    dc.check_restart(emu)


@pytest.mark.parametrize("fmt", [fc.S32, fc.F16, fc.F32])
def test_other_formats_are_unchanged(emu, fmt):
    dc.check_other_formats_unchanged(emu, fmt)


def test_steady_state_and_launch_counters(emu):
    dc.check_steady_state_and_launches(emu)


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips(emu, fmt):
    dc.check_clips(emu, fmt)


@pytest.mark.parametrize("fmt", dc.DITHERED_FORMATS)
def test_whole_clips_wide_output(emu, fmt):
    dc.check_clips(emu, fmt, wide=True)


def test_refusals(emu):
    dc.check_refusals(emu)


def test_cli_dither_emulated(emu, tmp_path):
    exe = str(tmp_path/"stretch_cli_emu")
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tools", "stretch_cli.cpp"), "-o", exe, "-L" + emu_dir,
                    "-l:libsmst_emu.so", "-Wl,-rpath," + emu_dir], check=True)
    dc.check_cli(exe, tmp_path)
