"""The sample-rate converter behind the engine in smst_batch_exact_pcm (include/smst.h, "Output resample") on the CPU stand-in: the numpy
mirror against the known answers and what defines E; the library's lengths; the kernel against the mirror bit for bit, with the source's
join in every position; whole clips through exactFrames against a twin batch that renders E frames; the level chain behind the converter
against the existing hooks on the mirror's image; the opt-in, the steady state, the refusals and the command-line tool
(tests/out_resample_cases.py has the mirror and the checks).  On a library without the new entry points every test but the mirror's own
fails at its first call."""
import os
import subprocess

import pytest

import out_resample_cases as oc
import pcm_format_cases as fc
import resample_cases as rs
from conftest import ROOT


def test_mirror_known_answers_and_render_length():
    oc.check_mirror()


def test_render_length(emu):
    oc.check_lengths(emu)


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
@pytest.mark.parametrize("up,down", rs.RATIOS)
def test_kernel_against_mirror(emu, up, down, channels):
    oc.check_kernel(emu, up, down, channels)


def test_eight_ratios_in_one_launch(emu):
    oc.check_mixed(emu)


@pytest.mark.parametrize("fmt,dithered", [(fc.S16, True), (fc.S24, True), (fc.S32, False), (fc.F16, False), (fc.F32, False)])
def test_whole_clips(emu, fmt, dithered):
    oc.check_clips(emu, fmt, dithered, calls=1)


def test_chain_runs_on_the_delivered_frames(emu):
    oc.check_chain(emu, calls=1)


def test_opt_in(emu):
    oc.check_opt_in(emu)


def test_steady_state(emu):
    oc.check_steady_state(emu)


def test_two_runs_are_bit_identical(emu):
    oc.check_reproducible(emu)


def test_refusals(emu):
    oc.check_refusals(emu)


def test_cli_out_resample_emulated(emu, tmp_path):
    exe = str(tmp_path/"stretch_cli_emu")
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tools", "stretch_cli.cpp"), "-o", exe, "-L" + emu_dir,
                    "-l:libsmst_emu.so", "-Wl,-rpath," + emu_dir], check=True)
    oc.check_cli(exe, tmp_path, emu)
