"""Packed int24, int32 and float16 frames through the batch API, and the overs counters, on the CPU stand-in: the conversion kernels
against the float64 mirror of the stated rule, code round trips, the frame calls against the planar calls, the counters against the
mirror's clamp masks, the refusals, and the command-line tool's 24-bit files.  Every comparison is exact (tests/pcm_format_cases.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import pcm_cases as pc
import pcm_format_cases as fc
from conftest import ROOT, package, synth_input


@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8, 16])
def test_s24_converter_against_mirror(emu, channels):
    """(on the parent commit the call returns -1: unknown format)"""
    fc.check_converter(emu, fc.S24, channels, range(16) if channels <= 3 else (0, 7))


@pytest.mark.parametrize("fmt", [fc.S32, fc.F16])
@pytest.mark.parametrize("channels", [1, 2, 3, 5, 8, 16])
def test_converter_against_mirror(emu, channels, fmt):
    fc.check_converter(emu, fmt, channels, (0, fc.ELEM_BYTES[fmt]))


@pytest.mark.parametrize("fmt", fc.NEW_FORMATS)
def test_converter_special_values(emu, fmt):
    fc.check_special_values(emu, fmt)


def test_s24_codes_round_trip(emu):
    """every 251st code and the 4096 at either end (all 2^24 run on the device)"""
    lo, hi = -2**23, 2**23
    fc.check_s24_codes(emu, np.unique(np.concatenate([np.arange(lo, hi, 251), np.arange(lo, lo + 4096), np.arange(hi - 4096, hi)])))


def test_f16_patterns_round_trip(emu):
    fc.check_f16_patterns(emu)


def test_s32_codes_round_trip(emu):
    fc.check_s32_codes(emu)


@pytest.mark.parametrize("fmt", fc.NEW_FORMATS)
def test_session_equals_planar(emu, fmt):
    fc.check_session(emu, 2, fmt)


@pytest.mark.parametrize("fmt", [fc.S16, fc.S24, fc.S32, fc.F16, fc.F32])
def test_overs_of_the_converter(emu, fmt):
    fc.check_overs_converter(emu, fmt)


@pytest.mark.parametrize("fmt", [fc.S16, fc.S24])
def test_overs_of_a_session(emu, fmt):
    fc.check_session_overs(emu, fmt)


def test_workspace_bytes_include_the_over_counters(emu):
    pkg = package()
    small, large = (pkg.StretchBatch(S, 2, lib=emu, **pc.GEOMETRY) for S in (1, 3))
    per_stream = (emu.smst_batch_workspace_bytes(large.h) - emu.smst_batch_workspace_bytes(small.h))/2
    assert per_stream == int(per_stream) and emu.smst_batch_workspace_bytes(small.h) > 8
    small.close()
    large.close()


def test_formats_and_strides_are_refused(emu):
    pkg = package()
    a, b = np.zeros(256, np.uint8), np.zeros(64, np.float32)
    n = np.array([4], np.int32)
    ip = n.ctypes.data_as(C.POINTER(C.c_int))
    call = lambda fmt, fs, src=a: emu.smst_debug_pcm_convert(0, 0, fmt, 1, 2, ip, C.c_void_p(src.ctypes.data if src is not None else None), 8, fs, C.c_void_p(b.ctypes.data), 16, 8)
    for fmt in (fc.S24, fc.S32, fc.F16):
        assert call(fmt, 2) == 0
        assert call(fmt, 1) == -1 and b"frame stride" in emu.smst_last_error()
        assert call(fmt, 2, None) == -1
    for fmt in (0, 3, 7, 8):
        assert call(fmt, 2) == -1 and b"format" in emu.smst_last_error()
    bt = pkg.StretchBatch(2, 2, lib=emu, **pc.GEOMETRY)
    x = np.zeros((2, 64, 2, 3), np.uint8)
    n2 = np.array([64, 64], np.int32)
    ip2 = n2.ctypes.data_as(C.POINTER(C.c_int))
    px, null = C.c_void_p(x.ctypes.data), C.c_void_p(None)
    for fmt in (0, 3, 7, 8):
        assert emu.smst_batch_process_pcm(bt.h, px, 128, 2, ip2, px, 128, 2, ip2, fmt, pkg.MEM_HOST) == -1 and b"format" in emu.smst_last_error()
        assert emu.smst_batch_seek_pcm(bt.h, px, 128, 2, ip2, None, fmt, pkg.MEM_HOST) == -1 and b"format" in emu.smst_last_error()
        assert emu.smst_batch_flush_pcm(bt.h, px, 128, 2, ip2, None, fmt, pkg.MEM_HOST) == -1 and b"format" in emu.smst_last_error()
        assert emu.smst_batch_output_seek_pcm(bt.h, px, 128, 2, ip2, fmt, pkg.MEM_HOST) == -1 and b"format" in emu.smst_last_error()
    assert emu.smst_batch_process_pcm(bt.h, px, 128, 1, ip2, px, 128, 2, ip2, fc.S24, pkg.MEM_HOST) == -1 and b"frame stride" in emu.smst_last_error()
    assert emu.smst_batch_process_pcm(bt.h, null, 128, 2, ip2, px, 128, 2, ip2, fc.S24, pkg.MEM_HOST) == -1 and b"null buffer" in emu.smst_last_error()
    assert emu.smst_batch_flush_pcm(bt.h, null, 128, 2, ip2, None, fc.F16, pkg.MEM_HOST) == -1
    # packed int24 whose frames are 7 bytes apart: no whole number of elements
    base = np.zeros((2, 64, 7), np.uint8)
    crooked = np.lib.stride_tricks.as_strided(base, shape=(2, 64, 2, 3), strides=(64*7, 7, 3, 1))
    with pytest.raises(pkg.StretchError, match="3 bytes"):
        bt.processFrames(crooked, 64)
    with pytest.raises(pkg.StretchError):
        bt.processFrames(np.zeros((2, 64, 2), np.int8), 64)
    with pytest.raises(pkg.StretchError):
        bt.flushFrames(10, dtype=np.int8)
    bt.close()


def test_strided_s24_frames_in_host_memory(emu):
    """frameStride > C for packed int24 in host memory: the result of dense frames, the gaps of the output untouched"""
    pkg = package()
    S, Cn, n = 3, 2, 700
    frames = fc.encode_frames(pc.inputs(S, Cn, n, pc.F32)[0], fc.S24)
    wide_in = np.zeros((S, n, Cn + 1, 3), np.uint8)
    wide_in[:, :, :Cn] = frames
    wide_out = np.full((S, n, Cn + 1, 3), 0x5A, np.uint8)
    b1, b2 = (pkg.StretchBatch(S, Cn, lib=emu, **pc.GEOMETRY) for _ in range(2))
    dense = b1.processFrames(frames, [n, 300, 0])
    assert dense.dtype == np.uint8 and dense.shape == (S, n, Cn, 3)
    b2.processFrames(wide_in[:, :, :Cn], [n, 300, 0], out=wide_out[:, :, :Cn])
    assert np.array_equal(wide_out[0, :, :Cn], dense[0]) and np.array_equal(wide_out[1, :300, :Cn], dense[1, :300]) and dense[0].any()
    assert (wide_out[:, :, Cn] == 0x5A).all() and (wide_out[1, 300:] == 0x5A).all() and (wide_out[2] == 0x5A).all()
    b1.close()
    b2.close()


# ---- the command-line tool ------------------------------------------------------------------------------------------------------------

def data_chunk(path):
    raw = open(path, "rb").read()
    pos = 12
    fmt = None
    while pos + 8 <= len(raw):
        tag, size = raw[pos:pos + 4], struct.unpack("<I", raw[pos + 4:pos + 8])[0]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", raw[pos + 8:pos + 24])
        if tag == b"data":
            return fmt, raw[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    raise ValueError("no data chunk")


def cli_out_format_cases(cli, tmp_path):
    """--out-format s24: the data chunk is the mirror of the float the run produced (taken from --out-format f32); without the option the
    file is what --out-format s16 writes and the int16 mirror of the same float: today's bytes."""
    from test_cli import write_wav16
    sr = 48000
    src = str(tmp_path/"in.wav")
    write_wav16(src, 1.2*synth_input(1, 2, 6001, sr), sr)      # (clips: the clamp is part of the rule)
    outs = {}
    for name, flags in (("default", []), ("s16", ["--out-format=s16"]), ("s24", ["--out-format", "s24"]), ("f32", ["--out-format=f32"])):
        outs[name] = str(tmp_path/(name + ".wav"))
        res = subprocess.run([cli, "--time=1.1", "--semitones=2"] + flags + [src, outs[name]], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
    fmt, data = data_chunk(outs["f32"])
    assert fmt[:2] == (3, 2) and fmt[5] == 32
    x = np.frombuffer(data, "<f4")
    assert len(x) == 2*round(6001*1.1) and np.abs(x).max() > 0.5
    fmt, data = data_chunk(outs["s24"])
    assert fmt == (1, 2, sr, sr*6, 6, 24)
    assert np.array_equal(np.frombuffer(data, np.uint8).reshape(-1, 3), fc.to_rows(fc.mirror(x, fc.S24)[0], fc.S24))
    fmt, data = data_chunk(outs["default"])
    assert fmt == (1, 2, sr, sr*4, 4, 16)
    assert np.array_equal(np.frombuffer(data, "<i2"), fc.mirror(x, fc.S16)[0])
    assert open(outs["default"], "rb").read() == open(outs["s16"], "rb").read()
    assert subprocess.run([cli, "--out-format=s8", src, outs["s16"]], capture_output=True).returncode != 0


def test_cli_out_format_emulated(emu, tmp_path):
    exe = str(tmp_path/"stretch_cli_emu")
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.run(["g++", "-std=c++11", "-O2", os.path.join(ROOT, "tools", "stretch_cli.cpp"), "-o", exe, "-L" + emu_dir,
                    "-l:libsmst_emu.so", "-Wl,-rpath," + emu_dir], check=True)
    cli_out_format_cases(exe, tmp_path)
