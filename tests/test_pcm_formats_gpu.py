"""Packed int24, int32 and float16 frames through the batch API, and the overs counters, on the device: the conversion kernels against
the float64 mirror of the stated rule, every code of the three formats there and back, the frame calls against the planar calls in host and
in device memory, float16 tensors ordered by events only, the counters, the launch counters and the command-line tool's 24-bit files.
Every comparison is exact (tests/pcm_format_cases.py)."""
import os

import numpy as np
import pytest

import pcm_cases as pc
import pcm_format_cases as fc
from conftest import package

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_s24_converter_against_mirror(hip, channels):
    """(on the parent commit the call returns -1: unknown format)"""
    fc.check_converter(hip, fc.S24, channels, range(16) if channels <= 3 else (0, 7))


@pytest.mark.parametrize("fmt", [fc.S32, fc.F16])
@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_converter_against_mirror(hip, channels, fmt):
    fc.check_converter(hip, fmt, channels, (0, fc.ELEM_BYTES[fmt]))


@pytest.mark.parametrize("fmt", fc.NEW_FORMATS)
def test_converter_special_values(hip, fmt):
    fc.check_special_values(hip, fmt)


def test_all_s24_codes_round_trip(hip):
    """all 2^24 codes, one call per direction"""
    fc.check_s24_codes(hip, np.arange(-2**23, 2**23, dtype=np.int32))


def test_f16_patterns_and_s32_codes_round_trip(hip):
    fc.check_f16_patterns(hip)
    fc.check_s32_codes(hip)


@pytest.mark.parametrize("fmt", fc.NEW_FORMATS)
def test_session_equals_planar_host_memory(hip, fmt):
    fc.check_session(hip, 2, fmt)


@pytest.mark.parametrize("fmt", fc.NEW_FORMATS)
def test_session_equals_planar_device_memory(hip, fmt):
    import torch
    fc.check_session(hip, 2, fmt, to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def test_torch_float16_frames_ordered_by_events(hip):
    """processFrames on torch float16 tensors: the producer (the upload and a torch op on torch's stream) and the consumer (a torch op and
    .cpu()) are ordered against the batch's streams by events alone -- no synchronize() anywhere."""
    import torch
    pkg = package()
    S, Cn, n = 3, 2, 6000
    frames = fc.encode_frames(pc.inputs(S, Cn, 2*n, pc.F32)[0], fc.F16)
    planar = np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fc.F16), (0, 2, 1)))
    ref = pkg.StretchBatch(S, Cn, lib=hip, **pc.GEOMETRY)
    b = pkg.StretchBatch(S, Cn, lib=hip, **pc.GEOMETRY)
    for k, (nout, nin) in enumerate((([7000, 3000, 0], [n, 2500, 0]), ([6100, 129, 515], [n, 128, 500]))):
        want = fc.encode_frames(pc.frames_of(ref.process(np.ascontiguousarray(planar[:, :, k*n:(k + 1)*n]), nout, in_samples=nin)), fc.F16)
        x = torch.from_numpy(np.ascontiguousarray(frames[:, k*n:(k + 1)*n])).cuda()*1   # produced by a kernel on torch's stream (x*1 is exact)
        y = b.processFrames(x, nout, in_samples=nin)
        assert y.dtype == torch.float16 and tuple(y.shape) == want.shape
        got = (y*1).cpu().numpy()                                                       # consumed by a kernel on torch's stream
        assert fc.same_values(got, want, fc.F16) and got.any(), k
    b.synchronize()
    ref.close()
    b.close()


@pytest.mark.parametrize("fmt", [fc.S16, fc.S24, fc.S32, fc.F16, fc.F32])
def test_overs_of_the_converter(hip, fmt):
    fc.check_overs_converter(hip, fmt)


@pytest.mark.parametrize("fmt", [fc.S16, fc.S24])
def test_overs_of_a_session(hip, fmt):
    fc.check_session_overs(hip, fmt)


def test_overs_of_device_memory_frames(hip):
    """the counters of an asynchronous device-memory call: takePcmOvers synchronises the batch before it reads them"""
    import torch
    pkg = package()
    S, Cn, n = 3, 2, 3000
    x = pc.inputs(S, Cn, n, pc.F32)[0]*np.array([4.0, 0.25, 1.0], np.float32)[:, None, None]
    frames = fc.encode_frames(x, fc.S24)
    planar = np.ascontiguousarray(np.transpose(fc.decode_frames(frames, fc.S24), (0, 2, 1)))
    ref, b = (pkg.StretchBatch(S, Cn, lib=hip, **pc.GEOMETRY) for _ in range(2))
    want = ref.process(planar, [n, 2000, 0])
    b.processFrames(torch.from_numpy(frames).cuda(), [n, 2000, 0])
    clamped, nans = b.takePcmOvers()
    expect = [int(fc.mirror(want[s, :, :k], fc.S24)[1].sum()) for s, k in enumerate([n, 2000, 0])]
    assert clamped.tolist() == expect and expect[0] > 0 and expect[1] == 0 and nans.tolist() == [0, 0, 0], (clamped.tolist(), expect)
    ref.close()
    b.close()


@pytest.mark.parametrize("fmt", fc.NEW_FORMATS)
def test_launch_counters(hip, fmt):
    """one pcm_in and one pcm_out launch per processFrames call, whatever the format"""
    pkg = package()
    S, Cn, n = 3, 2, 4000
    frames = fc.encode_frames(pc.inputs(S, Cn, n, pc.F32)[0], fmt)
    b = pkg.StretchBatch(S, Cn, lib=hip, **pc.GEOMETRY)
    before = (pkg.launch_count("pcm_in", hip), pkg.launch_count("pcm_out", hip))
    b.processFrames(frames, [n, 3000, 0])
    assert (pkg.launch_count("pcm_in", hip) - before[0], pkg.launch_count("pcm_out", hip) - before[1]) == (1, 1)
    before = (pkg.launch_count("pcm_in", hip), pkg.launch_count("pcm_out", hip))
    b.seekFrames(frames[:, :640], 1.0)                                  # one input conversion
    b.flushFrames([100, -1, 0], dtype=fc.frame_dtype(fmt))              # one output conversion
    b.processFrames(frames[:, :0], [64, 64, 64])                        # no input frames: only the output is converted
    assert (pkg.launch_count("pcm_in", hip) - before[0], pkg.launch_count("pcm_out", hip) - before[1]) == (1, 2)
    b.close()


def test_cli_out_format_gpu(tmp_path):
    from test_pcm_formats_emu import cli_out_format_cases
    pkg = package()
    exe = os.path.join(os.path.dirname(pkg.LIBRARY_PATH), "stretch_cli")
    assert os.path.exists(exe), "stretch_cli not built (csrc/Makefile)"
    cli_out_format_cases(exe, tmp_path)
