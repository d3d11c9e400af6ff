"""Interleaved PCM through the batch API on the device: the conversion kernels against the float64 mirror of the stated rule, the frame
calls against the planar calls in host and in device memory, torch int16 tensors ordered by events only, and the launch counters.
Every comparison is exact (tests/pcm_cases.py)."""
import numpy as np
import pytest

import pcm_cases as pc
from conftest import package

pytestmark = pytest.mark.gpu

ANALYSE = ("analyse_teams", "analyse_fast", "analyse_generic")
SYNTH = ("synth_teams", "synth_fast", "synth_generic", "synth_emit", "emit_carried")


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_converter_against_mirror(hip, channels):
    pc.check_converter(hip, channels)


def test_converter_special_values_and_all_codes(hip):
    pc.check_special_values(hip)
    pc.check_all_codes(hip)


@pytest.mark.parametrize("fmt", [pc.F32, pc.S16])
def test_session_equals_planar_host_memory(hip, fmt):
    pc.check_session(hip, 2, fmt)


@pytest.mark.parametrize("fmt", [pc.F32, pc.S16])
def test_session_equals_planar_device_memory(hip, fmt):
    import torch
    pc.check_session(hip, 2, fmt, to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


def test_torch_int16_frames_ordered_by_events(hip):
    """processFrames on torch int16 tensors: the producer (the upload and a torch op on torch's stream) and the consumer (.cpu()) are
    ordered against the batch's streams by events alone -- no synchronize() anywhere."""
    import torch
    pkg = package()
    S, Cn, n = 3, 2, 6000
    frames, planar = pc.inputs(S, Cn, 2*n, pc.S16)
    ref = pkg.StretchBatch(S, Cn, lib=hip, **pc.GEOMETRY)
    b = pkg.StretchBatch(S, Cn, lib=hip, **pc.GEOMETRY)
    for k, (nout, nin) in enumerate((([7000, 3000, 0], [n, 2500, 0]), ([6100, 129, 515], [n, 128, 500]))):
        want = pc.expect_frames(ref.process(np.ascontiguousarray(planar[:, :, k*n:(k + 1)*n]), nout, in_samples=nin), pc.S16)
        half = torch.from_numpy(np.ascontiguousarray(frames[:, k*n:(k + 1)*n]//2)).cuda()
        x = half*2 + torch.from_numpy(np.ascontiguousarray(frames[:, k*n:(k + 1)*n] % 2)).cuda()  # produced by a kernel on torch's stream
        y = b.processFrames(x, nout, in_samples=nin)
        assert y.dtype == torch.int16 and tuple(y.shape) == want.shape
        got = (y + 0).cpu().numpy()                                                              # consumed by a kernel on torch's stream
        assert np.array_equal(got, want), k
    b.synchronize()
    ref.close()
    b.close()


def test_launch_counters(hip):
    pkg = package()
    S, Cn, n = 3, 2, 4000
    frames, planar = pc.inputs(S, Cn, n, pc.S16)
    count = lambda names: sum(pkg.launch_count(k, hip) for k in names)
    assert pkg.launch_count("pcm_in", hip) >= 0 and pkg.launch_count("pcm_out", hip) >= 0
    a = pkg.StretchBatch(S, Cn, lib=hip, **pc.GEOMETRY)
    before = (count(ANALYSE), count(SYNTH))
    a.process(planar, [n, 3000, 0])
    planar_grew = (count(ANALYSE) - before[0], count(SYNTH) - before[1])
    b = pkg.StretchBatch(S, Cn, lib=hip, **pc.GEOMETRY)
    before = (count(ANALYSE), count(SYNTH), pkg.launch_count("pcm_in", hip), pkg.launch_count("pcm_out", hip))
    b.processFrames(frames, [n, 3000, 0])
    grew = (count(ANALYSE) - before[0], count(SYNTH) - before[1], pkg.launch_count("pcm_in", hip) - before[2], pkg.launch_count("pcm_out", hip) - before[3])
    assert grew == planar_grew + (1, 1) and planar_grew[0] > 0 and planar_grew[1] > 0, (grew, planar_grew)
    before = (pkg.launch_count("pcm_in", hip), pkg.launch_count("pcm_out", hip))
    b.seekFrames(frames[:, :640], 1.0)                   # one input conversion
    b.flushFrames([100, -1, 0])                          # one output conversion
    b.processFrames(frames[:, :0], [64, 64, 64])         # no input frames: only the output is converted
    assert (pkg.launch_count("pcm_in", hip) - before[0], pkg.launch_count("pcm_out", hip) - before[1]) == (1, 2)
    a.close()
    b.close()
