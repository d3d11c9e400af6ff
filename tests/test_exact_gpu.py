"""Whole clips of ragged lengths and rates in one call (smst_batch_exact / smst_batch_exact_pcm) on the device: the cases of
test_exact_emu.py (tests/exact_cases.py), host memory and torch tensors in device memory.  Every comparison is exact (the reference leg has
parity_cases' caps)."""
import numpy as np
import pytest

import exact_cases as xc
import pcm_format_cases as pf
from conftest import package

pytestmark = pytest.mark.gpu

FORMATS = (xc.PLANAR,) + xc.FRAME_FORMATS


def device_exact(batch, x, nout, nin, frames=False):
    """the call on torch tensors in device memory, ordered against torch's stream by events only (no synchronize() before the read)"""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out, ok = (batch.exactFrames if frames else batch.exact)(xt, nout, in_samples=nin)
    return out.cpu().numpy(), ok


def _run(memory):
    return xc.host_exact if memory == "host" else device_exact


@pytest.mark.parametrize("channels", [1, 2, 3, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_clip_kernels_against_mirror(hip, fmt, channels):
    sweep = channels == 2                                # every alignment of the caller's buffer with every alignment of the image
    xc.check_clip_kernels(hip, fmt, channels, xc.sub_alignments(fmt) if sweep else (0, 4 if fmt == xc.PLANAR else pf.ELEM_BYTES[fmt]),
                          image_offsets=xc.IMAGE_ALIGNMENTS if sweep else (1,))


@pytest.mark.parametrize("fmt", xc.FRAME_FORMATS)
def test_clip_kernels_with_wide_frames(hip, fmt):
    xc.check_clip_kernels(hip, fmt, 2, (0, pf.ELEM_BYTES[fmt]), wide_frames=True)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("memory", ["host", "device"])
def test_exact_equals_single_handles(hip, memory, split):
    xc.check_equals_single_handles(hip, 2, xc.CLIPS, split, run=_run(memory))


def test_exact_equals_single_handles_three_channels(hip):
    xc.check_equals_single_handles(hip, 3, xc.CLIPS_UNITY, False, run=device_exact)


@pytest.mark.parametrize("split", [False, True])
def test_exact_against_the_reference(hip, ref, split):
    if getattr(ref, "is_port", False):
        pytest.skip("the plain port does not restate exact()")
    xc.check_against_reference(hip, ref, split)


@pytest.mark.parametrize("split", [False, True])
def test_short_and_left_out_streams_keep_their_state(hip, split):
    xc.check_masks(hip, split)


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("fmt", xc.FRAME_FORMATS)
def test_exact_frames_equal_planar(hip, fmt, memory):
    run = _run(memory)
    xc.check_frames_equal_planar(hip, fmt, run_frames=lambda b, x, nout, nin: run(b, x, nout, nin, frames=True), run_planar=run)


def test_exact_refusals(hip):
    xc.check_refusals(hip)


@pytest.mark.parametrize("memory", ["host", "device"])
@pytest.mark.parametrize("frames", [False, True])
def test_exact_does_not_allocate_in_steady_state(hip, frames, memory):
    run = _run(memory)
    xc.check_steady_state(hip, lambda b, x, nout, nin: run(b, x, nout, nin, frames=frames), frames=frames)


def test_exact_runs_one_main_process(hip):
    xc.check_one_main_process(hip, device_exact)


def test_left_out_stream_in_device_memory(hip):
    """a torch output tensor keeps its sentinel where a stream is left out or a count ends, and the short stream comes back as zeros"""
    import torch
    nin, nout = list(xc.CLIPS["inputs"]), list(xc.CLIPS["outputs"])
    nout[4] = -1
    x = xc.clip_inputs(2, nin)
    b = package().StretchBatch(len(nin), 2, lib=hip, seed=9, **xc.GEOMETRY)
    out = torch.full((len(nin), 2, max(nout) + 5), 777.0, dtype=torch.float32, device="cuda:0")
    _, ok = b.exact(torch.from_numpy(x).cuda(), nout, in_samples=nin, out=out)
    y = out.cpu().numpy()
    assert ok.tolist() == [True, True, False, True, False]
    assert (y[4] == 777.0).all() and (y[2, :, :nout[2]] == 0).all()
    for s in range(4):
        assert (y[s, :, nout[s]:] == 777.0).all() and (s == 2 or np.any(y[s, :, :nout[s]] != 0))
    b.close()
