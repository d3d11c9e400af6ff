"""The stream meter of the frame output (include/smst.h, "Stream meter") on the device: cut invariance and the equality with the clip meters
bit for bit in every update form, readings mid-programme, the true-peak edge, the capacity, NaN and inf, a second rate, the float64 numpy
mirrors, processFrames and flushFrames end to end in host and in device memory, two runs, the opt-in, the steady state, the refusals and the
clearing rules (tests/stream_meter_cases.py has the checks).  On a library without the stream meter's entry points every test fails at its
first call.

Every comparison with the clip meters is one of bit patterns."""
import pytest

import stream_meter_cases as sm

pytestmark = pytest.mark.gpu


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("kind", sm.CUTS)
@pytest.mark.parametrize("channels", [1, 2, 3])
def test_cut_invariance_and_clip_equivalence(hip, channels, kind):
    sm.check_cut(hip, sm.FS, channels, kind)


@pytest.mark.parametrize("kind", sm.CUTS)
def test_cut_invariance_and_clip_equivalence_stable_rate(hip, kind):
    sm.check_cut(hip, sm.FS_STABLE, 2, kind)
    print("readings bit-identical to the clip meters so far: %d" % sm.compared["readings"])


def test_cut_invariance_16_channels(hip):
    sm.check_cut(hip, sm.FS, 16, "ragged")


def test_the_stable_programme_discriminates(hip):
    sm.check_discriminates(hip)


def test_weights_and_an_unmetered_stream(hip):
    sm.check_weights_and_unmetered(hip)


@pytest.mark.parametrize("form", sm.FORMS)
@pytest.mark.parametrize("fs", [sm.FS, sm.FS_STABLE])
def test_mid_programme_readings(hip, fs, form):
    sm.check_mid_readings(hip, fs, 2, form)


@pytest.mark.parametrize("form", sm.FORMS)
def test_true_peak_edge(hip, form):
    sm.check_true_peak_edge(hip, form)


@pytest.mark.parametrize("form", sm.FORMS)
def test_capacity(hip, form):
    sm.check_capacity(hip, form)


@pytest.mark.parametrize("form", sm.FORMS)
@pytest.mark.parametrize("fs", [sm.FS, sm.FS_STABLE])
def test_nan_and_inf(hip, fs, form):
    sm.check_nan_inf(hip, fs, form)


@pytest.mark.parametrize("form", sm.FORMS)
def test_second_rate(hip, form):
    sm.check_second_rate(hip, form)


def test_against_the_numpy_mirrors(hip):
    sm.check_against_mirrors(hip)


def test_two_runs_are_bit_identical(hip):
    sm.check_reproducible(hip)


def test_hook_refusals(hip):
    sm.check_hook_refusals(hip)


@pytest.mark.parametrize("fs", [sm.E2E_FS, sm.E2E_FS_STABLE])
def test_process_and_flush_host_memory(hip, fs):
    sm.check_e2e(hip, fs)


@pytest.mark.parametrize("fs", [sm.E2E_FS, sm.E2E_FS_STABLE])
def test_process_and_flush_device_memory(hip, fs):
    sm.check_e2e(hip, fs, **_device_memory())


@pytest.mark.parametrize("fmt,dithered", sm.FORMATS)
def test_the_meter_changes_no_output_byte_host_memory(hip, fmt, dithered):
    sm.check_e2e_bytes(hip, fmt, dithered)


@pytest.mark.parametrize("fmt,dithered", sm.FORMATS)
def test_the_meter_changes_no_output_byte_device_memory(hip, fmt, dithered):
    sm.check_e2e_bytes(hip, fmt, dithered, **_device_memory())


def test_opt_in_host_memory(hip):
    sm.check_opt_in(hip)


def test_opt_in_device_memory(hip):
    sm.check_opt_in(hip, **_device_memory())


def test_steady_state_host_memory(hip):
    sm.check_steady_state(hip)


def test_steady_state_device_memory(hip):
    sm.check_steady_state(hip, _device_memory()["to_memory"])


def test_refusals_and_getters(hip):
    sm.check_refusals(hip)
    sm.check_refusals(hip, **_device_memory())


@pytest.mark.parametrize("action", ["setter", "setter_one", "reset", "level"])
def test_clearing(hip, action):
    sm.check_clearing(hip, action)
