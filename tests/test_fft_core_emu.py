"""The FFT kernels' transform core on the CPU stand-in for the HIP runtime (tests/fft_core_cases.py)."""
import numpy as np
import pytest

import fft_core_cases as fc


def test_fft_complex_expectation_is_sound():
    """The float64 emulation of the device's fused multiply-adds, against the exactly rounded results for the test's own operands: within one
    ulp everywhere, equal on 99.9 % at least -- the slack the helper test grants is the expectation's, not the helpers'."""
    v = fc.fft_complex_operands()
    want = fc.fft_complex_expectation(v, True)
    exact = fc.fft_complex_exact(v)
    close = np.abs(want - exact) <= np.spacing(np.abs(exact).astype(np.float32))
    assert close.all()
    assert (want == exact).mean() >= 0.999
    assert not v[:16].any() and v[16:].all()


def test_fft_complex_helpers_emu(emu):
    fc.case_fft_complex_helpers(emu, fused=False)  # the stand-in's twin rounds every product (tests/emu/smst_fft_complex.h)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_fft_core_bit_identity_emu(emu, monkeypatch, name):
    fc.case_bit_identity(emu, monkeypatch, name, "emu")
