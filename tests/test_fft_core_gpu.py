"""The FFT kernels' transform core on the GPU (tests/fft_core_cases.py)."""
import pytest

import fft_core_cases as fc

pytestmark = pytest.mark.gpu


def test_fft_complex_helpers(hip):
    fc.case_fft_complex_helpers(hip, fused=True)


@pytest.mark.parametrize("name", list(fc.CASES))
def test_fft_core_bit_identity(hip, monkeypatch, name):
    fc.case_bit_identity(hip, monkeypatch, name, "gpu")
