"""The bin recurrence against its float64 mirror, bin by bin, on the MI355X (tests/recurrence_residual_cases.py has the mirror, the partner
streams, the bounds and the excuses): every row -- every form recurrenceForm chooses among -- at the three time factors of Tier A, and
Tier B's re-analysed previous input (1.6x, 0.8x, 2.5x with drawn time factors) on the 256-band rows, presetCheaper and presetDefault."""
import pytest

import recurrence_residual_cases as rr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tf", rr.TIER_A)
@pytest.mark.parametrize("row", list(rr.ROWS))
def test_tier_a(hip, ref, monkeypatch, row, tf):
    rr.case_residual(hip, ref, monkeypatch, row, tf)


@pytest.mark.parametrize("tf", rr.TIER_B)
@pytest.mark.parametrize("row", [r for r in rr.ROWS if rr.ROWS[r]["tier_b"]])
def test_tier_b(hip, ref, monkeypatch, row, tf):
    """A net for gross errors by design: the previous input of these hops is re-analysed inside the call, the mirror's is a float64 DFT."""
    rr.case_residual(hip, ref, monkeypatch, row, tf)
