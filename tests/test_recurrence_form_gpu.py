"""Which form of the bin recurrence a tile takes, on the GPU (tests/recurrence_form_cases.py)."""
import pytest

import recurrence_form_cases as rf

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(rf.SCENARIOS))
def test_recurrence_form(hip, monkeypatch, name):
    rf.case_recurrence_form(hip, monkeypatch, name, "gpu")
