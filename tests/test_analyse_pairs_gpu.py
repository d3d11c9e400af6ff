"""kAnalyseTeamPairs against the single-frame teams and the per-frame kernel, on the GPU (tests/analyse_pairs_cases.py)."""
import pytest

import analyse_pairs_cases as ac

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(ac.CASES))
def test_analyse_pairs(hip, monkeypatch, name):
    ac.case_analyse_pairs(hip, monkeypatch, name)
