"""kAnalyseTeamPairs against the single-frame teams and the per-frame kernel, on the CPU stand-in for the HIP runtime (tests/analyse_pairs_cases.py)."""
import pytest

import analyse_pairs_cases as ac


@pytest.mark.parametrize("name", ac.EMU_CASES)
def test_analyse_pairs_emu(emu, monkeypatch, name):
    ac.case_analyse_pairs(emu, monkeypatch, name)
