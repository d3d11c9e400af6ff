"""kSynthEmitTeams' hop loop at the edges of a tile, on the CPU stand-in for the HIP runtime (tests/synth_emit_hoploop_cases.py)."""
import pytest

import synth_emit_hoploop_cases as hc


@pytest.mark.parametrize("name", hc.EMU_CASES)
def test_synth_emit_hoploop_emu(emu, monkeypatch, name):
    hc.case_hoploop(emu, monkeypatch, **hc.CASES[name])
