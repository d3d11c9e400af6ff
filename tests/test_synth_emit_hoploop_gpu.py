"""kSynthEmitTeams' hop loop at the edges of a tile, on the GPU (tests/synth_emit_hoploop_cases.py)."""
import pytest

import synth_emit_hoploop_cases as hc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(hc.CASES))
def test_synth_emit_hoploop(hip, monkeypatch, name):
    hc.case_hoploop(hip, monkeypatch, **hc.CASES[name])
