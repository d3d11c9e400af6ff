"""The whole-call stages against the parent commit's digests, on the CPU stand-in for the HIP runtime (tests/whole_call_cases.py)."""
import pytest

import whole_call_cases as wc


@pytest.mark.parametrize("name", list(wc.SCENARIOS))
def test_whole_call_emu(emu, name):
    wc.case_whole_call(emu, name, "emu")


@pytest.mark.parametrize("name", list(wc.SCENARIOS))
def test_steady_state_emu(emu, name):
    wc.case_steady_state(emu, name)
