"""Which form of the bin recurrence a tile takes, on the CPU stand-in for the HIP runtime (tests/recurrence_form_cases.py)."""
import pytest

import recurrence_form_cases as rf


def test_golden_files_agree_on_the_counters():
    rf.case_golden_files_agree_on_the_counters()


def test_every_recurrence_kernel_runs_at_its_channel_limits():
    rf.case_channel_limits_are_covered(rf.EMU_SCENARIOS)


@pytest.mark.parametrize("name", rf.EMU_SCENARIOS)
def test_recurrence_form_emu(emu, monkeypatch, name):
    rf.case_recurrence_form(emu, monkeypatch, name, "emu")
