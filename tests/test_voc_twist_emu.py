"""Twisted tiles against SMST_VOC_TWIST=0, on the CPU stand-in for the HIP runtime (tests/voc_twist_cases.py)."""
import pytest

import voc_twist_cases as vc


@pytest.mark.parametrize("name", vc.EMU_CASES)
def test_voc_twist_emu(emu, monkeypatch, name):
    vc.case_voc_twist(emu, monkeypatch, name)
