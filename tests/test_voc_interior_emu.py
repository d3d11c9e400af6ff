"""The interior form of the line-aligned producers' block against SMST_VOC_INTERIOR=0, on the CPU stand-in for the HIP runtime (tests/voc_interior_cases.py)."""
import pytest

import voc_interior_cases as vc


@pytest.mark.parametrize("name", vc.EMU_CASES)
def test_voc_interior_emu(emu, monkeypatch, name):
    vc.case_voc_interior(emu, monkeypatch, name)
