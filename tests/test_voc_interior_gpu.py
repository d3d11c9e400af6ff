"""The interior form of the line-aligned producers' block against SMST_VOC_INTERIOR=0, on the GPU (tests/voc_interior_cases.py)."""
import pytest

import voc_interior_cases as vc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(vc.CASES))
def test_voc_interior(hip, monkeypatch, name):
    vc.case_voc_interior(hip, monkeypatch, name)
