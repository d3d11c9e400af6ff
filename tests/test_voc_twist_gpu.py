"""Twisted tiles against SMST_VOC_TWIST=0, on the GPU (tests/voc_twist_cases.py)."""
import pytest

import voc_twist_cases as vc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(vc.CASES))
def test_voc_twist(hip, monkeypatch, name):
    vc.case_voc_twist(hip, monkeypatch, name)
