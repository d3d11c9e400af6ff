"""The _pcm calls' per-call table against the parent commit's digests, on the GPU, on host and on device memory (tests/pcm_tables_cases.py)."""
import pytest

import pcm_tables_cases as pt

pytestmark = pytest.mark.gpu


def test_pcm_tables_host(hip):
    pt.case_pcm_tables(hip, "gpu", "host")


def test_pcm_tables_device(hip):
    pt.case_pcm_tables(hip, "gpu", "device", **pt.device_memory())
