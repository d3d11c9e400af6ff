"""The whole-call stages against the parent commit's digests, on the GPU and on device memory (tests/whole_call_cases.py)."""
import pytest

import whole_call_cases as wc

pytestmark = pytest.mark.gpu


def _device_memory():
    import torch
    return dict(to_memory=lambda a: torch.from_numpy(a).cuda(), to_host=lambda t: t.cpu().numpy())


@pytest.mark.parametrize("name", list(wc.SCENARIOS))
def test_whole_call(hip, name):
    wc.case_whole_call(hip, name, "gpu", **_device_memory())


@pytest.mark.parametrize("name", list(wc.SCENARIOS))
def test_steady_state(hip, name):
    wc.case_steady_state(hip, name, **_device_memory())
