"""The feed stage against its float64 mirror on the MI355X (tests/feed_stage_cases.py has the mirror, the bounds and the excuses): every
form launchFeed chooses among, each side of the 16 | 24 bins-per-thread and the register | LDS boundaries, 1 to 9 channels, a
split-computation geometry."""
import pytest

import feed_stage_cases as fs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", list(fs.MODES))
@pytest.mark.parametrize("mix", list(fs.MIXES))
@pytest.mark.parametrize("M", sorted(fs.BANDS))
def test_forms_and_shapes(hip, monkeypatch, M, mix, mode):
    fs.case_feed_stage(hip, monkeypatch, M, mix, mode)


@pytest.mark.parametrize("channels", [1, 3, 8, 9])
@pytest.mark.parametrize("mix,mode", [("maps", "default"), ("estimated", "default"), ("given", "separate")])
def test_channel_counts(hip, monkeypatch, channels, mix, mode):
    fs.case_feed_stage(hip, monkeypatch, 256, mix, mode, channels=channels)


@pytest.mark.parametrize("mix,mode", [("maps", "default"), ("given", "default"), ("estimated", "separate")])
def test_split_computation(hip, monkeypatch, mix, mode):
    """The steps of a hop spread over the calls of an interval: checked once the hop is complete."""
    fs.case_feed_stage(hip, monkeypatch, 256, mix, mode, split=True)
