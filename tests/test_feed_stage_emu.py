"""The feed stage against its float64 mirror on the CPU stand-in (tests/feed_stage_cases.py has the mirror, the bounds and the excuses):
the mirror against the checker, the yardsticks and the excused shares of the inputs with no product code involved, and every form of the
stage at the smallest shape that reaches it."""
import pytest

import feed_stage_cases as fs

SMALL = (160, 256)


def test_mirror_against_the_checker(ref):
    fs.check_mirror(ref)


@pytest.mark.parametrize("M,channels", sorted(fs.YARDSTICK))
def test_inputs_stay_within_caps(M, channels):
    """The float64 mirror alone, on numpy spectra of the cases' signals: the excused shares stay under their caps at every shape.  And the
    float32 mirror in the reference's order -- what the recorded yardsticks were measured with -- passes the check that the product has to
    pass (its figures are printed: they are the yardsticks up to the last bits of this machine's FFT and sine)."""
    worst, shares = fs.measure_yardsticks(M, channels)
    for mix, sh in shares.items():
        fs.assert_caps(sh, "%d bands, %d ch, %s (mirror alone)" % (M, channels, mix))
    print({k: float("%.2e" % v) for k, v in worst.items()})
    for k in fs.QUANTITIES:
        assert worst[k] <= fs.bound(M, k, channels), (M, channels, k, worst[k], fs.YARDSTICK[(M, channels)][k])


@pytest.mark.parametrize("mode", list(fs.MODES))
@pytest.mark.parametrize("mix", list(fs.MIXES))
@pytest.mark.parametrize("M", SMALL)
def test_small_shapes(emu, monkeypatch, M, mix, mode):
    fs.case_feed_stage(emu, monkeypatch, M, mix, mode)


@pytest.mark.parametrize("mix,mode", [("maps", "default"), ("given", "default"), ("estimated", "default"), ("estimated", "separate"), ("given", "serial")])
@pytest.mark.parametrize("M", [m for m in fs.BANDS if m not in SMALL])
def test_register_and_lds_forms(emu, monkeypatch, M, mix, mode):
    """16 | 24 bins per thread and the LDS form with its bisection, each side of both boundaries."""
    fs.case_feed_stage(emu, monkeypatch, M, mix, mode)


@pytest.mark.parametrize("channels", [1, 3, 8, 9])
@pytest.mark.parametrize("mix,mode", [("maps", "default"), ("estimated", "default"), ("given", "separate")])
def test_channel_counts(emu, monkeypatch, channels, mix, mode):
    fs.case_feed_stage(emu, monkeypatch, 256, mix, mode, channels=channels)


@pytest.mark.parametrize("mix,mode", [("maps", "default"), ("given", "default"), ("estimated", "separate")])
def test_split_computation(emu, monkeypatch, mix, mode):
    """The steps of a hop spread over the calls of an interval: checked once the hop is complete."""
    fs.case_feed_stage(emu, monkeypatch, 256, mix, mode, split=True)
