"""The bin recurrence against its float64 mirror, bin by bin, on the CPU stand-in (tests/recurrence_residual_cases.py has the mirror, the
partner streams, the bounds and the excuses): the mirror against the checker, the partner premise on the checker, the yardsticks, caps and
branch shares with no product code involved, and every form of the recurrence at the rows with 1024 bands at the most (presetDefault once)."""
import pytest

import recurrence_residual_cases as rr


def test_mirror_against_the_checker(ref):
    rr.check_mirror(ref)


def test_partner_premise_on_the_checker(ref):
    rr.case_partner_premise(ref)


def test_every_row_names_a_scenario_and_a_counter():
    for name, row in rr.ROWS.items():
        assert row["shows"] and all(k in rr.rf.COUNTERS for k in row["shows"]), name
        assert not row["sc"]["half_state"], name
        rr.layout(name)
    assert sorted(rr.YARDSTICK) == rr.SHAPES


@pytest.mark.parametrize("M,channels,tier", rr.SHAPES)
def test_inputs_stay_within_caps(ref, M, channels, tier):
    """The mirror alone on the checker's operands, through the cases' own calls: the excused bins and (Tier B) the bins with a large allowance
    stay under their caps, the quiet stream takes makeOutput's fallback and its normal branch on at least 5 % of its bins each, the silent
    channel is there.  And the float32 formula in the reference's order -- what the recorded yardsticks were measured with -- passes the
    check that the product has to pass (its figure is printed: the yardstick up to the last bits of this machine's FFT and sine)."""
    if getattr(ref, "is_port", False):
        return  # (the port restates none of the private members the operands are read from)
    fig = rr.measure_yardstick(ref, M, channels, tier)
    rr.assert_caps(fig, "%d bands, %d ch, tier %s (mirror alone)" % (M, channels, tier), tier)
    assert channels == 1 or fig["silent_bins"] > 0
    assert fig["yardstick"] <= rr.bound(M, channels, tier), (M, channels, tier, fig["yardstick"], rr.YARDSTICK[(M, channels, tier)])


EMU_ROWS = rr.EMU_ROWS + ("default_48k",)


@pytest.mark.parametrize("tf", rr.TIER_A)
@pytest.mark.parametrize("row", [r for r in EMU_ROWS if r != "default_48k"])
def test_tier_a(emu, ref, monkeypatch, row, tf):
    rr.case_residual(emu, ref, monkeypatch, row, tf)


def test_tier_a_default_48k(emu, ref, monkeypatch):
    rr.case_residual(emu, ref, monkeypatch, "default_48k", "I/(I-1)")


@pytest.mark.parametrize("tf", rr.TIER_B)
@pytest.mark.parametrize("row", [r for r in rr.EMU_ROWS if rr.ROWS[r]["tier_b"]])
def test_tier_b(emu, ref, monkeypatch, row, tf):
    """A net for gross errors by design: the previous input of these hops is re-analysed inside the call, the mirror's is a float64 DFT."""
    rr.case_residual(emu, ref, monkeypatch, row, tf)
