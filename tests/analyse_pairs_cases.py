"""kAnalyseTeamPairs (the analysis teams, two frames per pass) against the two forms it stands beside: shared by the CPU stand-in and the GPU test.

A case is ONE batch geometry run three times over the same two calls -- the pair form (the default), SMST_ANALYSE_PAIRS=0 (kAnalyseTeams, one
frame per pass) and SMST_FFT_TEAMS=0 (kAnalyseFast, one frame per workgroup) -- and asserts that each call's output, the carried sums and
window products after each call and the carried per-bin state at the end are byte-identical in all three, and by the launch counters that
each run went through the kernel it was meant for.  SMST_FFT_TEAMS=2 lets the small tiles of these batches take the team kernels.

The pair form takes two consecutive positions of one stream's job order per pass (the hop fastest, then window and channel), each with the
predicate of the single-frame teams: the frame is wanted (a new spectrum; for the window one interval earlier, a hop that re-analyses it)
and its window lies in the call's input.  What decides which passes occur is therefore the number of hops of the tile (odd: a pair
straddles two rows of the job order), which hops' windows lie in the call (the others reach into the carried history and are kAnalyseFast's),
and whether the hops re-analyse their previous window (not at stretch 1.0: whole rows are then unwanted).

Calls.  The first call fires `hops1` hops per stream, the first at sample 0, and ends half an interval into its last hop, so the second call's
first hop begins half an interval into that call.  At stretch f hop k's window ends k*I/f samples into the first call's input: at 1.5 and
block = 4 intervals the hops from 6 on lie in the call (their previous windows from hop 8 on), everything else is kAnalyseFast's -- both
kernels run.  The second call is ragged: another hop count and another length per stream, some streams without a hop.  Its input is
`in2` times its output: with a long input and few hops (`hops2` = 1, 2, 3) the hops' windows lie in the call, and the tile has that number of
hops."""
import numpy as np

from conftest import package, synth_input

SWITCHES = ("SMST_FFT_TEAMS", "SMST_ANALYSE_PAIRS")
COUNTERS = ("analyse_pairs", "analyse_teams", "analyse_fast", "analyse_generic")
FORMS = {
    # form: (environment, counters that grow, counters that do not)
    "pairs": ({"SMST_FFT_TEAMS": "2"}, ("analyse_pairs", "analyse_teams"), ("analyse_generic",)),
    "single": ({"SMST_FFT_TEAMS": "2", "SMST_ANALYSE_PAIRS": "0"}, ("analyse_teams",), ("analyse_pairs", "analyse_generic")),
    "per_frame": ({"SMST_FFT_TEAMS": "0"}, ("analyse_fast",), ("analyse_pairs", "analyse_teams", "analyse_generic")),
}

# hops2: the second call's hop counts, dealt to the streams in turn.  in2: its input length as a multiple of its output length.
# teams_in_call2: the second call has windows in the call (otherwise all of its frames are kAnalyseFast's and no team kernel is launched)
RAGGED = (0, 7, 9, 12, 8, 0, 10, 11, 13)
DEFAULTS = dict(preset="default", sample_rate=48000, channels=2, streams=7, stretch=1.5, hops1=9, hops2=RAGGED, in2=None, teams_in_call2=True)
CASES = {
    # every instantiation: EXACT R3 = 12, EXACT R3 = 10, the run-time geometry; stereo and mono
    "default_48k_stereo": dict(),
    "default_48k_mono": dict(channels=1, streams=9),
    "cheaper_48k_stereo": dict(preset="cheaper"),
    "cheaper_48k_mono": dict(preset="cheaper", channels=1, streams=9),
    "default_44k1_stereo": dict(sample_rate=44100),
    "default_44k1_mono": dict(sample_rate=44100, channels=1, streams=9),
    # no hop re-analyses its previous window: the rows of the window one interval earlier are unwanted as a whole
    "stretch_1": dict(stretch=1.0, streams=5),
    # tiles of 1, 2 and 3 hops whose windows lie in the call (9 hops: every first call)
    "tile_of_1": dict(hops2=(1, 1, 0, 1, 1), in2=12.0, streams=5),
    "tile_of_2": dict(hops2=(2, 1, 0, 2, 2), in2=9.0, streams=5),
    "tile_of_3": dict(preset="cheaper", hops2=(3, 2, 0, 3, 1, 3), in2=6.0, streams=6),
    # a first call in which one hop's window lies in the call and six reach into the history; a second call without a window in the call
    "short_first_call": dict(hops1=7, hops2=(2, 0, 3, 1, 2), streams=5, teams_in_call2=False),
    # the job order with gy = 2C = 6 rows per stream
    "three_channels": dict(channels=3, streams=5),
}
# the CPU stand-in runs a kernel lane by lane: the index logic of each instantiation's geometry, of whole unwanted rows, of the odd tiles, of three channels
EMU_CASES = ("default_48k_stereo", "cheaper_48k_mono", "default_44k1_stereo", "stretch_1", "tile_of_1", "tile_of_3", "short_first_call", "three_channels")


def plan(case, I):
    """-> [(n_in[streams], n_out[streams])] of the two calls"""
    S, f = case["streams"], case["stretch"]
    n_out1 = np.full(S, case["hops1"]*I - I//2, np.int64)  # hops at 0, I, ..; the last one half an interval before the end
    n_in1 = np.maximum((n_out1/f).astype(np.int64), 1)
    first = I - I//2                                       # where the second call's first hop begins
    n_out2, n_in2 = np.zeros(S, np.int64), np.zeros(S, np.int64)
    for s in range(S):
        h = case["hops2"][s % len(case["hops2"])]
        n_out2[s] = first + (h - 1)*I + 1 + 13*s if h else 30 + s  # (without a hop: carried samples only)
        n_in2[s] = max(int(n_out2[s]*case["in2"]) if case["in2"] else int(n_out2[s]/f), 1)
    return [(n_in1, n_out1), (n_in2, n_out2)]


def run_form(lib, env, case, form):
    """-> {what: bytes} of one run; env: pytest's monkeypatch"""
    pkg = package()
    switches, ran, idle = FORMS[form]
    for k in SWITCHES:
        env.delenv(k, raising=False)
    for k, val in switches.items():
        env.setenv(k, val)
    S, C, sr = case["streams"], case["channels"], case["sample_rate"]
    b = pkg.StretchBatch(S, C, preset=case["preset"], sample_rate=sr, lib=lib)
    calls = plan(case, b.intervalSamples())
    n_total = int(sum(n_in.max() for n_in, _ in calls))
    x = np.stack([synth_input(s, C, n_total, sr) for s in range(S)])
    got, grew = {}, []
    pos = np.zeros(S, np.int64)
    for call, (n_in, n_out) in enumerate(calls):
        before = {k: pkg.launch_count(k, lib) for k in COUNTERS}
        xin = np.zeros((S, C, int(n_in.max())), np.float32)
        for s in range(S):
            xin[s, :, :n_in[s]] = x[s, :, pos[s]:pos[s] + n_in[s]]
        pos += n_in
        y = np.array(b.process(xin, n_out.astype(np.int32), in_samples=n_in.astype(np.int32)), copy=True)
        if call == 0:
            assert float(np.abs(y).max()) > 0.05
        got["output %d" % call] = np.concatenate([y[s, :, :n_out[s]].ravel() for s in range(S)]).tobytes()
        carry = [b.debug_carry(s) for s in range(S)]
        got["carried sums %d" % call] = np.concatenate([c[0].ravel() for c in carry]).tobytes()
        got["carried products %d" % call] = np.concatenate([c[1].ravel() for c in carry]).tobytes()
        grew.append({k: pkg.launch_count(k, lib) - before[k] for k in COUNTERS})
    for which, what in enumerate(("input", "previous input", "output", "energy")):
        got["state: " + what] = np.concatenate([np.asarray(b.debug_state(s, which)).ravel() for s in range(S)]).tobytes()
    b.close()
    for k in SWITCHES:
        env.delenv(k, raising=False)
    # the intended kernel ran: in the first call always, in the second where the case puts windows into the call
    for call, g in enumerate(grew):
        expect = ran if (call == 0 or case["teams_in_call2"] or form == "per_frame") else ("analyse_fast",)
        assert all(g[k] > 0 for k in expect) and all(g[k] == 0 for k in idle), (form, call, g)
    if form != "per_frame":
        # the first hops of the first call reach into the history: the team forms leave them to kAnalyseFast, so both counters grew
        assert grew[0]["analyse_fast"] > 0, (form, grew[0])
    return got


def case_analyse_pairs(lib, monkeypatch, name):
    case = dict(DEFAULTS, **CASES[name])
    assert 5 <= case["streams"] <= 9
    runs = {form: run_form(lib, monkeypatch, case, form) for form in FORMS}
    for other in ("single", "per_frame"):
        assert sorted(runs["pairs"]) == sorted(runs[other])
        differing = [k for k in sorted(runs["pairs"]) if runs["pairs"][k] != runs[other][k]]
        assert not differing, (name, other, differing)
