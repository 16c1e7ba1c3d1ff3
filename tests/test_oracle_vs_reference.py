"""CPU: the oracle of the HEADLINE path against the reference itself.

linux/synth.c:27-208 (note tables, allocator, sum_tick_saw/square, synth_run),
stm32f103/pmeas.h:64-108 (pmeas_update) and stm32f103/mod_pdm.c:159-175 (OSC_HARD_SYNC, pwm_update)
compile verbatim with system headers alone
(oracle/Makefile `ref` streams those line ranges into gcc; nothing is stubbed).  Their
outputs are committed as tests/golden/synth_c_reference.npz / pmeas_reference.npz / pwmosc_reference.npz
(generator: tests/golden/make_golden.py) and the oracle must reproduce them bit for bit;
the oracle is also compared on random operation sequences: live when oracle/_ref is present
(it travels with the built tree), else against the reference's recorded answers to the committed
seeds (tests/golden/live_reference.npz, tests/refcases.py).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle
import refcases
import replay

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "synth_c_reference.npz"))


def test_note_to_inc_and_midi_tab_equal_reference_outputs(orc, gold):
    assert [orc.orc_note_to_inc(n) for n in range(128)] == gold["note_to_inc"].tolist()
    assert [orc.orc_midi_tab(n) for n in range(128)] == gold["midi_tab"].tolist()
    # note & 127 (linux/synth.c:119)
    assert orc.orc_note_to_inc(128 + 69) == int(gold["note_to_inc"][69])


def test_survey_known_answers_agree_with_the_compiled_reference(gold):
    """The numbers typed in from SURVEY Appendix A.2 are consistent with the real outputs."""
    with open(os.path.join(GOLD, "survey_known_answers.json")) as f:
        kat = json.load(f)
    inc = gold["note_to_inc"]
    assert inc[116:128].tolist() == kat["note_tab"]
    assert all(int(inc[int(n)]) == v for n, v in kat["note_to_inc"].items())
    assert int(inc.astype(np.uint64).sum()) == kat["note_to_inc_sum_0_127"]


@pytest.mark.parametrize("name", replay.SCRIPTS)
def test_oracle_reproduces_reference_scripts(orc, gold, name):
    vec, n2v, inc, st = replay.on_oracle(orc, gold[name + "_script"])
    assert np.array_equal(vec, gold[name + "_vec_bits"])
    assert np.array_equal(n2v, gold[name + "_note2voice"])
    assert np.array_equal(inc, gold[name + "_inc"])
    assert np.array_equal(st, gold[name + "_state"])


def test_fixture_covers_the_quirks(gold):
    """The committed vectors really contain the cases they are meant to pin."""
    s = gold["wrapping_mix_script"]
    assert (s[:, 0] == replay.OP_POKE).sum() >= 3 * 64
    q = gold["b64_quirks_script"]
    assert (q[:, 0] == replay.OP_ON).sum() > 64                   # more notes than voices: steal
    assert gold["b4096_random_vec_bits"].size == 3 * 4096
    assert gold["b1_ticks_script"][:, 1].max() >= 128            # note % 128
    sq = gold["square_vec_bits"].view(np.float32)
    assert set(np.unique(sq[:664]).tolist()) <= {0.0, 0.5}       # sum_tick_square: 0 or 0.5


def test_oracle_pmeas_reproduces_reference_traces(orc):
    g = np.load(os.path.join(GOLD, "pmeas_reference.npz"))
    fields = [str(x) for x in g["fields"]]
    names = sorted(k[:-6] for k in g.files if k.endswith("_trace"))
    assert len(names) >= 6
    published = 0
    for name in names:
        p = oracle.Pmeas(log_max=int(g[name + "_log_max"]))
        for cc, want in zip(g[name + "_cc"], g[name + "_trace"]):
            orc.orc_pmeas_update(C.byref(p), int(cc))
            got = dict(log_max=p.log_max, write=p.write, read=p.read, avg0=p.avg[0], num0=p.num_pub[0],
                       avg1=p.avg[1], num1=p.num_pub[1], num=p.num, accu=p.accu, last_cc=p.last_cc)
            assert [got[f] for f in fields] == want.tolist(), name
        published += p.write
    assert published > 20                                          # the publish branch (pmeas.h:85-91) ran


def pwmosc_cases(g):
    return sorted(k[:-5] for k in g.files if k.endswith("_duty"))


def test_oracle_pwm_update_reproduces_reference_outputs(orc):
    """Row a-8b: orc_pwm_update / orc_pwmosc_run == the reference's pwm_update + OSC_HARD_SYNC
    (mod_pdm.c:159-175 compiled verbatim), 70 000 ticks per case."""
    g = np.load(os.path.join(GOLD, "pwmosc_reference.npz"))
    assert int(g["default_speed"]) == 256 * 13 and int(g["default_phase"]) == 0       # mod_pdm.c:160-161
    assert int(g["control_div"]) == 256                                              # mod_pdm.c:164
    nt = int(g["nticks"])
    names = pwmosc_cases(g)
    assert len(names) >= 6 and nt >= 70000
    for name in names:
        phase = np.array([g[name + "_phase0"]], np.uint32)
        speed = np.array([g[name + "_speed"]], np.uint32)
        sync = np.zeros((nt, 1), np.uint32)
        sync[g[name + "_sync_ticks"], 0] = 1
        # tick by tick through orc_pwm_update for the phases ...
        ph = int(phase[0])
        p1 = np.zeros(1, np.uint32)
        seen = []
        duty1 = np.zeros(nt, np.uint8)
        for t in range(nt):
            if sync[t, 0]:
                ph = 0
            p1[0] = ph
            duty1[t] = orc.orc_pwm_update(p1, int(speed[0])) & 0xFF
            ph = int(p1[0])
            if t % 16 == 15:
                seen.append(ph)
        assert np.array_equal(duty1, g[name + "_duty"]), name
        assert seen == g[name + "_phase_every16"].tolist(), name
        assert ph == int(g[name + "_phase_end"]), name
        # ... and the bank loop the GPU tests use as their oracle
        duty = np.zeros((nt, 1), np.uint8)
        orc.orc_pwmosc_run(phase, speed, 1, sync.ctypes.data, nt, duty.ctypes.data)
        assert np.array_equal(duty[:, 0], g[name + "_duty"]), name
        assert int(phase[0]) == int(g[name + "_phase_end"]), name
        assert int(g[name + "_wraps"]) >= 19, name          # the 24-bit mask (mod_pdm.c:162) is crossed many times


# ---- random inputs: live when the compiled reference is present, else its recorded answers ----------
# (tests/refcases.py; the answers to the committed seeds are tests/golden/live_reference.npz)
def _want(ref, on_reference, cases_of, seed, recorded):
    """-> (inputs, the reference's answers to them): live from oracle/_ref when it is there (and then the recorded
    answers must be what it gives), else the committed seed's inputs and the recorded answers."""
    live = ref is not None
    cases = cases_of(refcases.rng(seed, live))
    if not live:
        return cases, recorded
    want = on_reference(ref, cases)
    if not refcases.soaking():
        for w, r in zip(want if isinstance(want, tuple) else want.values(),
                        recorded if isinstance(recorded, tuple) else recorded.values()):
            assert np.array_equal(w, r), "tests/golden/live_reference.npz is stale (tests/golden/make_golden.py)"
    return cases, want


def test_live_random_pwm_updates_against_compiled_mod_pdm_c(orc):
    g = refcases.recorded()
    cases, (want_duty, want_phase) = _want(oracle.load_ref_pwmosc(), refcases.pwm_on_reference, refcases.pwm_cases,
                                           refcases.PWM_SEED, (g["pwm_duty"], g["pwm_phase_end"]))
    duty, phase = refcases.pwm_on_oracle(orc, cases)
    for case in range(len(cases)):
        assert np.array_equal(duty[case], want_duty[case]), case
        assert phase[case] == want_phase[case], case


def test_live_random_ops_against_compiled_synth_c(orc):
    g = refcases.recorded()
    rec = {k: g["synth_" + k] for k in ("run_bits", "square_bits", "alloc", "snapshots")}
    ops, want = _want(oracle.load_ref_synth(), refcases.synth_on_reference, refcases.synth_ops,
                      refcases.SYNTH_SEED, rec)
    got = refcases.synth_on_oracle(orc, ops)
    for k in rec:
        assert got[k].shape == want[k].shape, k
        diff = got[k] != want[k]
        bad = np.flatnonzero(diff.any(axis=1) if diff.ndim > 1 else diff)
        assert len(bad) == 0, (k, int(bad[0]))


def test_live_random_timestamps_against_compiled_pmeas_h(orc):
    g = refcases.recorded()
    cases, (want_steps, want_end) = _want(oracle.load_ref_pmeas(), refcases.pmeas_on_reference, refcases.pmeas_cases,
                                          refcases.PMEAS_SEED, (g["pmeas_steps"], g["pmeas_end"]))
    steps, end = refcases.pmeas_on_oracle(orc, cases)
    for k, (lm, _) in enumerate(cases):
        bad = np.flatnonzero((steps[k] != want_steps[k]).any(axis=1))
        assert len(bad) == 0, (lm, int(bad[0]))
        assert np.array_equal(end[k], want_end[k]), lm
        assert steps[k, -1, 0] > 0                      # write
