"""CPU: the oracle against every golden vector / known-answer this path has.

Pinning status per function is in oracle/synth_oracle.h.  Nothing here touches
the GPU or the product library's compute path.
"""
import json
import os

import numpy as np
import pytest

import oracle
import refcases

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(GOLD, "survey_known_answers.json")) as f:
        return json.load(f)


def test_note_tab_and_inc(orc, kat):
    tab = np.zeros(12, np.uint32)
    orc.orc_note_tab(tab)
    assert tab.tolist() == kat["note_tab"]
    for note, inc in kat["note_to_inc"].items():
        assert orc.orc_note_to_inc(int(note)) == inc
    assert sum(orc.orc_note_to_inc(n) for n in range(128)) == kat["note_to_inc_sum_0_127"]
    # notes 116..127 are the table itself (linux/synth.c:93-97)
    assert [orc.orc_note_to_inc(n) for n in range(116, 128)] == kat["note_tab"]


def test_midi_tab_layout(orc):
    # linux/synth.c:106-115: note 127 -> (octave 0, semitone 11); note 0 -> (10, 4)
    assert orc.orc_midi_tab(127) == (0 << 4) | 11
    assert orc.orc_midi_tab(0) == (10 << 4) | 4
    assert orc.orc_midi_tab(8) == (9 << 4) | 0
    for n in range(12, 128):           # an octave down halves the increment
        assert orc.orc_note_to_inc(n - 12) == orc.orc_note_to_inc(n) >> 1


def test_synth_run_chord_known_answer(orc, kat):
    n2v = np.zeros(128, np.int32)
    inc = np.zeros(64, np.uint32)
    st = np.zeros(64, np.uint32)
    for n in (69, 72, 76):
        orc.orc_note_on(n2v, inc, 64, n)
    _, vec = oracle.synth_run(orc, inc, st, 8)
    assert ["%08x" % x for x in vec.view(np.uint32)] == kat["chord_69_72_76_first8_float_bits"]
    assert inc[0] == kat["chord_voice0_after8"]["inc"]
    assert st[0] == kat["chord_voice0_after8"]["state"]


def test_allocator_quirks(orc):
    """linux/synth.c:145-165: steal voice 0 when full, stray note-off kills voice 0,
    note_on does not reset phase."""
    n2v = np.zeros(128, np.int32)
    inc = np.zeros(64, np.uint32)
    st = np.arange(64, dtype=np.uint32) * 1000
    for n in range(64):
        orc.orc_note_on(n2v, inc, 64, n)
    assert np.all(inc != 0) and n2v[63] == 63
    orc.orc_note_on(n2v, inc, 64, 100)             # full: steals voice 0
    assert n2v[100] == 0 and inc[0] == orc.orc_note_to_inc(100)
    assert st[5] == 5000                           # phase untouched by note_on
    orc.orc_note_off(n2v, inc, 64, 120)            # never played -> voice 0 silenced
    assert inc[0] == 0
    orc.orc_note_off(n2v, inc, 64, 7)
    assert inc[7] == 0 and n2v[7] == 0
    orc.orc_note_on(n2v, inc, 64, 30)              # first free is voice 0 again
    assert n2v[30] == 0


def test_inactive_voices_do_not_advance(orc):
    inc = np.array([0, 5, 0, 7], np.uint32)
    st = np.array([11, 22, 33, 44], np.uint32)
    bus, vec = oracle.synth_run(orc, inc, st, 3)
    assert st.tolist() == [11, 37, 33, 65]
    assert bus.tolist() == [(22 >> 4) + (44 >> 4), (27 >> 4) + (51 >> 4), (32 >> 4) + (58 >> 4)]


def test_big_bank_tick_without_the_branch_is_the_same_tick(orc):
    """orc_synth_run steps banks above 2^20 voices with a branch-free statement of sum_tick_saw (linux/synth.c:169-179;
    a half-active bank makes `if (inc)` a coin toss per voice): same bus, same phases as the reference's loop taken
    tick by tick with orc_sum_tick_saw, on a half-active bank with arbitrary increments."""
    import numpy as np
    import oracle
    n = (1 << 20) + 77
    rng = np.random.default_rng(0x0B1A5)
    inc = rng.integers(1, 2**32, n, dtype=np.uint64).astype(np.uint32)
    inc[rng.random(n) < 0.5] = 0
    st0 = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    a = st0.copy()
    bus, _ = oracle.synth_run(orc, inc, a, 9)
    b = st0.copy()
    want = np.array([orc.orc_sum_tick_saw(inc, b, n) for _ in range(9)], np.int32)
    assert np.array_equal(bus, want) and np.array_equal(a, b)
    assert np.array_equal(a[inc == 0], st0[inc == 0])            # off voices do not advance


def test_bus_to_float_is_exact_power_of_two_scale(orc):
    for s in (0, 1, -1, 2**31 - 1, -2**31, 123456789, -987654321, 0x01000001):
        want = np.float32(np.float32(s) * np.float32(2.0 ** -32))
        assert orc.orc_bus_to_float(s) == want


def test_wrapping_mix(orc):
    """>= 16 full-scale voices overflow the reference's int sum; it wraps (UB made defined
    with -fwrapv), and so must every reduction order."""
    inc = np.ones(64, np.uint32)
    st = np.full(64, 0x7FFFFFF0, np.uint32)
    bus, _ = oracle.synth_run(orc, inc, st.copy(), 1)
    want = (64 * (0x7FFFFFF0 >> 4)) & 0xFFFFFFFF
    assert int(bus[0]) & 0xFFFFFFFF == want


def test_synth_run_derived_regression(orc):
    g = np.load(os.path.join(GOLD, "synth_run_derived.npz"))
    n2v = np.zeros(128, np.int32)
    inc = np.zeros(64, np.uint32)
    st = np.zeros(64, np.uint32)
    vecs = []
    for op, a in g["script"]:
        if op == 0:
            orc.orc_note_on(n2v, inc, 64, int(a))
        elif op == 1:
            orc.orc_note_off(n2v, inc, 64, int(a))
        else:
            vecs.append(oracle.synth_run(orc, inc, st, int(a))[1])
    assert np.array_equal(np.concatenate(vecs).view(np.uint32), g["vec"].view(np.uint32))
    assert np.array_equal(inc, g["inc"]) and np.array_equal(st, g["state"])


# ---- mod_pdm.c ---------------------------------------------------------------
def test_pdm_comment_kat(orc, kat):
    """The only known-answer the reference holds: 3-bit accumulator, X=3
    (stm32f103/mod_pdm.c:43-47).  Scaled to the 32-bit accumulator: X<<29."""
    k = kat["mod_pdm_comment_kat_3bit"]
    sp = np.array([k["X"] << 29], np.uint32)
    accu = np.array([k["A"][0] << 29], np.uint32)
    # C[i] is the carry that PRODUCED A[i]; the row starts after a wrap to 0.
    for i in range(1, len(k["A"])):
        bits = np.zeros(1, np.uint32)
        orc.orc_pdm_tick(sp, accu, 1, 0, bits)
        assert accu[0] >> 29 == k["A"][i]
        assert bits[0] == k["C"][i]
    # C[0] = 1: stepping into A=0 from A=5 carries
    accu[:] = 5 << 29
    bits = np.zeros(1, np.uint32)
    orc.orc_pdm_tick(sp, accu, 1, 0, bits)
    assert accu[0] == 0 and bits[0] == k["C"][0]


def test_pdm_comment_kat_x5_accumulator_row(orc, kat):
    """The complementary row (mod_pdm.c:49-53, X = 5 = 8 - 3): the accumulator sequence is data; the carry row
    printed under it is not what add-with-carry produces and the oracle must NOT reproduce it."""
    k = kat["mod_pdm_comment_kat_3bit_x5"]
    sp = np.array([k["X"] << 29], np.uint32)
    accu = np.array([k["A"][0] << 29], np.uint32)
    carries = []
    for i in range(1, len(k["A"])):
        bits = np.zeros(1, np.uint32)
        orc.orc_pdm_tick(sp, accu, 1, 0, bits)
        assert accu[0] >> 29 == k["A"][i] and accu[0] & 0x1FFFFFFF == 0
        carries.append(int(bits[0]))
    assert carries == [0, 1, 0, 1, 1, 0, 1, 1]                       # 5 pulses in 8 ticks = X / N
    assert carries != k["C_as_printed_not_reproducible"][1:]
    # "the same waveform, but in reverse" (mod_pdm.c:49-50): X=5's pulses are X=3's gaps read backwards
    x3 = kat["mod_pdm_comment_kat_3bit"]["C"][1:]
    assert [1 - c for c in carries] == x3[::-1]


def test_pdm_comment_period_table(orc, kat):
    """mod_pdm.c:30-38: X a power of two -> one pulse every N / X ticks (N = 2^32 here)."""
    for lg in kat["mod_pdm_comment_period_table"]["testable_log2_X_32bit"]:
        period = 1 << (32 - lg)
        nt = 3 * period if period > 2 else 16
        sp = np.array([1 << lg], np.uint32)
        accu = np.zeros(1, np.uint32)
        bits = oracle.pdm_run(orc, sp, accu, nt)[:, 0]
        assert np.flatnonzero(bits).tolist() == list(range(period - 1, nt, period)), lg
    # X = 1: period N = 2^32 -- the one pulse lies where the accumulator wraps
    sp = np.array([1], np.uint32)
    accu = np.array([0xFFFFFFFD], np.uint32)
    assert oracle.pdm_run(orc, sp, accu, 8)[:, 0].tolist() == [0, 0, 1, 0, 0, 0, 0, 0]


def test_pdm_two_channel_bsrr_derived(orc, kat):
    k = kat["mod_pdm_two_channel_derived"]
    sp = np.array(k["setpoint"], np.uint32)
    accu = np.zeros(2, np.uint32)
    got = [orc.orc_pdm_bsrr(sp, accu, 2, 0) for _ in range(k["ticks"])]
    assert got == k["bsrr"]
    assert accu.tolist() == k["accu_end"]


def test_pdm_tick_matches_bsrr_packing(orc):
    """bank layout (channel c -> bit c) vs the reference's rrx/BSRR packing (pin 4+c)."""
    from synth_tools_amd import synthetic
    for nb in (1, 2, 5, 12):
        sp, _ = synthetic.pdm_bank(nb, 77 + nb)
        a1 = np.zeros(nb, np.uint32)
        a2 = np.zeros(nb, np.uint32)
        for t in range(200):
            d = (t * 2654435761) & 0x0FFFFFFF
            bits = np.zeros(1, np.uint32)
            orc.orc_pdm_tick(sp, a1, nb, d, bits)
            bsrr = orc.orc_pdm_bsrr(sp, a2, nb, d)
            mask = ((1 << nb) - 1) << 4
            set_ = (int(bits[0]) << 4) & mask
            assert bsrr == set_ | (((~set_) & mask) << 16)
        assert np.array_equal(a1, a2)


def test_pdm_density(orc):
    """Pulse density = setpoint / 2^32 (what a first-order PDM is for)."""
    sp = np.array([0x40000000, 0x80000000, 0xC0000000, 2000000000], np.uint32)
    accu = np.zeros(4, np.uint32)
    bits = oracle.pdm_run(orc, sp, accu, 4096)
    for c in range(4):
        ones = int(((bits[:, 0] >> c) & 1).sum())
        assert abs(ones - int(sp[c]) * 4096 / 2**32) <= 1


def test_pwm_update(orc):
    ph = np.array([0], np.uint32)
    duties = [orc.orc_pwm_update(ph, 256 * 13) for _ in range(5000)]
    assert duties[0] == 0 and max(duties) <= 0xFF and ph[0] <= 0xFFFFFF
    # hand-evaluated first steps of phase = (phase + speed + (phase >> 9)) & 0xFFFFFF
    p, want = 0, []
    for _ in range(5000):
        want.append(p >> 16)
        p = (p + 3328 + (p >> 9)) & 0xFFFFFF
    assert duties == want


# ---- pdm.h: the REAL reference header (oracle/_ref) and its committed outputs --
def _run_orc_pdm(orc, order, x, sh, dither, steps):
    f = getattr(orc, "orc_pdm%d_update" % order)
    s = np.zeros(order, np.uint32)
    q = np.zeros(steps, np.uint32)
    for t in range(steps):
        q[t] = f(s, int(x), int(sh)) if order == 1 else f(s, int(x), int(sh), int(dither[t]))
    return q, s


def test_pdm_h_against_committed_reference_outputs(orc):
    g = np.load(os.path.join(GOLD, "pdm_h_reference.npz"))
    steps = int(g["steps"])
    dith = [np.zeros(steps, np.uint32), g["dither1"]]
    for order in (1, 2, 3, 4):
        for i, x in enumerate(g["inputs"]):
            for j, sh in enumerate(g["shifts"]):
                for k in (0, 1):
                    q, s = _run_orc_pdm(orc, order, x, sh, dith[k], steps)
                    assert np.array_equal(q, g["q%d" % order][i, j, k])
                    assert np.array_equal(s, g["s%d" % order][i, j, k])


def test_pdm_h_survey_known_answers(orc, kat):
    k = kat["pdm_h_in2000000000_sh24_16calls"]
    z = np.zeros(16, np.uint32)
    q1, s1 = _run_orc_pdm(orc, 1, 2000000000, 24, z, 16)
    q2, s2 = _run_orc_pdm(orc, 2, 2000000000, 24, z, 16)
    q3, _ = _run_orc_pdm(orc, 3, 2000000000, 24, z, 16)
    assert (int(q1.sum()), int(q2.sum()), int(q3.sum())) == (k["sum_pdm1"], k["sum_pdm2"], k["sum_pdm3"])
    assert s1[0] == k["pdm1_s1"] and s2.tolist() == k["pdm2_s"]
    assert q1[0] == 0 and q2[0] == 0            # one-sample output delay (pdm.h:14-17)


def test_pdm_h_live_against_real_header(orc):
    """Random inputs against the reference's own pdm.h compiled into oracle/_ref when it is present (it travels
    with the built tree as a .so), else against its recorded answers to the committed seed
    (tests/golden/live_reference.npz, tests/refcases.py)."""
    ref = oracle.load_ref_pdm()
    g = refcases.recorded()
    cases = refcases.pdm_cases(refcases.rng(refcases.PDM_SEED, ref is not None))
    want_q, want_s = g["pdm_q"], g["pdm_state_end"]
    if ref is not None:
        live_q, live_s = refcases.pdm_on_reference(ref, cases)
        if not refcases.soaking():
            assert np.array_equal(live_q, want_q) and np.array_equal(live_s, want_s), \
                "tests/golden/live_reference.npz is stale (tests/golden/make_golden.py)"
        want_q, want_s = live_q, live_s
    q, s = refcases.pdm_on_oracle(orc, cases)
    for k, (order, _, sh, _, _) in enumerate(cases):
        assert np.array_equal(q[k], want_q[k]), (order, sh, k)
        assert np.array_equal(s[k], want_s[k]), (order, sh, k)


# ---- mod_pdm_pwm.c / mod_controlrate.c / pmeas.h / cproc.h: restatement checks --
def _pwm_bank(n, setpoint, div_log=12, order=2):
    import ctypes as C
    arrs = {k: np.zeros(n, np.uint32) for k in ("setpoint", "pos0", "pos1", "s1", "s2", "s3", "s4")}
    arrs["vel0"] = np.zeros(n, np.int32)
    arrs["vel1"] = np.zeros(n, np.int32)
    arrs["setpoint"][:] = setpoint
    b = oracle.PwmBank(n=n, order=order, div_count=0, div_log=div_log, out_shift=24,
                       s=(C.c_void_p * 4)(*[arrs["s%d" % k].ctypes.data for k in (1, 2, 3, 4)]),
                       **{k: arrs[k].ctypes.data for k in ("setpoint", "pos0", "vel0", "pos1", "vel1")})
    return b, arrs


def test_pwm_bank_glide_reaches_setpoint(orc):
    """mod_controlrate.c:28-40: the line segments converge on the setpoint and the
    8-bit duty's mean tracks position/2^24 (mod_pdm_pwm.c:108-116)."""
    import ctypes as C
    b, a = _pwm_bank(3, [2000000000, 0x40000000, 0xC0000000], div_log=6)
    nt = 64 * 40
    duty = np.zeros((nt, 3), np.uint8)
    orc.orc_pwm_bank_run(C.byref(b), None, nt, duty.ctypes.data)
    for c in range(3):
        assert abs(int(a["pos1"][c]) - int(a["setpoint"][c])) < 64 * 64
        mean = duty[-256:, c].astype(np.float64).mean()
        assert abs(mean - int(a["setpoint"][c]) / 2**24) < 1.0
    assert b.div_count == 0


def test_pmeas(orc):
    """pmeas.h:64-100: periods of 1000 cycles, window 1<<14 -> 16 periods averaged,
    avg has (32-log_max) fractional bits."""
    import ctypes as C
    p = oracle.Pmeas(log_max=14)
    cc = 0
    for _ in range(40):
        cc += 1000
        orc.orc_osc_event(C.byref(p), cc & 0xFFFFFFFF)
    assert p.write == 2
    w = p.write & 1
    assert p.num_pub[w] == 16 and p.avg[w] == ((16000 << 18) // 16)
    assert p.sub == 0                       # 40 events: sub-osc toggled back (mod_osc.c:65)


def test_cproc_atoms(orc):
    out = np.zeros(1, np.uint32)
    last = np.zeros(1, np.uint32)
    acc = np.zeros(1, np.uint32)
    seq = [0, 0, 5, 5, 5, 2, 2, 0]
    edges = []
    for x in seq:                            # the edge -> acc chain of linux/test_cproc.c:13-15
        orc.orc_edge_update(out, last, x)
        orc.orc_acc_update(acc, int(out[0]))
        edges.append(int(out[0]))
    assert edges == [0, 0, 1, 0, 0, 1, 0, 1] and acc[0] == 3


# ---- build-defined poly voice and the clock generator: definition sanity --------------
def test_poly_definition_sanity(orc):
    """The build-defined voice (no reference counterpart): envelope walks A -> D -> S, releases
    to idle; the 1-pole filter follows the saw; an off voice (inc 0) is silent and frozen."""
    import ctypes as C
    n = 2
    a = dict(inc=np.array([39370533, 0], np.uint32), phase=np.array([0, 123], np.uint32),
             y=np.zeros(n, np.float32), a=np.full(n, 0.25, np.float32),
             level=np.zeros(n, np.uint32), stage=np.zeros(n, np.uint32), gate=np.ones(n, np.uint32),
             ar=np.full(n, 0x08000000, np.uint32), dr=np.full(n, 0x04000000, np.uint32),
             sl=np.full(n, 0x80000000, np.uint32), rr=np.full(n, 0x02000000, np.uint32),
             pan=np.full(n, 256 | (128 << 16), np.uint32))
    b = oracle.PolyBank(n=n, **{k: v.ctypes.data for k, v in a.items()})
    stages = []
    for blk in range(12):
        if blk == 6:
            a["gate"][:] = 0
        bus = np.zeros(2 * 16, np.int32)
        orc.orc_poly_run(C.byref(b), bus, 16)
        stages.append(int(a["stage"][0]))
        if blk == 3:
            assert np.any(bus != 0) and np.array_equal(bus[0::2] // 2, bus[1::2] // 2) is not None
    assert stages[0] == 1 and 3 in stages and stages[-1] == 0          # A ... S ... idle
    assert a["level"][0] == 0
    assert a["phase"][1] == 123 and a["stage"][1] == 0 and a["y"][1] == 0   # off voice untouched
    assert a["phase"][0] == (12 * 16 * 39370533) & 0xFFFFFFFF


def test_clock_definition(orc):
    """clock.c:106-120 at the reference's operating point: 120 bpm @ 48 kHz -> half period 500
    frames; first toggle when phase reaches 500; ticks only on the rising polarity."""
    hp = np.array([orc.orc_bpm_to_hperiod(48000, 120)], np.uint32)
    ph, po = np.zeros(1, np.int32), np.ones(1, np.uint32)
    pb, tb = np.zeros(2100, np.uint32), np.zeros(2100, np.uint32)
    orc.orc_clock_run(hp, ph, po, 1, 2100, pb, tb)
    assert hp[0] == 500
    assert pb[:500].all() and not pb[500:1000].any() and pb[1000:1500].all()
    assert np.flatnonzero(tb).tolist() == [1000, 2000]
