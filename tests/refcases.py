"""The randomised oracle-vs-reference cases: their seeded inputs, and the answers of the compiled reference
(oracle/_ref) or of the oracle to them.  The reference's answers for the committed seeds are recorded in
tests/golden/live_reference.npz (generator: tests/golden/make_golden.py), so the tests hold where oracle/_ref
cannot be built; where it is present they are also computed live.  Test helper only."""
import ctypes as C
import os

import numpy as np

import oracle

GOLD_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live_reference.npz")

PWM_SEED, SYNTH_SEED, PMEAS_SEED, PDM_SEED = 159175, 20261004, 77, 1234
PMEAS_LOG_MAX = (8, 12, 20, 26, 30)


def rng(seed, live):
    """The committed inputs come from PCG64(seed) (what np.random.default_rng(seed) gives); a live comparison draws
    through np.random.default_rng so that SMX_SOAK_SEED (tests/conftest.py) can give it other data."""
    return np.random.default_rng(seed) if live else np.random.Generator(np.random.PCG64(seed))


def recorded():
    return np.load(GOLD_FILE)


def soaking():
    return bool(os.environ.get("SMX_SOAK_SEED"))


# ---- pwm_update + OSC_HARD_SYNC (mod_pdm.c:159-175) ------------------------------------------
def pwm_cases(r, ncases=40, nt=5000):
    """-> [(phase0, speed, sync uint8[nt])]."""
    out = []
    for _ in range(ncases):
        phase0 = int(r.integers(0, 1 << 24))
        speed = int(r.integers(0, 1 << int(r.integers(1, 33))))
        sync = (r.random(nt) < r.choice([0.0, 0.001, 0.05])).astype(np.uint8)
        out.append((phase0, speed, sync))
    return out


def pwm_on_reference(ref, cases):
    """-> (duty uint8[cases, nt], phase after the last tick uint32[cases])."""
    duty = np.zeros((len(cases), len(cases[0][2])), np.uint8)
    phase = np.zeros(len(cases), np.uint32)
    for k, (phase0, speed, sync) in enumerate(cases):
        ref.ref_pwm_set(phase0, speed)
        ref.ref_pwmosc_run(len(sync), sync.ctypes.data, duty[k].ctypes.data, None)
        phase[k] = ref.ref_pwm_get_phase()
    return duty, phase


def pwm_on_oracle(orc, cases):
    duty = np.zeros((len(cases), len(cases[0][2])), np.uint8)
    phase = np.zeros(len(cases), np.uint32)
    for k, (phase0, speed, sync) in enumerate(cases):
        nt = len(sync)
        ph = np.array([phase0], np.uint32)
        got = np.zeros((nt, 1), np.uint8)
        sync_words = np.ascontiguousarray(sync.astype(np.uint32).reshape(nt, 1))     # kept alive across the call
        orc.orc_pwmosc_run(ph, np.array([speed], np.uint32), 1, sync_words.ctypes.data, nt, got.ctypes.data)
        duty[k] = got[:, 0]
        phase[k] = ph[0]
    return duty, phase


# ---- linux/synth.c:27-208 on a random operation sequence ------------------------------------
OP_ON, OP_OFF, OP_POKE, OP_SQUARE, OP_ALLOC, OP_RUN = range(6)


def synth_ops(r, n=3000):
    """-> [(op, arg)]: note-on/off of notes 0..1023, all 64 phases poked, sum_tick_square, voice_alloc, runs."""
    ops = []
    for _ in range(n):
        x = r.random()
        if x < 0.35:
            ops.append((OP_ON, int(r.integers(0, 1024))))
        elif x < 0.6:
            ops.append((OP_OFF, int(r.integers(0, 1024))))
        elif x < 0.65:
            ops.append((OP_POKE, np.array([int(r.integers(0, 2**32)) for _ in range(64)], np.uint32)))
        elif x < 0.7:
            ops.append((OP_SQUARE, None))
        elif x < 0.72:
            ops.append((OP_ALLOC, None))
        else:
            ops.append((OP_RUN, int(r.choice([1, 2, 7, 64, 300]))))
    return ops


class _Record:
    """What the sequence answers: float bits of every run and square tick, every voice_alloc, and
    note2voice | inc | state after every 100th operation and at the end."""

    def __init__(self):
        self.run, self.square, self.alloc, self.snap = [], [], [], []

    def snapshot(self, n2v, inc, st):
        self.snap.append(np.concatenate([np.asarray(n2v, np.int32).view(np.uint32), inc, st]))

    def arrays(self):
        f32 = lambda v: np.array(v, np.float32).view(np.uint32)         # noqa: E731
        return {"run_bits": np.concatenate(self.run).view(np.uint32) if self.run else np.zeros(0, np.uint32),
                "square_bits": f32(self.square), "alloc": np.array(self.alloc, np.int32),
                "snapshots": np.array(self.snap, np.uint32)}


def synth_on_reference(ref, ops):
    rec = _Record()
    x = oracle.RefSynth()
    ref.synth_init(C.byref(x))
    with oracle.quiet_stderr():
        for i, (op, a) in enumerate(ops):
            if op == OP_ON:
                ref.synth_note_on(C.byref(x), a)
            elif op == OP_OFF:
                ref.synth_note_off(C.byref(x), a)
            elif op == OP_POKE:
                for v in range(64):
                    x.voice[v].note_state = int(a[v])
            elif op == OP_SQUARE:
                rec.square.append(ref.sum_tick_square(C.byref(x)))
            elif op == OP_ALLOC:
                rec.alloc.append(ref.voice_alloc(C.byref(x)))
            else:
                v = np.zeros(a, np.float32)
                ref.synth_run(C.byref(x), v, a)
                rec.run.append(v)
            if i % 100 == 0:
                rec.snapshot(*x.arrays())
    rec.snapshot(*x.arrays())
    return rec.arrays()


def synth_on_oracle(orc, ops):
    rec = _Record()
    n2v = np.zeros(128, np.int32)
    inc = np.zeros(64, np.uint32)
    st = np.zeros(64, np.uint32)
    for i, (op, a) in enumerate(ops):
        if op == OP_ON:
            orc.orc_note_on(n2v, inc, 64, a)
        elif op == OP_OFF:
            orc.orc_note_off(n2v, inc, 64, a)
        elif op == OP_POKE:
            st[:] = a
        elif op == OP_SQUARE:
            rec.square.append(orc.orc_sum_tick_square(inc, st, 64))
        elif op == OP_ALLOC:
            rec.alloc.append(orc.orc_voice_alloc(inc, 64))
        else:
            rec.run.append(oracle.synth_run(orc, inc, st, a)[1])
        if i % 100 == 0:
            rec.snapshot(n2v, inc, st)
    rec.snapshot(n2v, inc, st)
    return rec.arrays()


# ---- pmeas_update (pmeas.h:64-108) on random timestamps ---------------------------------------
def pmeas_cases(r, n=4000):
    """-> [(log_max, cycle counter uint32[n])]: increments 1 .. 2^(1..log_max+1)."""
    out = []
    for lm in PMEAS_LOG_MAX:
        cc, c = np.zeros(n, np.uint32), 0
        for i in range(n):
            c = (c + int(r.integers(1, 1 << int(r.integers(1, lm + 2))))) & 0xFFFFFFFF
            cc[i] = c
        out.append((lm, cc))
    return out


PMEAS_STEP = ("write", "num", "accu", "last_cc")
PMEAS_END = ("avg0", "avg1", "num0", "num1")


def pmeas_on_reference(ref, cases):
    """-> (write, num, accu, last_cc after every call uint32[cases, n, 4], avg0, avg1, num0, num1 at the end
    uint32[cases, 4])."""
    steps = np.zeros((len(cases), len(cases[0][1]), 4), np.uint32)
    end = np.zeros((len(cases), 4), np.uint32)
    for k, (lm, cc) in enumerate(cases):
        p = oracle.RefPmeas(ref, lm)
        for i, c in enumerate(cc):
            p.update(c)
            steps[k, i] = [p.get(f) for f in PMEAS_STEP]
        end[k] = [p.get(f) for f in PMEAS_END]
    return steps, end


def pmeas_on_oracle(orc, cases):
    steps = np.zeros((len(cases), len(cases[0][1]), 4), np.uint32)
    end = np.zeros((len(cases), 4), np.uint32)
    for k, (lm, cc) in enumerate(cases):
        p = oracle.Pmeas(log_max=lm)
        for i, c in enumerate(cc):
            orc.orc_pmeas_update(C.byref(p), int(c))
            steps[k, i] = [p.write, p.num, p.accu, p.last_cc]
        end[k] = [p.avg[0], p.avg[1], p.num_pub[0], p.num_pub[1]]
    return steps, end


# ---- pdm1..4_update (pdm.h) on random inputs ---------------------------------------------------
def pdm_cases(r, per_order=20, steps=300):
    """-> [(order, initial state uint32[order], shift, x uint32[steps], dither uint32[steps])]; the dither is 0
    at every third step."""
    out = []
    for order in (1, 2, 3, 4):
        for _ in range(per_order):
            s0 = r.integers(0, 2**32, order, dtype=np.uint64).astype(np.uint32)
            sh = int(r.integers(1, 32))
            x = np.zeros(steps, np.uint32)
            d = np.zeros(steps, np.uint32)
            for t in range(steps):
                x[t] = int(r.integers(0, 2**32))
                d[t] = int(r.integers(0, 2**32)) if t % 3 else 0
            out.append((order, s0, sh, x, d))
    return out


def _pdm_run(lib, prefix, cases):
    """-> (outputs uint32[cases, steps], final states uint32[cases, 4], zero-padded beyond the order)."""
    q = np.zeros((len(cases), len(cases[0][3])), np.uint32)
    fin = np.zeros((len(cases), 4), np.uint32)
    for k, (order, s0, sh, x, d) in enumerate(cases):
        f = getattr(lib, "%s_pdm%d_update" % (prefix, order))
        s = s0.copy()
        for t in range(len(x)):
            q[k, t] = f(s, int(x[t]), sh) if order == 1 else f(s, int(x[t]), sh, int(d[t]))
        fin[k, :order] = s
    return q, fin


def pdm_on_reference(ref, cases):
    return _pdm_run(ref, "ref", cases)


def pdm_on_oracle(orc, cases):
    return _pdm_run(orc, "orc", cases)
