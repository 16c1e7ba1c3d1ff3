"""GPU: the poly bank's controllers -- sustain pedal (CC 64), all sound off (CC 120), reset all controllers (CC 121),
all notes off (CC 123) and pitch bend (0xE0) -- against a sequential numpy statement of the rule
(include/synth_mi355x.h).

The model extends tests/test_poly_notes_gpu.py's.  After every batch the device's inc/gate/stage, note map and
sustained bits must equal the model exactly, and every block's bus must be bit-exact against oracle orc_poly_run run
on the model's arrays; a bent block runs the oracle with inc_eff written into its inc array, then restores it."""
import os
import subprocess

import ctypes as C
import numpy as np
import pytest

import oracle
from test_poly_notes_gpu import IDLE, R, S, Model, Rig, off, on, patch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE = 8192


def cc(num, val):
    return [0xB0, num, val]


def bend(b):
    return [0xE0, b & 0x7F, b >> 7]


PEDAL_DOWN, PEDAL_UP, SOUND_OFF, RESET, NOTES_OFF = cc(64, 127), cc(64, 0), cc(120, 0), cc(121, 0), cc(123, 0)


class CtlModel(Model):
    """The note rule plus the controllers, one event at a time."""

    def __init__(self, orc, keep, smx):
        super().__init__(orc, keep)
        self.smx = smx
        self.pedal = False
        self.sus = np.zeros(128, np.uint8)
        self.bend, self.range = CENTRE, 2

    def clear_maps(self):
        super().clear_maps()
        self.sus[:] = 0

    def mul(self):
        return self.smx.poly_bend_mul(self.bend, self.range)

    def release(self, m):                     # a real note_off, whatever the pedal
        self.sus[m] = 0
        super().note_off(m)

    def note_off(self, note):
        m = note % 128
        if self.pedal:
            if self.n2v[m] >= 0:
                self.sus[m] = 1
            return
        self.release(m)

    def note_on(self, note):
        m = note % 128
        if self.n2v[m] >= 0:
            self.release(m)
        v = self.pick()
        if self.vnote[v] >= 0:
            self.sus[self.vnote[v]] = 0       # a steal clears the stolen note's bit
        return super().note_on(m)           # n2v[m] is none now: no second release

    def pedal_up(self):
        self.pedal = False
        for m in np.nonzero(self.sus)[0]:
            self.release(int(m))

    def sound_off(self):
        for f in ("gate", "stage", "level"):
            self.k[f][:] = 0
        self.clear_maps()

    def midi(self, msg):
        if len(msg) != 3:
            return
        st, d1, d2 = int(msg[0]), int(msg[1]), int(msg[2])
        if st in (0x90, 0x80):
            return super().midi(msg)
        if st == 0xE0:
            self.bend = (d1 & 0x7F) | (d2 & 0x7F) << 7
        elif st == 0xB0:
            if d1 == 64:
                down = d2 >= 64
                if down and not self.pedal:
                    self.pedal = True
                elif not down and self.pedal:
                    self.pedal_up()
            elif d1 == 120:
                self.sound_off()
            elif d1 == 121:
                if self.pedal:
                    self.pedal_up()
                self.bend = CENTRE
            elif d1 == 123:
                for m in np.nonzero(self.n2v >= 0)[0]:
                    self.note_off(int(m))


class CRig(Rig):
    def __init__(self, smx, orc, arrs, controllers=True):
        super().__init__(smx, orc, arrs)
        self.m = CtlModel(orc, self.keep, smx)
        if controllers:
            self.bank.set_controllers(1)
        else:                                 # the model honours only notes
            self.m.midi = lambda msg: Model.midi(self.m, msg)

    def set_range(self, semitones):
        self.bank.set_bend_range(semitones)
        self.m.range = semitones

    def check(self, what=""):
        super().check(what)
        assert np.array_equal(self.bank.read_sustain(), self.m.sus), what

    def block(self, nf=64):
        mul = self.m.mul()
        if mul == 65536:
            return super().block(nf)
        inc = self.keep["inc"].copy()
        self.keep["inc"][:] = ((inc.astype(np.uint64) * np.uint64(mul)) >> np.uint64(16)).astype(np.uint32)
        try:
            return super().block(nf)
        finally:
            self.keep["inc"][:] = inc

    def check_state(self):
        """phase, y and level read back exactly; inc is still the notes' increments."""
        got = self.bank.read(("inc", "phase", "y", "level"))
        for f in ("inc", "phase", "level"):
            assert np.array_equal(got[f], self.keep[f]), f
        assert np.array_equal(got["y"].view(np.uint32), self.keep["y"].view(np.uint32))


def quick(n, inc_table, **kw):
    return patch(n, inc_table, ar=0x10000000, dr=0x01000000, sl=0x80000000, rr=0x02000000, **kw)


# ---- sustain pedal --------------------------------------------------------------------------------------------------
def test_note_off_under_pedal_then_pedal_up(smx, orc, inc_table):
    r = CRig(smx, orc, quick(64, inc_table))
    r.events([on(60), on(62), on(64), PEDAL_DOWN, off(60), off(62), cc(64, 100)])   # a repeated "down": no-op
    r.check()
    assert list(r.bank.read_sustain()[[60, 62, 64]]) == [1, 1, 0]
    assert list(r.bank.read(("gate",))["gate"][:3]) == [1, 1, 1]
    assert list(r.bank.read_notes()[[60, 62, 64]]) == [0, 1, 2]
    r.block()
    r.events([off(70), cc(64, 63)])                      # unmapped note_off: nothing sustained; 63 is "up"
    r.check()
    assert (r.bank.read_sustain() == 0).all()
    assert list(r.bank.read(("gate",))["gate"][:3]) == [0, 0, 1]
    assert r.bank.read_notes()[64] == 2 and (r.bank.read_notes()[[60, 62]] == -1).all()
    r.block()
    r.events([PEDAL_UP, off(64)])                        # repeated "up": no-op; the pedal is up, so 64 releases
    r.check()
    r.block()
    r.close()


def test_restrike_sustained_note(smx, orc, inc_table):
    r = CRig(smx, orc, quick(16, inc_table))
    r.events([PEDAL_DOWN, on(60), off(60)])
    r.block()
    r.events([on(60)])                                   # the sustained voice releases, a fresh voice takes 60
    r.check()
    assert r.bank.read_notes()[60] == 1 and r.bank.read_sustain()[60] == 0
    assert list(r.bank.read(("gate",))["gate"][:2]) == [0, 1]
    r.events([off(60), PEDAL_UP])
    r.check()
    r.block()
    r.close()


def test_steal_sustained_voice(smx, orc, inc_table):
    n = 4
    r = CRig(smx, orc, quick(n, inc_table))
    r.events([PEDAL_DOWN] + [on(60 + i) for i in range(n)] + [off(60), off(61)])
    r.block()
    r.keep["level"][:] = [1, 9, 9, 9]
    r.keep["level"] *= 0x10000000
    r.bank.load(level=r.keep["level"])
    r.events([on(90)])                                   # every voice held (sustained ones too): quietest is 0
    r.check()
    assert r.bank.read_notes()[90] == 0 and r.bank.read_sustain()[60] == 0 and r.bank.read_sustain()[61] == 1
    r.events([PEDAL_UP])
    r.check()
    assert list(r.bank.read(("gate",))["gate"]) == [1, 0, 1, 1]
    r.block()
    r.close()


@pytest.mark.parametrize("pedal", [False, True])
def test_all_notes_off(smx, orc, inc_table, pedal):
    r = CRig(smx, orc, quick(256, inc_table))
    r.events([on(m) for m in range(0, 128, 3)])
    r.block()
    r.events(([PEDAL_DOWN] if pedal else []) + [off(3), cc(123, 77)])
    r.check()
    if pedal:
        assert (r.bank.read_sustain()[r.m.n2v >= 0] == 1).all() and (r.m.n2v >= 0).sum() == 43
        r.events([PEDAL_UP])
        r.check()
    assert (r.bank.read_notes() == -1).all() and (r.bank.read(("gate",))["gate"] == 0).all()
    r.block()
    r.close()


def test_sound_off_mid_batch(smx, orc, inc_table):
    n = 1536
    r = CRig(smx, orc, quick(n, inc_table))
    r.events([PEDAL_DOWN] + [on(m) for m in range(40, 80)] + [off(45)])
    r.block()
    r.block()
    r.events([on(30), off(50), cc(120, 5), on(31), on(32), off(31)])    # before / after in the same batch
    r.check()
    got = r.bank.read(("level", "stage", "gate"))
    assert (got["level"][2:] == 0).all() and got["gate"][0] == 1 and got["gate"][1] == 1    # 31 is sustained
    assert r.bank.read_sustain()[31] == 1 and list(r.bank.read_notes()[[31, 32]]) == [0, 1]
    r.check_state()
    r.block()
    r.events([PEDAL_UP])                                 # the pedal state survived CC 120
    r.check()
    r.block()
    r.close()


def test_reset_all_controllers(smx, orc, inc_table):
    r = CRig(smx, orc, quick(64, inc_table))
    r.set_range(12)
    r.events([on(60), on(67), bend(12000), PEDAL_DOWN, off(60)])
    r.block()
    r.check_state()
    r.events([RESET])
    r.check()
    assert r.m.mul() == 65536 and (r.bank.read_sustain() == 0).all() and r.bank.read_notes()[60] == -1
    r.block()
    r.check_state()
    r.events([RESET])                                    # pedal up already: nothing to release
    r.check()
    r.close()


# ---- pitch bend ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rng_", [0, 2, 12, 24])
def test_bend_values(smx, orc, inc_table, rng_):
    r = CRig(smx, orc, quick(1024, inc_table))
    r.set_range(rng_)
    r.events([on(m) for m in (0, 1, 33, 60, 64, 100, 127)])
    notes_inc = r.keep["inc"].copy()
    for b in (0, 8191, 8192, 8193, 16383):
        r.events([bend(b)])
        want_mul = 65536 if (b == CENTRE or rng_ == 0) else None
        if want_mul:
            assert smx.poly_bend_mul(b, rng_) == want_mul
        r.block()
        r.block(17)
        r.check()
        r.check_state()
        assert np.array_equal(r.bank.read(("inc",))["inc"], notes_inc)
    r.close()


def test_range_change_while_bent(smx, orc, inc_table):
    r = CRig(smx, orc, quick(512, inc_table))
    r.events([on(m) for m in range(50, 70)] + [bend(3000)])
    r.block()
    r.set_range(24)
    r.block(5)
    r.check_state()
    r.set_range(0)                                       # range 0: unbent whatever b
    r.block()
    r.set_range(7)
    r.bank.load(phase=r.keep["phase"])                   # bend and range persist across loads
    r.block(64)
    r.check_state()
    r.close()


def test_bend_wraps_near_2_32(smx, orc, inc_table):
    n = 1024
    arrs = quick(n, inc_table)
    arrs["inc"][:8] = [0xFFFFFFFF, 0xFFFFFFF0, 0xF0000000, 0xC0000001, 1, 2, 3, 0x80000000]
    arrs["gate"][:8] = 1
    r = CRig(smx, orc, arrs)
    r.set_range(24)
    r.events([bend(16383)])
    mul = smx.poly_bend_mul(16383, 24)
    assert (0xFFFFFFFF * mul) >> 16 >= 1 << 32                     # the product wraps
    r.block()
    r.check_state()
    r.events([bend(0)])                                  # inc 1..3 bent down to 0: frozen
    assert (3 * smx.poly_bend_mul(0, 24)) >> 16 == 0
    r.block()
    r.check_state()
    r.close()


def test_set_bend_range_rejects(smx):
    b = smx.PolyBank(1024)
    for bad in (-1, 25):
        with pytest.raises(smx.SmxError):
            b.set_bend_range(bad)
    b.set_bend_range(0)
    b.set_bend_range(24)
    b.close()


# ---- release-all at full width ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,gx", [(512, 1), (1536, 3), (65537, 65)])
def test_release_all_128_in_mixed_batch(smx, orc, inc_table, n, gx):
    r = CRig(smx, orc, quick(n, inc_table))
    r.events([PEDAL_DOWN] + [on(m) for m in range(128)])
    r.block()
    r.events([off(m) for m in range(128)])
    r.check()
    assert (r.bank.read_sustain() == 1).all()
    rng = np.random.default_rng(n)
    notes = [int(x) for x in rng.integers(0, 128, 63)]
    batch = [(on if i % 3 else off)(m) for i, m in enumerate(notes)]
    r.events(batch[:40] + [PEDAL_UP] + batch[40:])       # 63 note events + one release of 128 sustained voices
    r.check()
    r.block()
    r.events([PEDAL_DOWN] + [off(m) for m in range(128)] + [on(5), PEDAL_UP, on(6)])
    r.check()
    r.block()
    r.close()


# ---- fuzz ---------------------------------------------------------------------------------------------------------
def _ctl_events(rng, count):
    out = []
    for _ in range(count):
        u = rng.random()
        nt = int(rng.integers(36, 100))
        if u < 0.5:
            out.append(on(nt))
        elif u < 0.75:
            out.append(off(nt))
        elif u < 0.85:
            out.append(cc(64, int(rng.integers(0, 128))))
        elif u < 0.93:
            out.append(bend(int(rng.integers(0, 1 << 14))))
        elif u < 0.96:
            out.append(cc(123, 0))
        elif u < 0.98:
            out.append(cc(121, 0))
        elif u < 0.99:
            out.append(cc(120, 0))
        else:
            out.append([int(rng.choice([0xB1, 0xE1, 0xB0])), int(rng.choice([7, 64, 120])), 1])
    return out


@pytest.mark.parametrize("n,blocks", [(1 << 10, 12), (1 << 18, 6), (1 << 22, 3)])
@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_controllers(smx, orc, inc_table, n, blocks, seed):
    s = 0xC0DE + 97 * seed + n
    rng = np.random.default_rng(s)
    arrs = quick(n, inc_table)
    live = rng.random(n) < (0.02 if n > 4096 else 0.5)
    arrs["inc"][live] = inc_table[rng.integers(0, 128, int(live.sum()))]
    arrs["gate"][live] = 1
    r = CRig(smx, orc, arrs)
    r.set_range(int(rng.choice([2, 12, 24])))
    for blk in range(blocks):
        count = int(rng.choice([1, 5, 64, 65, 150]))
        if n > 1 << 12:
            count = min(count, 65)
        r.events(_ctl_events(rng, count))
        r.check("block %d" % blk)
        r.block((1, 17, 64)[blk % 3])
    r.check_state()
    r.close()


# ---- dispatch ----------------------------------------------------------------------------------------------------
def test_controllers_off_ignores_them(smx, orc, inc_table):
    r = CRig(smx, orc, quick(64, inc_table), controllers=False)
    r.events([on(60), on(61), PEDAL_DOWN, bend(0), off(60), cc(123, 0), cc(121, 0)])
    r.check()
    assert r.bank.read_notes()[61] == 1 and (r.bank.read_sustain() == 0).all()
    r.block()
    r.events([cc(120, 0)])
    r.check()
    r.block()
    r.check_state()
    r.close()


def test_other_channels_ignored(smx, orc, inc_table):
    r = CRig(smx, orc, quick(64, inc_table))
    r.events([on(60), on(61), [0xB1, 64, 127], [0xE1, 0, 0], off(60), [0xB1, 120, 0], [0xB1, 123, 0],
              [0xBF, 121, 0], [0xB0, 7, 100], [0xB0, 65, 127]])
    r.check()
    assert r.bank.read_notes()[61] == 1 and r.bank.read_notes()[60] == -1
    r.block()
    r.bank.midi_event(np.array([0xB0, 64], np.uint8))   # not 3 bytes
    r.bank.midi_event(np.array([0xE0, 0, 0, 0], np.uint8))
    r.events([off(61)])
    r.check()
    r.block()
    r.close()


def test_single_calls_equal_one_batch(smx, orc, inc_table):
    n = 300
    arrs = quick(n, inc_table)
    rng = np.random.default_rng(21)
    msgs = _ctl_events(rng, 400)
    a, b = smx.PolyBank(n), smx.PolyBank(n)
    for x in (a, b):
        x.load(**arrs)
        x.set_controllers(1)
        x.set_bend_range(5)
    a.midi_events(np.array(msgs, np.uint8))
    for mm in msgs:
        b.midi_event(np.array(mm, np.uint8))
    ra, rb = a.read(), b.read()
    for k in ra:
        assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32)), k
    assert np.array_equal(a.read_notes(), b.read_notes())
    assert np.array_equal(a.read_sustain(), b.read_sustain())
    assert np.array_equal(a.run(64)[0], b.run(64)[0])
    a.close()
    b.close()


def test_load_clears_sustain(smx, orc, inc_table):
    r = CRig(smx, orc, quick(64, inc_table))
    r.events([PEDAL_DOWN, on(60), on(61), off(60), off(61)])
    r.bank.load(level=r.keep["level"])                   # neither inc nor gate: bits kept
    r.check()
    r.bank.load(gate=r.keep["gate"])
    r.m.clear_maps()
    r.check()
    r.events([PEDAL_UP])                                 # nothing sustained any more: nothing released
    r.check()
    assert (r.bank.read(("gate",))["gate"][:2] == 1).all()
    r.close()


# ---- host program -------------------------------------------------------------------------------------------------
def test_host_poly_controllers_fake_jack(smx, orc, inc_table, tmp_path):
    """SYNTH_POLY_CONTROLLERS=1 in --fake-jack mode: pedal, bend and CC 120 across blocks, bit-exact against the
    model + orc_poly_run."""
    elf = os.path.join(ROOT, "host", "synth.dynamic.host.elf")
    n, nblocks, nframes, brange = 512, 14, 64, 7
    patch_s = (0.125, 0x02000000, 0x00400000, 0x60000000, 0x01000000, 100 | (156 << 16))
    rng = np.random.default_rng(9)
    rec = []
    for blk in range(nblocks):
        for _ in range(int(rng.integers(0, 10))):
            nt = int(rng.integers(30, 90))
            st = 0x90 if rng.random() < 0.6 else 0x80
            rec.append((blk, 3, st, nt, 90 if st == 0x90 else 0))
        if blk == 2:
            rec.append((blk, 3, 0xB0, 64, 127))
        if blk == 4:
            rec.append((blk, 3, 0xE0, 0x11, 0x60))
        if blk == 6:
            rec.append((blk, 3, 0xB0, 64, 0))
        if blk == 8:
            rec.append((blk, 3, 0xB0, 120, 0))
        if blk == 10:
            rec.append((blk, 3, 0xE0, 0x00, 0x20))
    ev = np.zeros(len(rec), np.dtype([("block", "<u4"), ("size", "u1"), ("b", "u1", 3)]))
    for i, (b, sz, *m) in enumerate(rec):
        ev[i] = (b, sz, m)
    evf, outf = tmp_path / "ev.bin", tmp_path / "out.f32"
    ev.tofile(evf)
    env = dict(os.environ, SYNTH_POLY=str(n), SYNTH_POLY_PATCH="%r,%d,%d,%d,%d,%d" % patch_s,
               SYNTH_POLY_CONTROLLERS="1", SYNTH_POLY_BEND_RANGE=str(brange))
    env.pop("SYNTH_RANKS", None)
    p = subprocess.run([elf, "--fake-jack", str(nblocks), str(nframes), str(evf), str(outf)], env=env,
                       stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert p.returncode == 1, p.stderr.decode()
    assert b"fake-jack rendered" in p.stderr
    got = np.fromfile(outf, np.float32).reshape(nblocks, 2, nframes)

    z = np.zeros(n, np.uint32)
    a, ar, dr, sl, rr, pan = patch_s
    arrs = dict(inc=z.copy(), phase=z.copy(), y=np.zeros(n, np.float32), a=np.full(n, a, np.float32),
                level=z.copy(), stage=z.copy(), gate=z.copy(), ar=np.full(n, ar, np.uint32),
                dr=np.full(n, dr, np.uint32), sl=np.full(n, sl, np.uint32), rr=np.full(n, rr, np.uint32),
                pan=np.full(n, pan, np.uint32))
    ob = oracle.PolyBank(n=n, **{k: v.ctypes.data for k, v in arrs.items()})
    m = CtlModel(orc, arrs, smx)
    m.range = brange
    bent = 0
    for blk in range(nblocks):
        for (b, sz, *msg) in rec:
            if b == blk and sz == 3:
                m.midi(msg)
        mul = m.mul()
        inc = arrs["inc"].copy()
        if mul != 65536:
            bent += 1
            arrs["inc"][:] = ((inc.astype(np.uint64) * np.uint64(mul)) >> np.uint64(16)).astype(np.uint32)
        want = np.zeros(2 * nframes, np.int32)
        orc.orc_poly_run(C.byref(ob), want, nframes)
        arrs["inc"][:] = inc
        wf = np.array([orc.orc_bus_to_float(int(s)) for s in want], np.float32).reshape(nframes, 2)
        assert np.array_equal(got[blk, 0].view(np.uint32), wf[:, 0].view(np.uint32)), blk
        assert np.array_equal(got[blk, 1].view(np.uint32), wf[:, 1].view(np.uint32)), blk
    assert bent >= 8 and np.abs(got).max() > 0
