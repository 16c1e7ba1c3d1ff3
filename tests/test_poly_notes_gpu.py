"""GPU: playing the poly voice bank -- smx_poly_note_on/_off, smx_poly_midi_event(s), smx_poly_read_notes -- against
a sequential numpy statement of the allocation rule (include/synth_mi355x.h).

After every batch the device's inc/gate/stage and note map must equal the model exactly, and every block's bus must
be bit-exact against oracle orc_poly_run run on the model's arrays."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from synth_tools_amd import synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDLE, A, D, S, R = 0, 1, 2, 3, 4


class Model:
    """§1 of the rule, one event at a time, on the arrays the oracle runs (keep)."""

    def __init__(self, orc, keep):
        self.orc, self.k = orc, keep
        self.n = len(keep["inc"])
        self.n2v = np.full(128, -1, np.int32)
        self.vnote = np.full(self.n, -1, np.int32)
        self.idx = np.arange(self.n)

    def clear_maps(self):
        self.n2v[:] = -1
        self.vnote[:] = -1

    def free(self):
        k = self.k
        return (k["inc"] == 0) | ((k["gate"] == 0) & (k["stage"] == IDLE))

    def pick(self):
        fr = self.free()
        if fr.any():
            return int(np.argmax(fr))
        g, lv = self.k["gate"], self.k["level"]
        cand = g == g.min()
        cand &= lv == lv[cand].min()
        return int(np.argmax(cand))

    def note_off(self, note):
        m = note % 128
        v = self.n2v[m]
        if v < 0:
            return
        self.k["gate"][v] = 0
        self.vnote[v] = -1
        self.n2v[m] = -1

    def note_on(self, note):
        m = note % 128
        if self.n2v[m] >= 0:
            self.note_off(m)
        v = self.pick()
        if self.vnote[v] >= 0:
            self.n2v[self.vnote[v]] = -1
        if self.k["gate"][v] == 1:
            self.k["stage"][v] = R
        self.k["inc"][v] = self.orc.orc_note_to_inc(m)
        self.k["gate"][v] = 1
        self.vnote[v] = m
        self.n2v[m] = v
        return v

    def midi(self, msg):
        if len(msg) != 3:
            return
        if msg[0] == 0x90:
            (self.note_on if msg[2] else self.note_off)(int(msg[1]))
        elif msg[0] == 0x80:
            self.note_off(int(msg[1]))


class Rig:
    def __init__(self, smx, orc, arrs):
        self.orc = orc
        self.keep = {k: np.ascontiguousarray(v).copy() for k, v in arrs.items()}
        self.ob = oracle.PolyBank(n=len(self.keep["inc"]), **{k: v.ctypes.data for k, v in self.keep.items()})
        self.bank = smx.PolyBank(len(self.keep["inc"]))
        self.bank.load(**self.keep)
        self.m = Model(orc, self.keep)

    def check(self, what=""):
        got = self.bank.read(("inc", "gate", "stage"))
        for f in ("inc", "gate", "stage"):
            bad = np.nonzero(got[f] != self.keep[f])[0]
            assert len(bad) == 0, "%s %s differs at voices %s" % (what, f, bad[:8])
        assert np.array_equal(self.bank.read_notes(), self.m.n2v), what

    def block(self, nf=64):
        bus, _ = self.bank.run(nf)
        want = np.zeros(2 * nf, np.int32)
        self.orc.orc_poly_run(C.byref(self.ob), want, nf)
        assert np.array_equal(bus.reshape(-1), want)
        return bus

    def events(self, msgs):
        msgs = np.asarray(msgs, np.uint8).reshape(-1, 3)
        self.bank.midi_events(msgs)
        for mm in msgs:
            self.m.midi(mm)

    def close(self):
        self.bank.close()


def patch(n, inc_table, seed=1, **kw):
    """A silent bank (inc 0) with the c4 patch distribution; kw overrides whole arrays or scalars."""
    arrs = synthetic.poly_bank(n, seed, inc_table)
    arrs["inc"][:] = 0
    arrs["gate"][:] = 0
    for k, v in kw.items():
        arrs[k] = np.broadcast_to(np.asarray(v, arrs[k].dtype), (n,)).copy()
    return arrs


def on(n):
    return [0x90, n, 100]


def off(n):
    return [0x80, n, 0]


def test_first_free_order(smx, orc, inc_table):
    arrs = patch(1024, inc_table)
    arrs["inc"][[0, 2, 5]] = inc_table[60]
    arrs["gate"][[0, 2, 5]] = 1
    r = Rig(smx, orc, arrs)
    r.events([on(60), on(61), on(62), on(63)])
    r.check()
    assert list(r.bank.read_notes()[60:64]) == [1, 3, 4, 6]
    r.block()
    r.close()


def test_voice_reused_once_release_ends(smx, orc, inc_table):
    n = 4
    r = Rig(smx, orc, patch(n, inc_table, ar=0x40000000, dr=0x10000000, sl=0x80000000, rr=0x20000000))
    r.events([on(60), on(62), on(64), on(65)])
    r.block()
    r.check()
    r.events([off(62)])           # voice 1 releases: 8 frames from sustain to 0, inside the next block
    r.check()
    assert r.bank.read(("stage",))["stage"][1] == S
    r.block()
    assert r.bank.read(("stage",))["stage"][1] == IDLE
    r.events([on(67)])
    r.check()
    assert r.bank.read_notes()[67] == 1
    r.block()
    r.close()


def test_steal_quietest_releasing_voice(smx, orc, inc_table):
    n = 8
    arrs = patch(n, inc_table, rr=0x00100000)
    r = Rig(smx, orc, arrs)
    r.events([on(40 + i) for i in range(n)])
    # different levels: voices 0..7 at decreasing sustain, then all but 2 and 5 held
    r.keep["level"][:] = [9, 8, 7, 6, 5, 4, 3, 2]
    r.keep["level"] *= 0x10000000
    r.keep["stage"][:] = S
    r.bank.load(level=r.keep["level"], stage=r.keep["stage"])
    r.events([off(42), off(45)])
    r.block()
    r.check()
    assert not r.m.free().any()
    r.events([on(90)])
    r.check()
    assert r.bank.read_notes()[90] == 5      # releasing, lower level than voice 2
    r.block()
    r.close()


def test_steal_held_voice_reattacks(smx, orc, inc_table):
    n = 6
    arrs = patch(n, inc_table, ar=0x08000000, dr=0x01000000, sl=0x40000000)
    r = Rig(smx, orc, arrs)
    r.events([on(50 + i) for i in range(n)])
    r.block()
    r.keep["level"][:] = [5, 3, 1, 4, 2, 6]
    r.keep["level"] *= 0x08000000
    r.bank.load(level=r.keep["level"])
    r.events([on(100)])
    r.check()
    assert r.bank.read_notes()[100] == 2 and r.bank.read_notes()[52] == -1
    assert r.bank.read(("stage",))["stage"][2] == R
    r.block()
    assert r.keep["stage"][2] in (A, D)       # re-attacked at the block start
    r.check()
    r.close()


def test_ties_broken_by_index(smx, orc, inc_table):
    n = 16
    r = Rig(smx, orc, patch(n, inc_table, sl=0x30000000, ar=0xFFFFFFFF, dr=0xFFFFFFFF))
    r.events([on(20 + i) for i in range(n)])
    r.block()                                 # every voice sits at the same sustain level
    assert len(set(r.keep["level"].tolist())) == 1
    # 80 steals voice 0; voice 0 still has the smallest (gate, level, index), so 81 steals it again; the note_off
    # makes voice 10 the only releasing voice, and 82 takes it
    r.events([on(80), on(81), off(30), on(82)])
    r.check()
    notes = r.bank.read_notes()
    assert (notes[80], notes[81], notes[82]) == (-1, 0, 10)
    r.block()
    r.close()


def test_note_on_of_held_note(smx, orc, inc_table):
    n = 4
    r = Rig(smx, orc, patch(n, inc_table))
    r.events([on(60), on(61)])
    r.block()
    r.events([on(60)])                        # released from voice 0 (not free: its envelope runs), takes voice 2
    r.check()
    notes = r.bank.read_notes()
    assert notes[60] == 2 and notes[61] == 1
    assert list(r.bank.read(("gate",))["gate"][:3]) == [0, 1, 1]
    r.events([on(62), on(63)])                # 62 takes voice 3; then the bank is full: 63 steals released voice 0
    r.check()
    assert r.bank.read_notes()[63] == 0
    r.block()
    r.events([on(63), on(63)])                # never free within the batch: each steals the voice it released
    r.check()
    r.block()
    r.close()


def test_note_off_unmapped_is_noop(smx, orc, inc_table):
    n = 64
    arrs = patch(n, inc_table)
    arrs["inc"][:] = inc_table[70]
    arrs["gate"][:] = 1
    r = Rig(smx, orc, arrs)
    r.events([off(70), off(0), [0x90, 70, 0]])
    r.check()
    assert (r.bank.read(("gate",))["gate"] == 1).all()
    r.block()
    r.close()


def test_velocity_zero_and_0x80(smx, orc, inc_table):
    r = Rig(smx, orc, patch(32, inc_table))
    r.events([on(60), on(61), [0x90, 60, 0], [0x80, 61, 64]])
    r.check()
    assert (r.bank.read_notes() == -1).all()
    assert list(r.bank.read(("gate",))["gate"][:2]) == [0, 0]
    r.close()


def test_ignored_statuses_channels_and_sizes(smx, orc, inc_table):
    r = Rig(smx, orc, patch(32, inc_table))
    r.events([[0x91, 60, 100], [0xB0, 23, 5], [0x81, 60, 0], [0xE0, 1, 2], [0x9F, 61, 1]])
    r.bank.midi_event(np.array([0x90, 60], np.uint8))          # not 3 bytes
    r.bank.midi_event(np.array([0x90, 60, 100, 0], np.uint8))
    r.check()
    assert (r.bank.read_notes() == -1).all() and (r.bank.read(("inc",))["inc"] == 0).all()
    r.events([on(60), [0x81, 60, 0]])
    r.check()
    assert r.bank.read_notes()[60] == 0
    r.close()


def test_note_mod_128_and_negative(smx, orc, inc_table):
    r = Rig(smx, orc, patch(32, inc_table))
    r.bank.note_on(200)
    r.m.note_on(200)
    r.events([[0x90, 0xC8 - 1, 1]])          # byte 199 -> note 71
    r.check()
    notes = r.bank.read_notes()
    assert notes[72] == 0 and notes[71] == 1
    assert r.bank.read(("inc",))["inc"][0] == orc.orc_note_to_inc(72)
    r.bank.note_off(72 + 128)
    r.m.note_off(72 + 128)
    r.check()
    for fn in (smx.lib().smx_poly_note_on, smx.lib().smx_poly_note_off):
        assert fn(r.bank._h, -1) == -1                           # SMX_E_ARG
    r.check()
    r.close()


def test_load_clears_maps(smx, orc, inc_table):
    n = 64
    r = Rig(smx, orc, patch(n, inc_table))
    r.events([on(60), on(61)])
    r.bank.load(phase=r.keep["phase"], level=r.keep["level"])   # neither inc nor gate: maps kept
    r.check()
    r.bank.load(gate=r.keep["gate"])
    r.m.clear_maps()
    r.check()
    r.events([off(60)])                                         # unmapped now: gate of voice 0 stays 1
    r.check()
    assert r.bank.read(("gate",))["gate"][0] == 1
    r.events([on(61)])
    r.bank.load(inc=r.keep["inc"])
    r.m.clear_maps()
    r.check()
    r.block()
    r.close()


def test_batch_larger_than_launch_cap(smx, orc, inc_table):
    n = 300
    r = Rig(smx, orc, patch(n, inc_table, rr=0x01000000))
    rng = np.random.default_rng(7)
    msgs = []
    for _ in range(1000):
        nt = int(rng.integers(0, 128))
        msgs.append(on(nt) if rng.random() < 0.6 else off(nt))
    r.events(msgs)
    r.check()
    r.block()
    r.events(msgs[::-1])
    r.check()
    r.block()
    r.close()


def test_single_calls_equal_one_batch(smx, orc, inc_table):
    n = 200
    arrs = patch(n, inc_table)
    rng = np.random.default_rng(11)
    msgs = [(on if rng.random() < 0.7 else off)(int(rng.integers(0, 128))) for _ in range(300)]
    a, b = smx.PolyBank(n), smx.PolyBank(n)
    a.load(**arrs)
    b.load(**arrs)
    a.midi_events(np.array(msgs, np.uint8))
    for mm in msgs:
        b.midi_event(np.array(mm, np.uint8))
    ra, rb = a.read(), b.read()
    for k in ra:
        assert np.array_equal(ra[k].view(np.uint32), rb[k].view(np.uint32)), k
    assert np.array_equal(a.read_notes(), b.read_notes())
    assert np.array_equal(a.run(64)[0], b.run(64)[0])
    a.close()
    b.close()


def test_events_between_async_blocks(smx, orc, inc_table):
    n = 4096
    r = Rig(smx, orc, patch(n, inc_table, ar=0x02000000, rr=0x00800000))
    rng = np.random.default_rng(5)
    for blk in range(12):
        msgs = [(on if rng.random() < 0.65 else off)(int(rng.integers(0, 128))) for _ in range(int(rng.integers(0, 40)))]
        if msgs:
            r.events(msgs)
        r.bank.run_async(64)
        want = np.zeros(128, np.int32)
        orc.orc_poly_run(C.byref(r.ob), want, 64)
    r.bank.sync()
    got = r.bank.read()
    for k in ("inc", "gate", "stage", "phase", "level"):
        assert np.array_equal(got[k], r.keep[k]), k
    assert np.array_equal(got["y"].view(np.uint32), r.keep["y"].view(np.uint32))
    assert np.array_equal(r.bank.read_notes(), r.m.n2v)
    r.block()
    r.close()


# ---- fuzz ---------------------------------------------------------------------------------------------------------
def _fuzz_bank(n, seed, inc_table, mix):
    arrs = synthetic.poly_bank(n, seed, inc_table)
    rng = np.random.default_rng(seed)
    # fast envelopes for part of the bank, so that releases end and voices come free again within the test
    fast = rng.random(n) < 0.5
    arrs["rr"] = np.where(fast, np.uint32(0x04000000), arrs["rr"]).astype(np.uint32)
    arrs["ar"] = np.where(fast, np.uint32(0x08000000), arrs["ar"]).astype(np.uint32)
    if mix == "free":            # mostly free: a few voices sounding
        live = rng.random(n) < 0.05
    else:                        # fully held: every voice sounding, envelopes anywhere
        live = np.ones(n, bool)
        arrs["stage"] = rng.integers(0, 5, n).astype(np.uint32)
        arrs["level"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        arrs["level"][rng.random(n) < 0.3] = 0x20000000          # ties on the level
    arrs["inc"] = np.where(live, arrs["inc"] | np.uint32(1), 0).astype(np.uint32)
    arrs["gate"] = np.where(live, 1, np.where(rng.random(n) < 0.5, arrs["gate"], 0)).astype(np.uint32)
    if mix == "held":
        arrs["gate"][:] = 1
    return arrs


def _fuzz_events(rng, mix, count):
    p_on = {"free": 0.7, "held": 0.9, "offs": 0.35}[mix]
    lo, hi = (48, 72) if mix == "offs" else (0, 128)           # dense note-offs: few notes, often mapped
    out = []
    for _ in range(count):
        nt = int(rng.integers(lo, hi))
        u = rng.random()
        if u < p_on:
            out.append([0x90, nt, int(rng.integers(1, 128))])
        elif u < p_on + (1 - p_on) * 0.5:
            out.append([0x80, nt, 0])
        elif u < p_on + (1 - p_on) * 0.9:
            out.append([0x90, nt, 0])
        else:
            out.append([int(rng.choice([0xB0, 0x91, 0x81, 0xA0])), nt, 1])
    return out


@pytest.mark.parametrize("n,nf,blocks", [(1 << 10, 64, 10), (1 << 18, 64, 4), (1 << 22, 8, 3)])
@pytest.mark.parametrize("mix", ["free", "held", "offs"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_against_model(smx, orc, inc_table, n, nf, blocks, mix, seed):
    s = 0x90E0 + 131 * seed + {"free": 0, "held": 1, "offs": 2}[mix] + n
    r = Rig(smx, orc, _fuzz_bank(n, s, inc_table, mix))
    rng = np.random.default_rng(s)
    for blk in range(blocks):
        count = int(rng.choice([0, 1, 5, 64, 65, 200]))
        if mix == "held" and n > 1 << 12:
            count = min(count, 65)          # the model's steal search is a pass over the whole bank per event
        msgs = _fuzz_events(rng, mix, count)
        if msgs:
            r.events(msgs)
        r.check("block %d" % blk)
        r.block(nf)
    r.close()


# ---- host program -------------------------------------------------------------------------------------------------
def test_host_poly_fake_jack(smx, orc, inc_table, tmp_path):
    """SYNTH_POLY in --fake-jack mode: L then R floats per block, bit-exact against the model + orc_poly_run."""
    elf = os.path.join(ROOT, "host", "synth.dynamic.host.elf")
    n, nblocks, nframes = 512, 12, 64
    patch_s = (0.125, 0x02000000, 0x00400000, 0x60000000, 0x01000000, 100 | (156 << 16))
    rng = np.random.default_rng(3)
    rec = []
    for blk in range(nblocks):
        for _ in range(int(rng.integers(0, 12))):
            nt = int(rng.integers(30, 90))
            st = 0x90 if rng.random() < 0.6 else 0x80
            rec.append((blk, 3, st, nt, 90 if st == 0x90 else 0))
        if blk == 3:
            rec.append((blk, 2, 0x90, 10, 0))           # not 3 bytes: ignored
    ev = np.zeros(len(rec), np.dtype([("block", "<u4"), ("size", "u1"), ("b", "u1", 3)]))
    for i, (b, sz, *m) in enumerate(rec):
        ev[i] = (b, sz, m)
    evf, outf = tmp_path / "ev.bin", tmp_path / "out.f32"
    ev.tofile(evf)
    env = dict(os.environ, SYNTH_POLY=str(n), SYNTH_POLY_PATCH="%r,%d,%d,%d,%d,%d" % patch_s)
    env.pop("SYNTH_RANKS", None)
    p = subprocess.run([elf, "--fake-jack", str(nblocks), str(nframes), str(evf), str(outf)], env=env,
                       stdin=subprocess.DEVNULL, capture_output=True, timeout=120)
    assert p.returncode == 1, p.stderr.decode()                  # EOF on stdin -> exit(1), linux/synth.c:305-310
    assert b"fake-jack rendered" in p.stderr
    got = np.fromfile(outf, np.float32).reshape(nblocks, 2, nframes)

    z = np.zeros(n, np.uint32)
    a, ar, dr, sl, rr, pan = patch_s
    arrs = dict(inc=z.copy(), phase=z.copy(), y=np.zeros(n, np.float32), a=np.full(n, a, np.float32),
                level=z.copy(), stage=z.copy(), gate=z.copy(), ar=np.full(n, ar, np.uint32),
                dr=np.full(n, dr, np.uint32), sl=np.full(n, sl, np.uint32), rr=np.full(n, rr, np.uint32),
                pan=np.full(n, pan, np.uint32))
    ob = oracle.PolyBank(n=n, **{k: v.ctypes.data for k, v in arrs.items()})
    m = Model(orc, arrs)
    for blk in range(nblocks):
        for (b, sz, *msg) in rec:
            if b == blk and sz == 3:
                m.midi(msg)
        want = np.zeros(2 * nframes, np.int32)
        orc.orc_poly_run(C.byref(ob), want, nframes)
        wf = np.array([orc.orc_bus_to_float(int(s)) for s in want], np.float32).reshape(nframes, 2)
        assert np.array_equal(got[blk, 0].view(np.uint32), wf[:, 0].view(np.uint32)), blk
        assert np.array_equal(got[blk, 1].view(np.uint32), wf[:, 1].view(np.uint32)), blk
    assert np.abs(got).max() > 0


def test_host_poly_refuses_ranks(tmp_path):
    elf = os.path.join(ROOT, "host", "synth.dynamic.host.elf")
    (tmp_path / "ev.bin").write_bytes(b"")
    env = dict(os.environ, SYNTH_POLY="1024", SYNTH_RANKS="2")
    p = subprocess.run([elf, "--fake-jack", "1", "64", str(tmp_path / "ev.bin"), str(tmp_path / "o.f32")], env=env,
                       stdin=subprocess.DEVNULL, capture_output=True, timeout=60)
    assert p.returncode == 1 and b"SYNTH_POLY does not shard" in p.stderr
    assert not (tmp_path / "o.f32").exists()
