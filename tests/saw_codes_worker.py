"""The note-code scenarios of tests/test_saw_codes_gpu.py (test helper).  Every scenario drives a saw bank through loads,
note events and tick blocks (1..4 frames, the kernel that reads the 1-byte codes), checks each bus bit-exactly against
the closed form of the linear phasor and the bank's escape count (SawBank.code_stats) after each change, and returns
its buses.  Run as a script (usually with SMX_SAW_NO_CODES=1, the 8-byte path) it prints every scenario's buses as one
JSON object, so the test can compare the two paths on the same inputs.  Usage: saw_codes_worker.py [scenario ...]."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MIB = 1 << 20


class Model:
    """The bank as numpy sees it: increments and the phases NOW (the bank's state0 + elapsed * inc)."""

    def __init__(self, bank, inc, phase):
        self.bank, self.inc, self.phase = bank, inc.copy(), phase.copy()
        self.buses = []

    def bus(self, nf):
        on = self.inc != 0
        out = np.empty(nf, np.int32)
        with np.errstate(over="ignore"):
            for f in range(nf):
                p = (self.phase + np.uint32(f) * self.inc).view(np.int32) >> 4
                s = int(np.where(on, p, 0).sum(dtype=np.int64))
                out[f] = np.int32(((s + (1 << 31)) % (1 << 32)) - (1 << 31))
        return out

    def step(self, nf):
        want = self.bus(nf)
        got, _ = self.bank.run(nf)
        assert np.array_equal(got, want), (nf, got, want)
        with np.errstate(over="ignore"):
            self.phase += np.uint32(nf) * self.inc
        self.buses.append([int(x) for x in got])

    def advance(self, nf):
        """A long block (not checked here): moves elapsed far enough that elapsed * inc wraps."""
        self.bank.run_async(nf)
        with np.errstate(over="ignore"):
            self.phase += np.uint32(nf) * self.inc

    def set(self, voice, inc):
        self.inc[voice] = inc

    def expect_escapes(self, k):
        assert self.bank.code_stats() == k, (self.bank.code_stats(), k)


def _bank(sta, inc, phase):
    bank = sta.SawBank(len(inc))
    bank.load(inc, phase)
    return Model(bank, inc, phase)


def _rand(n, seed):
    from synth_tools_amd import synthetic
    return synthetic.splitmix64(seed, n)


def _piano(tab, n, seed, active=0.8):
    from synth_tools_amd import synthetic
    return synthetic.saw_bank(n, seed, tab, active_fraction=active)


def _all_notes(tab, n, seed):
    r = _rand(n, seed)
    inc = tab[(r % np.uint64(128)).astype(np.int64)].astype(np.uint32)
    return inc, (r >> np.uint64(32)).astype(np.uint32)


def _esc(tab):
    """An increment outside the alphabet (one above a note's)."""
    e = np.uint32(tab[60] + 1)
    assert e not in tab
    return e


def sc_frames(sta, tab, n, kind):
    """1, 2, 3 and 4 frames before and after elapsed * inc wraps."""
    inc, st = _piano(tab, n, 0x5EEDC0DE + n % 4093) if kind == "piano" else _all_notes(tab, n, 0x5EEDC0DF + n % 4093)
    m = _bank(sta, inc, st)
    m.expect_escapes(0)
    for nf in (1, 2, 3, 4):
        m.step(nf)
    m.advance(4099 if n >= (1 << 24) else 65539)
    for nf in (1, 2, 3, 4, 1):
        m.step(nf)
    m.expect_escapes(0)
    return m


def sc_escape_positions(sta, tab, n=MIB + 4096):
    """One escape at the first, a middle and the last voice: counted, and the bus stays right."""
    out = []
    for pos in (0, n // 2 + 1, n - 1):
        inc, st = _piano(tab, n, 0x5EED0E5C + pos)
        inc[pos] = _esc(tab)
        m = _bank(sta, inc, st)
        m.expect_escapes(1)
        m.advance(1000)
        for nf in (1, 4, 2):
            m.step(nf)
        out.extend(m.buses)
        m.bank.close()
    return out


def sc_event_replaces_escape(sta, tab, n=MIB):
    """A full bank with escapes at 0, in the middle and at the end: a note-on steals voice 0 (the only voice a note
    event can take from a full bank), the count goes down, and the bus is right on both sides."""
    inc, st = _all_notes(tab, n, 0x5EEDE5C0)
    esc = _esc(tab)
    for v in (0, n // 3, n - 1):
        inc[v] = esc
    m = _bank(sta, inc, st)
    m.expect_escapes(3)
    m.step(1)
    m.bank.note_on(64)                                     # no voice free: voice 0 is stolen
    m.set(0, tab[64])
    m.expect_escapes(2)
    m.advance(777)
    m.step(4)
    # the other two escapes replaced by a reload of the increments, one escape at a time
    inc2, _ = m.bank.read()
    assert np.array_equal(inc2, m.inc)
    inc2[n // 3] = tab[10]
    m.bank.load(inc2, None)
    m.inc = inc2.copy()
    m.expect_escapes(1)
    m.step(2)
    inc2[n - 1] = 0
    m.bank.load(inc2, None)
    m.inc = inc2.copy()
    m.expect_escapes(0)                                    # codable again: the coded path
    m.step(1)
    m.step(3)
    # and a single note event on the now codable bank: note_off of note 64 turns voice 0 off
    m.bank.note_off(64)
    m.set(0, 0)
    m.expect_escapes(0)
    m.step(4)
    return m


def sc_single_events(sta, tab, n=MIB):
    """Note on / off one event at a time on a half-full bank, blocks in between."""
    inc, st = _piano(tab, n, 0x5EED5E00, active=0.5)
    m = _bank(sta, inc, st)
    m.advance(5000)
    free = list(np.flatnonzero(m.inc == 0)[:8])
    for k, note in enumerate((21, 60, 127, 0, 108)):
        m.bank.note_on(note)
        m.set(free[k], tab[note])
        m.step(1 + k % 4)
    m.bank.note_off(60)
    m.set(free[1], 0)
    m.step(2)
    m.expect_escapes(0)
    return m


def sc_batch_events(sta, tab, n=MIB + 4096):
    """Batched events (smx_bank_midi_events): one batch that removes an escape (steal of voice 0 on a full bank) and
    turns voices off and on again, then batches on the codable bank."""
    inc, st = _all_notes(tab, n, 0x5EEDBA7C)
    esc = _esc(tab)
    inc[0] = esc
    inc[n // 2] = esc
    m = _bank(sta, inc, st)
    m.expect_escapes(2)
    m.advance(3000)
    m.step(1)
    # full bank: note_on 70 steals voice 0 (escape removed); note_off 70 frees it; note_on 71 takes it again
    m.bank.midi_events(np.array([[0x90, 70, 100], [0x80, 70, 0], [0x90, 71, 90]], np.uint8))
    m.set(0, tab[71])
    m.expect_escapes(1)
    m.step(4)
    # the middle escape goes by reload; then batches on a codable bank, with voices going off and back on
    inc2 = m.inc.copy()
    inc2[n // 2] = tab[33]
    inc2[5:9] = 0
    m.bank.load(inc2, None)
    m.inc = inc2.copy()
    m.expect_escapes(0)
    m.step(3)
    m.bank.midi_events(np.array([[0x90, 40, 1], [0x90, 41, 1], [0xB0, 23, 5], [0x90, 127, 5]], np.uint8))
    for v, note in zip((5, 6, 7), (40, 41, 127)):
        m.set(v, tab[note])
    m.step(2)
    m.bank.midi_events(np.array([[0x80, 41, 0], [0x90, 99, 3]], np.uint8))
    m.set(6, tab[99])                                       # 41 off frees voice 6, 99 takes it back
    m.expect_escapes(0)
    m.step(4)
    return m


def sc_round_trips(sta, tab, n=MIB):
    """smx_bank_read / smx_bank_load round trips, reloads from escape to codable and back, smx_bank_load_run."""
    inc, st = _piano(tab, n, 0x5EED7217)
    m = _bank(sta, inc, st)
    m.advance(2000)
    m.step(1)
    ginc, gst = m.bank.read()
    assert np.array_equal(ginc, m.inc) and np.array_equal(gst, m.phase)
    m.bank.load(ginc, gst)                                  # the same bank again
    m.expect_escapes(0)
    m.step(4)
    bad = ginc.copy()
    bad[12345] = _esc(tab)
    bad[777] = 1
    m.bank.load(bad, None)
    m.inc = bad.copy()
    m.expect_escapes(2)
    m.step(2)
    m.bank.load(ginc, None)
    m.inc = ginc.copy()
    m.expect_escapes(0)
    m.step(3)
    # load_run: new increments and phases and one block in one call
    inc3, st3 = _all_notes(tab, n, 0x5EED7218)
    inc3[n - 1] = _esc(tab)
    m.inc, m.phase = inc3.copy(), st3.copy()
    want = m.bus(1)
    got, _ = m.bank.load_run(inc3, st3, 1)
    assert np.array_equal(got, want)
    m.buses.append([int(x) for x in got])
    with np.errstate(over="ignore"):
        m.phase += inc3
    m.expect_escapes(1)
    inc3[n - 1] = tab[90]
    with np.errstate(over="ignore"):
        m.inc, m.phase = inc3.copy(), st3 + np.uint32(7) * inc3
    got, _ = m.bank.load_run(inc3, m.phase, 4)
    assert np.array_equal(got, m.bus(4))
    m.buses.append([int(x) for x in got])
    with np.errstate(over="ignore"):
        m.phase += np.uint32(4) * m.inc
    m.expect_escapes(0)
    m.step(1)
    return m


def sc_shard(sta, tab, n=MIB):
    """A sharded bank (one shard of one): the collective load and routed note events keep the codes."""
    inc, st = _piano(tab, n, 0x5EED54AD)
    bank = sta.SawBank(n)
    bank.shard(0, n)
    inc[3] = _esc(tab)
    bank.load(inc, st)
    m = Model(bank, inc, st)
    m.expect_escapes(1)
    m.step(4)
    inc[3] = 0
    bank.load(inc, None)
    m.inc = inc.copy()
    m.expect_escapes(0)
    m.step(1)
    bank.note_on(50)                                        # the first free voice
    m.set(int(np.flatnonzero(m.inc == 0)[0]), tab[50])
    m.expect_escapes(0)
    m.step(2)
    return m


SCENARIOS = {
    "frames_piano_1m": lambda sta, tab: sc_frames(sta, tab, MIB, "piano"),
    "frames_notes_1m": lambda sta, tab: sc_frames(sta, tab, MIB, "notes"),
    "frames_piano_1m_4096": lambda sta, tab: sc_frames(sta, tab, MIB + 4096, "piano"),
    "frames_notes_1m_4096": lambda sta, tab: sc_frames(sta, tab, MIB + 4096, "notes"),
    "frames_piano_16m": lambda sta, tab: sc_frames(sta, tab, 1 << 24, "piano"),
    "frames_notes_16m": lambda sta, tab: sc_frames(sta, tab, 1 << 24, "notes"),
    "escape_positions": sc_escape_positions,
    "event_replaces_escape": sc_event_replaces_escape,
    "single_events": sc_single_events,
    "batch_events": sc_batch_events,
    "round_trips": sc_round_trips,
    "shard": sc_shard,
}


def run(name):
    """One scenario -> its buses (a list of lists of ints)."""
    import synth_tools_amd as sta
    from synth_tools_amd import synthetic
    tab = synthetic.note_inc_table(sta.lib().note_to_inc)
    r = SCENARIOS[name](sta, tab)
    if isinstance(r, Model):
        r.bank.close()
        r = r.buses
    return r


def main():
    names = sys.argv[1:] or list(SCENARIOS)
    print(json.dumps({k: run(k) for k in names}))


if __name__ == "__main__":
    main()
