"""GPU: the poly voice bank where its kernels change shape -- the allocator's scan grids and list merge
(poly_alloc.hip), voice placements that stress the per-workgroup list truncations, the 64-event launch cap on
multi-workgroup banks, and the grid-stride and thread-count forms of the render kernel (poly_bank.hip).

The allocator is checked as in tests/test_poly_notes_gpu.py: the device's inc/gate/stage and note map must equal
the sequential model of the rule (include/synth_mi355x.h) after every batch, and the next block's bus must be
bit-exact against oracle orc_poly_run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_poly_bank_gpu import _run_case
from test_poly_notes_gpu import IDLE, R, S, Rig, off, on, patch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SCAN_NT, MAX_WG = 512, 128       # poly_alloc.hip SCAN_NT, smx_common.h POLY_ALLOC_MAX_WG


def scan_grid(n):
    """launch_poly_alloc's scan grid: (gx, tiles per workgroup)."""
    tiles = -(-n // SCAN_NT)
    tpw = -(-tiles // min(tiles, MAX_WG))
    return -(-tiles // tpw), tpw


def span(n, g):
    """The voices scan workgroup g reads."""
    _, tpw = scan_grid(n)
    return g * tpw * SCAN_NT, min(n, (g + 1) * tpw * SCAN_NT)


def held_bank(n, inc_table, seed):
    """Every voice sounding and held (gate 1, stage S) at a loud level in [2^30, 2^32): nothing free, and the voices
    a test makes releasing (gate 0) or quieter are stolen first."""
    rng = np.random.default_rng(seed)
    arrs = patch(n, inc_table, seed)
    arrs["inc"][:] = inc_table[rng.integers(0, 128, n)]
    arrs["gate"][:] = 1
    arrs["stage"][:] = S
    arrs["level"][:] = rng.integers(1 << 30, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return arrs, rng


def releasing(arrs, idx, level):
    arrs["gate"][idx] = 0
    arrs["stage"][idx] = R
    arrs["level"][idx] = level


def ons(notes):
    return [on(int(m) % 128) for m in notes]


# ---- A. the allocator at the edges of its scan grid ---------------------------------------------------------------
# tiles = ceil(n / 512), G = min(tiles, 128), tpw = ceil(tiles / G), gx = ceil(tiles / tpw) scan workgroups;
# poly_alloc_apply pads the gx key lists to Gp (the next power of two) for its merge tree.
#          n   tiles  tpw   gx   Gp
#          1       1    1    1    1   one voice
#        511       1    1    1    1   one partial tile
#        512       1    1    1    1   one full tile
#        513       2    1    2    2   a second workgroup holding one voice
#       1536       3    1    3    4   padded merge
#      65536     128    1  128  128   one tile per workgroup, every list of the merge used
#      65537     129    2   65  128   two tiles per workgroup, gx < G: the last workgroup holds one voice
#   2^20 + 17   2049   17  121  128   the last workgroup holds 8 full tiles and 17 voices
GRID_EDGES = [(1, 1), (511, 1), (512, 1), (513, 2), (1536, 3), (65536, 128), (65537, 65), ((1 << 20) + 17, 121)]


@pytest.mark.parametrize("n,gx", GRID_EDGES)
def test_alloc_scan_grid_edges(smx, orc, inc_table, n, gx):
    assert scan_grid(n)[0] == gx
    arrs, rng = held_bank(n, inc_table, 0x5CA0 + n)
    # per scan workgroup: its last voice free, three releasing voices at tied or extreme levels, and the voices on
    # both sides of its boundary with the next one releasing at the same level
    for g in range(gx):
        lo, hi = span(n, g)
        arrs["inc"][hi - 1] = 0
        pick = rng.integers(lo, hi, 3)
        releasing(arrs, pick, np.array([0x100, 0x100, [0, 0x80000000, 0xFFFFFFFF][g % 3]], np.uint32))
        if hi < n:
            releasing(arrs, [hi - 2, hi], 0x100)
    r = Rig(smx, orc, arrs)
    r.events(ons(range(65)))                 # launches of 64 and 1: free picks, then steals
    r.check("65 note-ons")
    r.block()
    msgs = []
    for _ in range(200):                     # re-ons of held notes, note-offs, new notes
        m = int(rng.integers(0, 96))
        msgs.append(on(m) if rng.random() < 0.75 else off(m))
    r.events(msgs)
    r.check("mixed 200")
    r.block()
    r.events([off(m) for m in range(64)] + ons(range(64, 129)))
    r.check("64 note-offs + 65 note-ons")
    r.block()
    r.close()


# ---- B. adversarial placement --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,g,count", [(4096, 3, 300),              # gx 8: a middle workgroup, full span
                                       (1300, 2, 200),              # gx 3: the last workgroup, 276 voices
                                       (65536 + 300, 64, 300)])     # gx 65: the last workgroup, 300 voices
def test_best_keys_crowd_one_workgroup(smx, orc, inc_table, n, g, count):
    """More than 128 releasing voices, the globally smallest keys, all inside scan workgroup g's span: its list of
    128 keys is truncated, and 64 steals per launch must come from it alone, in (level, index) order."""
    gx, _ = scan_grid(n)
    assert g < gx
    arrs, rng = held_bank(n, inc_table, 0xC0DE + n)
    lo, hi = span(n, g)
    idx = rng.choice(np.arange(lo, hi), count, replace=False)
    releasing(arrs, idx, rng.integers(0, 16, count).astype(np.uint32) << 24)    # many ties on each level
    r = Rig(smx, orc, arrs)
    for k, cnt in enumerate((64, 64, 65)):
        r.events(ons(range(64 * k, 64 * k + cnt)))
        r.check("batch %d" % k)
        assert not r.m.free().any()
        got = r.bank.read_notes()
        assert ((got[got >= 0] >= lo) & (got[got >= 0] < hi)).all()       # every steal inside the span
    r.block()
    r.close()


@pytest.mark.parametrize("n,nfree", [(1300, 129), (65536 + 300, 150), ((1 << 20) + 17, 129)])
def test_free_voices_only_in_last_workgroup(smx, orc, inc_table, n, nfree):
    """Free voices only in the last scan workgroup (whose span is partial), behind full workgroups with empty free
    lists; releasing voices spread over the bank.  Batches of 64, 65, 65 note-ons use up the free voices and then
    steal, the crossing inside a launch."""
    gx, _ = scan_grid(n)
    arrs, rng = held_bank(n, inc_table, 0xF3EE + n)
    lo, hi = span(n, gx - 1)
    assert hi - lo < 512 * scan_grid(n)[1]
    arrs["inc"][rng.choice(np.arange(lo, hi), nfree, replace=False)] = 0
    releasing(arrs, rng.choice(lo, 200, replace=False), rng.integers(0, 4, 200).astype(np.uint32) << 28)
    r = Rig(smx, orc, arrs)
    done = 0
    for cnt in (64, 65, 65):
        r.events(ons(range(done, done + cnt)))
        done += cnt
        r.check("%d note-ons" % done)
    assert not r.m.free().any()
    r.block()
    r.close()


@pytest.mark.parametrize("seq", [(64, 65), (1, 64, 65), (2, 64, 64)])
@pytest.mark.parametrize("scope", ["workgroup", "bank"])
@pytest.mark.parametrize("nfree", [127, 128, 129])
def test_free_count_at_list_size(smx, orc, inc_table, nfree, scope, seq):
    """Exactly 127, 128 or 129 free voices, in one scan workgroup (its free list full or overflowing) or over the
    whole bank (the concatenated list), then batches of note-ons that run from free picks into steals: one of the
    three batch sequences crosses inside a launch for each count."""
    n = 2048                                                             # gx 4
    arrs, rng = held_bank(n, inc_table, 0x127 + nfree)
    lo, hi = span(n, 2) if scope == "workgroup" else (0, n)
    arrs["inc"][rng.choice(np.arange(lo, hi), nfree, replace=False)] = 0
    rel = rng.choice(n, 150, replace=False)
    rel = rel[arrs["inc"][rel] != 0]
    releasing(arrs, rel, rng.integers(0, 1 << 31, len(rel)).astype(np.uint32))
    r = Rig(smx, orc, arrs)
    done = 0
    for cnt in seq:
        r.events(ons(range(done, done + cnt)))
        done += cnt
        r.check("%d note-ons" % done)
    assert not r.m.free().any()
    r.block()
    r.close()


@pytest.mark.parametrize("n", [1024, 1536, 65537])
def test_level_ties_across_workgroups(smx, orc, inc_table, n):
    """Releasing voices at one level on both sides of every scan-workgroup boundary and scattered in every
    workgroup: which of them a steal takes depends on the index alone, across lists."""
    gx, _ = scan_grid(n)
    arrs, rng = held_bank(n, inc_table, 0x71E + n)
    L = 0x30000000
    for g in range(gx):
        lo, hi = span(n, g)
        releasing(arrs, rng.choice(np.arange(lo, hi), min(40, hi - lo), replace=False), L)
        releasing(arrs, np.arange(max(lo, hi - 12), min(n, hi + 12)), L)
    releasing(arrs, rng.choice(n, 30, replace=False), L + 1)            # a second level of ties behind the first
    r = Rig(smx, orc, arrs)
    for k in range(3):
        r.events(ons(range(64 * k, 64 * k + 64)))
        r.check("batch %d" % k)
    r.block()
    r.close()


def test_extreme_levels(smx, orc, inc_table):
    """Levels 0, 0x80000000 and 0xFFFFFFFF, releasing and held, in every workgroup: bit 31 of the level is bit 62
    of the steal key, just below the gate."""
    n = 1536
    arrs, rng = held_bank(n, inc_table, 0xE7)
    for lvl in (0, 0x80000000, 0xFFFFFFFF):
        releasing(arrs, rng.choice(n, 20, replace=False), lvl)
        arrs["level"][rng.choice(n, 20, replace=False)] = lvl           # held (or releasing) at the same level
    r = Rig(smx, orc, arrs)
    done = 0
    for cnt in (64, 64, 65):
        r.events(ons(range(done, done + cnt)))
        done += cnt
        r.check("%d note-ons" % done)
    r.block()
    r.close()


def test_idle_held_and_released_free_again_in_one_launch(smx, orc, inc_table):
    """Gate 1 in stage IDLE is held (not free); gate 0 in stage R is releasing (not free).  A note_on and a note_off
    of the same voice in one launch leave it free again when its stage is IDLE, and not when an inc-0 voice was
    sitting in stage S."""
    n = 1024                                                              # gx 2
    arrs, rng = held_bank(n, inc_table, 0x1D7E)
    arrs["inc"][300] = 0                                                  # free by inc 0, gate 0, stage S
    arrs["gate"][300] = 0
    arrs["gate"][700] = 0                                                 # free by gate 0 + IDLE
    arrs["stage"][700] = IDLE
    held_idle = np.array([5, 511, 512, 1000])
    arrs["stage"][held_idle] = IDLE
    arrs["level"][held_idle] = 0
    releasing(arrs, [100, 600, 900], [0x40000000, 0x20000000, 0x20000000])
    r = Rig(smx, orc, arrs)
    r.events([on(60), off(60), on(61), off(61), on(62), on(63), on(64), on(65), on(66), on(67), on(68), on(69)])
    r.check()
    notes = r.bank.read_notes()
    assert notes[60] == -1 and notes[61] == -1 and notes[62] == 700
    assert notes[63] == 600 and notes[64] == 900                         # releasing, quietest then lowest index
    r.block()
    r.close()


# ---- C. the 64-event launch cap on a multi-workgroup bank ----------------------------------------------------------
def cap_bank(smx, orc, inc_table, seed):
    n = 2560                                                              # gx 5, Gp 8
    arrs, rng = held_bank(n, inc_table, seed)
    arrs["inc"][rng.choice(n, 40, replace=False)] = 0
    rel = rng.choice(n, 400, replace=False)
    releasing(arrs, rel, rng.integers(0, 8, 400).astype(np.uint32) << 24)
    return Rig(smx, orc, arrs), rng


@pytest.mark.parametrize("count", [63, 64, 65, 128, 129])
def test_launch_cap_counts(smx, orc, inc_table, count):
    r, rng = cap_bank(smx, orc, inc_table, 0xCA9 + count)
    for k in range(3):
        msgs = []
        for _ in range(count):
            m = int(rng.integers(0, 128))
            msgs.append(on(m) if rng.random() < 0.7 else off(m))
        r.events(msgs)
        r.check("batch %d" % k)
        r.block()
    r.close()


def test_launch_of_note_offs_only(smx, orc, inc_table):
    """The first 64 events of a batch are all note-offs (mapped and unmapped): that launch runs no scan.  The
    next launch's note-ons see its releases."""
    r, rng = cap_bank(smx, orc, inc_table, 0x0FF)
    r.events(ons(range(100)))
    r.check()
    r.block()
    offs = [off(m) for m in rng.permutation(128)[:64]]
    r.events(offs + ons(range(100, 128)) + [off(3), on(3)])
    r.check()
    r.block()
    r.close()


@pytest.mark.parametrize("pos", [63, 64])
def test_held_note_on_at_launch_edge(smx, orc, inc_table, pos):
    """A note_on of a held note as the 64th event of a launch, and as the 65th (the first of the next)."""
    r, _ = cap_bank(smx, orc, inc_table, 0x64 + pos)
    r.events(ons(range(64)))
    r.check()
    batch = ons(range(64, 64 + pos)) + [on(5)] + ons(range(64 + pos, 64 + pos + 3))
    r.events(batch)
    r.check()
    r.block()
    r.close()


def test_64_steals_of_fresh_voices_in_one_launch(smx, orc, inc_table):
    """64 free voices (inc 0, gate 0, stage S: loud and not free once released) take notes 0..63; then a launch of
    64 note_ons of those held notes releases 64 voices and steals 64 others (quieter, releasing): 128 distinct voices
    touched in one launch, the bound the lists are sized for."""
    n = 2560
    arrs, rng = held_bank(n, inc_table, 0x128)
    idx = rng.permutation(n)
    arrs["inc"][idx[:64]] = 0
    arrs["gate"][idx[:64]] = 0
    releasing(arrs, idx[64:264], rng.integers(0, 1 << 20, 200).astype(np.uint32))
    r = Rig(smx, orc, arrs)
    r.events(ons(range(64)))
    r.check()
    before = r.bank.read_notes()[:64].copy()
    r.events(ons(range(64)))
    r.check()
    after = r.bank.read_notes()[:64]
    assert len(set(before.tolist()) | set(after.tolist())) == 128
    r.events(ons(range(64)) + [on(0)])
    r.check()
    r.block()
    r.close()


# ---- D. the render kernel ------------------------------------------------------------------------------------------
# launch_poly_bank: 512 threads, rows = n_pad / 512, grid min(rows, 1024): above 512 Ki voices a workgroup renders
# more than one row.  (1<<20) + 1027 voices: n_pad 1026 Ki, 2052 rows -> 4 workgroups of 3 rows, 1020 of 2;
# 2^22: 8192 rows, 8 per workgroup.  The 64-frame blocks run poly_bank_kernel<512, true>; 1, 63 and 65 frames
# (65 = 64 + 1 on the host) the general form, on the same state.
@pytest.mark.parametrize("n", [(1 << 20) + 1024 + 3, 1 << 22])
def test_render_grid_stride(smx, orc, inc_table, n):
    _run_case(smx, orc, n, 0x5EED0600 + n % 1009, inc_table, [64, 1, 64, 63, 65, 64])


# The tuning overrides are read once per process: each form in a process of its own (tests/poly_form_worker.py).
#   SMX_POLY_NT=256  on 300 000 voices: 1172 rows, grid 1024 -> 148 workgroups of 2 rows
#   SMX_POLY_NT=1024 on 600 000 voices: 586 rows, grid 512 (its own cap) -> 74 workgroups of 2 rows
#   SMX_POLY_GRID=7  on 100 000 voices: 196 rows of 512 -> 28 per workgroup
@pytest.mark.parametrize("switch,n", [("SMX_POLY_NT=256", 300000), ("SMX_POLY_NT=1024", 600000),
                                      ("SMX_POLY_GRID=7", 100000)])
def test_render_tuning_forms(smx, switch, n):
    env = dict(os.environ)
    for k in ("SMX_POLY_NT", "SMX_POLY_GRID", "SMX_POLY_NO_DEFER"):
        env.pop(k, None)
    k, v = switch.split("=")
    env[k] = v
    p = subprocess.run([sys.executable, os.path.join(HERE, "poly_form_worker.py"), str(n)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().startswith("ok"), p.stdout[-500:]
