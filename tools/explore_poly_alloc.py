"""Cost of the poly bank's note events (poly_alloc.hip): batches of E = 1, 64, 1024 MIDI events on 2^18 and 2^22
voices, on a silent bank (every pick finds a free voice) and on a full one (every note_on steals), next to the
64-frame block.  Device-event time per batch (copy + launches, timed on the bank's stream) and per block, medians
over REPS batches, each batch followed by one block.  One configuration per process with `--one LOG2N MIX E`
(for `rocprofv3 --kernel-trace --stats`, one run per configuration: tools/prof_poly_alloc.sh)."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import synth_tools_amd as sta                # noqa: E402
from synth_tools_amd import synthetic        # noqa: E402

REPS = 30


def bank_for(log2n, mix):
    n = 1 << log2n
    tab = synthetic.note_inc_table(sta.lib().note_to_inc)
    arrs = synthetic.poly_bank(n, 0x5EED0004, tab)
    if mix == "silent":
        arrs["inc"][:] = 0
        arrs["gate"][:] = 0
    else:                                    # every voice held, levels spread
        arrs["inc"] |= np.uint32(1)
        arrs["gate"][:] = 1
        arrs["stage"][:] = 3
        arrs["level"] = np.random.default_rng(1).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    b = sta.PolyBank(n)
    b.load(**arrs)
    return b


def batch(rng, e):
    notes = rng.integers(0, 128, e)
    st = np.where(rng.random(e) < 0.75, 0x90, 0x80)
    return np.stack([st, notes, np.full(e, 100)], 1).astype(np.uint8)


def measure(log2n, mix, e):
    b = bank_for(log2n, mix)
    rng = np.random.default_rng(log2n * 1000 + e)
    for _ in range(3):                       # warm-up: code objects, staging
        b.midi_events(batch(rng, e))
        b.run(64)
    tb, tk = [], []
    for _ in range(REPS):
        m = batch(rng, e)
        b.sync()
        b.timer_start()
        b.midi_events(m)
        tb.append(b.timer_stop() * 1e3)
        b.timer_start()
        b.run_async(64)
        tk.append(b.timer_stop() * 1e3)
    b.sync()
    b.close()
    return {"voices": 1 << log2n, "mix": mix, "events": e, "batch_us_median": float(np.median(tb)),
            "batch_us_min": float(np.min(tb)), "block64_us_median": float(np.median(tk))}


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--one":
        print(json.dumps(measure(int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))))
    else:
        for log2n in (18, 22):
            for mix in ("silent", "full"):
                for e in (1, 64, 1024):
                    print(json.dumps(measure(log2n, mix, e)), flush=True)
