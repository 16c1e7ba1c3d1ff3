"""Cost of the poly bank's controllers: the 64-frame block on 256 Ki voices unbent and bent, all
sound off (CC 120) on 256 Ki and 4 Mi voices, and a pedal-up launch that releases 128 sustained voices.  Device-event
time on the bank's stream, medians over REPS.  `--root DIR` imports synth_tools_amd from DIR instead (an A/B against
another tree: a library without the controllers reports only the unbent block).  `--one WHAT LOG2N` measures one
configuration per process, for `rocprofv3 --kernel-trace --stats` (tools/prof_poly_ctrl.sh)."""
import json
import os
import sys

import numpy as np

args = sys.argv[1:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if args[:1] == ["--root"]:
    root, args = os.path.abspath(args[1]), args[2:]
sys.path.insert(0, root)
import synth_tools_amd as sta                # noqa: E402
from synth_tools_amd import synthetic        # noqa: E402

REPS = 50
HAS_CTL = hasattr(sta.PolyBank, "set_controllers")


def bank(log2n):
    n = 1 << log2n
    tab = synthetic.note_inc_table(sta.lib().note_to_inc)
    b = sta.PolyBank(n)
    b.load(**synthetic.poly_bank(n, 0x5EED0004, tab))
    if HAS_CTL:
        b.set_controllers(1)
    return b


def timed(b, fn):
    out = []
    for i in range(REPS + 3):
        b.sync()
        b.timer_start()
        fn()
        t = b.timer_stop() * 1e3
        if i >= 3:
            out.append(t)
    return float(np.median(out)), float(np.min(out))


def block(log2n, bent):
    b = bank(log2n)
    if bent:
        b.midi_events(np.array([[0xE0, 0x11, 0x50]], np.uint8))
    med, mn = timed(b, lambda: b.run_async(64))
    b.close()
    return {"what": "block64_bent" if bent else "block64", "voices": 1 << log2n, "us_median": med, "us_min": mn}


def sound_off(log2n):
    b = bank(log2n)
    m = np.array([[0xB0, 120, 0]], np.uint8)
    med, mn = timed(b, lambda: b.midi_events(m))
    b.close()
    return {"what": "sound_off", "voices": 1 << log2n, "us_median": med, "us_min": mn}


def pedal_up_128(log2n):
    b = bank(log2n)
    hold = np.array([[0xB0, 64, 127]] + [[0x90, k, 100] for k in range(128)] + [[0x80, k, 0] for k in range(128)],
                    np.uint8)
    up = np.array([[0xB0, 64, 0]], np.uint8)
    out = []
    for i in range(REPS + 3):
        b.midi_events(hold)
        b.sync()
        assert b.read_sustain().sum() == 128
        b.timer_start()
        b.midi_events(up)
        t = b.timer_stop() * 1e3
        if i >= 3:
            out.append(t)
    b.close()
    return {"what": "pedal_up_128", "voices": 1 << log2n, "us_median": float(np.median(out)), "us_min": float(np.min(out))}


def run(what, log2n):
    return {"block64": lambda: block(log2n, False), "block64_bent": lambda: block(log2n, True),
            "sound_off": lambda: sound_off(log2n), "pedal_up_128": lambda: pedal_up_128(log2n)}[what]()


if __name__ == "__main__":
    if args[:1] == ["--one"]:
        print(json.dumps(run(args[1], int(args[2]))))
    else:
        todo = [("block64", 18)]
        if HAS_CTL:
            todo += [("block64_bent", 18), ("sound_off", 18), ("sound_off", 22), ("pedal_up_128", 18)]
        for what, l in todo:
            print(json.dumps(dict(run(what, l), root=os.path.basename(root) or root)), flush=True)
