"""The saw bank's note codes (saw_bank.hip: 1-byte codes instead of 4-byte increments on the tick path while no voice
holds an increment outside the note alphabet).  Every scenario of tests/saw_codes_worker.py checks its buses bit-exactly
against the closed form and the escape count after every load and note event; the same scenarios then run in a child
process with SMX_SAW_NO_CODES=1 (the 8-byte path) and must give the same buses."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import saw_codes_worker as w

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_buses = {}


@pytest.mark.parametrize("name", list(w.SCENARIOS))
def test_coded_scenario(name):
    _buses[name] = w.run(name)


def test_same_buses_without_codes():
    names = list(w.SCENARIOS)
    for k in names:
        if k not in _buses:
            _buses[k] = w.run(k)
    env = dict(os.environ, SMX_SAW_NO_CODES="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "saw_codes_worker.py")] + names, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-4000:]
    other = json.loads(r.stdout.strip().splitlines()[-1])
    for k in names:
        assert other[k] == _buses[k], k


def test_code_stats_small_bank():
    """Banks below 2^16 voices keep no codes: the query says so instead of answering."""
    import synth_tools_amd as sta
    bank = sta.SawBank(5000)
    with pytest.raises(Exception):
        bank.code_stats()
    bank.close()
    big = sta.SawBank(1 << 16)
    assert big.code_stats() == 0
    tab = np.array([sta.lib().note_to_inc(n) for n in range(128)], np.uint32)
    inc = np.zeros(1 << 16, np.uint32)
    inc[::7] = tab[60]
    inc[100] = 3
    big.load(inc, None)
    assert big.code_stats() == 1
    big.close()
