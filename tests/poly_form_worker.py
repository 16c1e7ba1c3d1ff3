"""One process with one of the poly render kernel's tuning overrides set (SMX_POLY_NT, SMX_POLY_GRID; test helper
for tests/test_poly_shapes_gpu.py): 64-frame and shorter blocks of an n-voice bank against the oracle, as
tests/test_poly_bank_gpu.py checks them.  Usage: poly_form_worker.py <voices>.  Prints "ok"."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import oracle
    import synth_tools_amd as sta
    from synth_tools_amd import synthetic
    from test_poly_bank_gpu import _run_case
    n = int(sys.argv[1])
    tab = synthetic.note_inc_table(sta.lib().note_to_inc)
    _run_case(sta, oracle.load(), n, 0x5EED0700 + n % 1013, tab, [64, 1, 64, 63, 65, 64])
    print("ok")


if __name__ == "__main__":
    main()
