"""CPU: smx_poly_bend_mul, the pitch bend's Q16 increment multiplier of the poly bank (include/synth_mi355x.h,
DESIGN.md §3.5c): round(65536 * 2^(range * (b - 8192) / (8192 * 12))).  No GPU needed."""
import numpy as np
import pytest

RANGES = list(range(0, 25))


def test_centre_and_range_zero_exact(smx):
    for r in RANGES:
        assert smx.poly_bend_mul(8192, r) == 65536
    for b in (0, 1, 4096, 8191, 8193, 16383):
        assert smx.poly_bend_mul(b, 0) == 65536


@pytest.mark.parametrize("r", [1, 2, 7, 12, 24])
def test_monotonic_and_close_to_numpy(smx, r):
    b = np.arange(16384)
    got = np.array([smx.poly_bend_mul(int(x), r) for x in b], np.int64)
    assert (np.diff(got) >= 0).all()
    assert got[0] < 65536 < got[-1]
    want = np.round(65536.0 * np.exp2(r * (b - 8192) / (8192.0 * 12.0))).astype(np.int64)
    assert np.abs(got - want).max() <= 1


def test_octave_points(smx):
    assert smx.poly_bend_mul(0, 12) == 32768                 # one octave down is exact
    assert smx.poly_bend_mul(0, 24) == 16384
    assert abs(smx.poly_bend_mul(16383, 12) - 131072) <= 12   # 8191/8192 of an octave up


def test_out_of_range_arguments_clamp(smx):
    assert smx.poly_bend_mul(-5, 2) == smx.poly_bend_mul(0, 2)
    assert smx.poly_bend_mul(20000, 2) == smx.poly_bend_mul(16383, 2)
    assert smx.poly_bend_mul(0, 30) == smx.poly_bend_mul(0, 24)
    assert smx.poly_bend_mul(0, -3) == 65536
