"""CPU tests of oracle.fixed_point_grad, the restatement of the reproducible mode's fixed-point sum (seg_grad.hip,
seg_reduce_kernel with deterministic = 1 on a row whose segment is not sorted): hand-made segments with known answers, and
an independent per-element evaluation in Python integers on random segments."""
import numpy as np

import oracle as O


def _one(addends):
    """One segment of one channel -> its float32 result."""
    a = np.asarray(addends, np.float32).reshape(-1, 1)
    return O.fixed_point_grad(1, np.zeros(len(a), np.int64), a)[0, 0]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_length_one_segment_is_exact():
    for v in (1.0, -3.25, 1e-30, -7e37, 3.4e38, 2.0 ** -126, 2.0 ** -149, 5 * 2.0 ** -149, 1.17e-40):
        assert _bits(_one([v])) == _bits(np.float32(v)), v


def test_ties_round_half_to_even():
    # [1, -1, x]: 3 entries (logc = 2), max 1.0 (exponent field 127) -> k = 62 - 2 - 1 = 59, unit 2^-59; x = q * 2^-60 is
    # q/2 units: 1/2 -> 0, 3/2 -> 2, 5/2 -> 2, 7/2 -> 4 (half to even; half away from zero would give 1, 2, 3, 4)
    u = 2.0 ** -59
    for q, units in ((1, 0), (3, 2), (5, 2), (7, 4), (-1, 0), (-3, -2), (-5, -2)):
        got = _one([1.0, -1.0, q * 2.0 ** -60])
        assert got == np.float32(units * u), (q, got)
    # the same x, order of the entries shuffled: same bits
    assert _bits(_one([3 * 2.0 ** -60, 1.0, -1.0])) == _bits(np.float32(2 * u))


def test_subnormal_maximum():
    # every |addend| subnormal: exponent field 0 -> k = 62 - logc + 126, the sum is exact
    d = 2.0 ** -149
    assert _one([5 * d, 3 * d]) == np.float32(8 * d)
    assert _one([5 * d, -3 * d, 1000 * d]) == np.float32(1002 * d)
    # a normal maximum beside subnormals: they fall below the unit 2^-(k) and vanish
    assert _one([1.0, d]) == np.float32(1.0)


def test_cancellation_gives_plus_zero():
    for seg in ([1.0, -1.0], [-1.0, 1.0], [-0.0], [-0.0, -0.0], [0.75, -0.25, -0.5], [-(2.0 ** -149), 2.0 ** -149]):
        assert _bits(_one(seg)) == 0, seg


def test_mixed_magnitudes_of_two_to_the_sixty():
    big, small = 2.0 ** 60, 2.0 ** -60
    # max 2^60 (exponent field 187) over 3 entries -> k = 62 - 2 - 61 = -1: 2^-60 is far below the unit 2^1
    assert _one([big, small, -big]) == np.float32(0.0)
    assert _one([small, big, small]) == np.float32(big)
    # max 2^-60 -> every addend a multiple of the unit: exact
    assert _one([small, 3 * small, -small]) == np.float32(3 * small)
    # the conversion back rounds twice, int64 -> float64 -> float32, as the kernel does: max 2^57 over 3 entries ->
    # k = 62 - 2 - 58 = 2; fx = 2^59 + 2^35 + 1 -> float64 2^59 + 2^35 (ulp 2^7) -> float32 ties to even: 2^59 -> 2^57.
    # One rounding of the exact sum would give 2^57 + 2^34.
    assert _one([2.0 ** 57, 2.0 ** 33, 0.25]) == np.float32(2.0 ** 57)


def test_non_finite_keeps_the_plain_sum_per_element():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    a = np.array([[1.0, 1.0, 2.0], [inf, 2.0, -inf], [1.0, nan, inf]], np.float32)      # 3 entries of one row, 3 channels
    got = O.fixed_point_grad(1, np.zeros(3, np.int64), a)[0]
    assert got[0] == inf and np.isnan(got[1]) and np.isnan(got[2])
    # a finite channel beside them is still the fixed-point sum
    b = np.array([[inf, 1.0], [1.0, 2.0 ** -30]], np.float32)
    got = O.fixed_point_grad(1, np.zeros(2, np.int64), b)[0]
    assert got[0] == inf and got[1] == np.float32(1.0 + 2.0 ** -30)


def test_rows_channels_and_empty_rows():
    target = np.array([2, 0, 2, 2], np.int64)
    a = np.array([[1.0, 4.0], [5.0, -2.0], [2.0, 0.5], [-0.5, 0.25]], np.float32)
    got = O.fixed_point_grad(4, target, a)
    assert np.array_equal(got, np.array([[5.0, -2.0], [0.0, 0.0], [2.5, 4.75], [0.0, 0.0]], np.float32))
    assert np.all(_bits(got[[1, 3]]) == 0)
    assert O.fixed_point_grad(3, np.zeros(0, np.int64), np.zeros((0, 5), np.float32)).shape == (3, 5)


def _exact_element(vals, k):
    """One element in Python integers and fractions: the definition, independent of numpy's vectorisation."""
    from fractions import Fraction
    fx = 0
    for v in vals:
        q = Fraction(float(v)) * Fraction(2) ** k
        fl = q.numerator // q.denominator
        rem = q - fl
        fx += fl + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1) else 0)
    return np.float32(np.ldexp(np.float64(fx), -k))      # int -> float64 rounds to nearest even, like the kernel


def test_random_segments_against_the_definition():
    rng = np.random.default_rng(7)
    rows, c = 12, 3
    target = rng.integers(0, rows - 2, size=300)                    # the last two rows stay empty
    target[:40] = 1                                                 # one long segment
    a = (rng.standard_normal((300, c)) * 10.0 ** rng.uniform(-30, 30, size=(300, 1))).astype(np.float32)
    got = O.fixed_point_grad(rows, target, a)
    for r in range(rows):
        sel = a[target == r]
        for ch in range(c):
            if len(sel) == 0:
                assert _bits(got[r, ch]) == 0
                continue
            mx = np.abs(sel[:, ch]).max()
            logc = (len(sel) - 1).bit_length()
            k = 62 - logc - (int(_bits(mx)) >> 23) + 126
            assert _bits(got[r, ch]) == _bits(_exact_element(sel[:, ch], k)), (r, ch)
    # the order of the entries does not matter
    perm = rng.permutation(300)
    assert np.array_equal(_bits(O.fixed_point_grad(rows, target[perm], a[perm])), _bits(got))
    # one shift for the whole call (det_grad.hip's form)
    k = 62 - 9 - (int(_bits(np.abs(a).max())) >> 23) + 126 - 1
    whole = O.fixed_point_grad(rows, target, a, shift=k)
    for r in (0, 1, 5):
        for ch in range(c):
            assert _bits(whole[r, ch]) == _bits(_exact_element(a[target == r][:, ch], k)), (r, ch)
