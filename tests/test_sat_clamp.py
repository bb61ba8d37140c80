"""The SIGMA pass's threshold conversions (sgh_ceil_sat_max / sgh_floor_sat_min and the rounding-band
test's negated axis in csrc/sg_stack_hist.hip) against the forms they replace.

The kernel used to clamp the threshold as a double (sgh_ceil_clamp: max(x, 0), min(., 65536), ceil,
convert; sgh_floor_clamp: min(x, 65535), max(., -1), floor, convert) and then clamp the integer
against the kept interval (max with A, min with B).  It now rounds first, converts with
v_cvt_i32_f64, which saturates at the ends of the int32 range, and clamps the integer alone:
max(min(i, 65536), A) and min(max(i, -1), B).  Both forms are restated here in numpy and compared
for every finite double that matters: around every integer from -3 to 65539 (the integer, its two
neighbouring doubles, the half between), around the int32 limits, huge and tiny magnitudes, and
every pair with the bounds A and B at their ends and inside.

The rounding-band test of the high half runs on the negated axis: amb0 = max(ceil_clamp(bhi - tol), A)
is computed as -min(max(floor(tol - bhi), -65536), -A); tol - bhi == -(bhi - tol) holds for every
pair of doubles because rounding to nearest is symmetric.
"""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
BOUNDS_A = [0, 1, 777, 65535, 65536]        # 0 <= A <= 65536
BOUNDS_B = [-1, 0, 777, 65534, 65535]       # -1 <= B <= 65535


def sat_i32(y):
    """v_cvt_i32_f64 of an integral finite double: the value, saturated to the int32 range"""
    return np.clip(y, float(I32_MIN), float(I32_MAX)).astype(np.int64)


def grid():
    k = np.arange(-3, 65540, dtype=np.float64)
    around = [k, np.nextafter(k, -np.inf), np.nextafter(k, np.inf), k + 0.5, k + 0.25, k - 1e-9]
    edges = []
    for e in (float(I32_MIN), float(I32_MAX), 2.0 ** 31, 2.0 ** 32, 2.0 ** 53, 2.0 ** 63):
        for s in (1.0, -1.0):
            v = s * e
            edges += [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf), v - 0.5, v + 0.5, v - 1.0, v + 1.0]
    far = [1e300, -1e300, 1e10, -1e10, 1.7e308, -1.7e308, 0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300]
    rng = np.random.default_rng(3)
    rnd = np.concatenate([rng.uniform(-70000, 140000, 50000), rng.normal(0, 1e6, 20000),
                          (rng.integers(-70000, 140000, 20000) + rng.choice([-1, 1], 20000) * 2.0 ** -rng.integers(1, 52, 20000))])
    x = np.concatenate(around + [np.array(edges + far), rnd])
    assert np.isfinite(x).all()
    return x


X = grid()


def old_ceil_max(x, A):
    y = np.where(x > 0.0, x, 0.0)
    y = np.where(y > 65536.0, 65536.0, y)
    return np.maximum(np.ceil(y).astype(np.int64), A)


def old_floor_min(x, B):
    y = np.where(x < 65535.0, x, 65535.0)
    y = np.where(y < -1.0, -1.0, y)
    return np.minimum(np.floor(y).astype(np.int64), B)


def new_ceil_max(x, A):
    return np.maximum(np.minimum(sat_i32(np.ceil(x)), 65536), A)


def new_floor_min(x, B):
    return np.minimum(np.maximum(sat_i32(np.floor(x)), -1), B)


def test_ceil_form():
    for A in BOUNDS_A:
        assert np.array_equal(old_ceil_max(X, A), new_ceil_max(X, A)), A


def test_floor_form():
    for B in BOUNDS_B:
        assert np.array_equal(old_floor_min(X, B), new_floor_min(X, B)), B


def test_negated_axis_of_the_high_half():
    """amb0 from floor(-x) (the conversion saturates at the other end for |x| >= 2^31), and the
    comparisons and the query value the kernel derives from e = -amb0"""
    for A in BOUNDS_A:
        e = np.minimum(np.maximum(sat_i32(np.floor(-X)), -65536), -A)
        amb0 = old_ceil_max(X, A)
        assert np.array_equal(-e, amb0), A
        assert np.array_equal(~e, amb0 - 1)
        for bt in BOUNDS_B:
            assert np.array_equal(-bt <= e, amb0 <= bt)


def test_negation_commutes_with_the_rounded_difference():
    rng = np.random.default_rng(5)
    bhi = np.concatenate([rng.uniform(-1e5, 2e5, 100000), rng.normal(0, 1e9, 1000), X[:100000]])
    tol = np.abs(bhi) * 1e-13 * rng.uniform(0.5, 4.0, bhi.size) + rng.choice([0.0, 1e-13, 2.0 ** -40], bhi.size)
    assert np.array_equal(tol - bhi, -(bhi - tol))
    assert np.array_equal(np.floor(tol - bhi), -np.ceil(bhi - tol))
