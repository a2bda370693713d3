"""The budget rule's restatement (tests/budget_spec.py) held to what the header states about it, on random states and on
hand-made ones.  No GPU."""
import numpy as np
import pytest

import budget_spec as BS
import sampling_spec as SS

F = np.float32
ROWS, W = 9, 37


def random_state(seed, kmax, nan=False):
    """sums of n samples of random colours per pixel (some pixels black, some finished, some below two samples)"""
    r = np.random.default_rng(seed)
    n = r.integers(0, kmax + 1, (ROWS, W))
    n[r.uniform(size=n.shape) < 0.15] = kmax
    s = (r.uniform(0, 2, (kmax, ROWS, W, 3)) * (r.uniform(size=(1, ROWS, W, 1)) < 0.8)).astype(F)
    sums = np.zeros((ROWS, W, 4), F)
    for k in range(kmax):
        m = n > k
        sums[m] = SS.fold(s[k][m][None], sums[m])
    if nan:
        sums[1, 3] = [np.nan, 1, 1, 2]
        sums[2, 5] = [np.inf, 1, 1, np.inf]
        sums[3, 7] = [1, 1, 1, np.nan]
    return sums, n


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("threshold,radius,min_samples", [(0.5, 1, 8), (0.05, 0, 2), (0.0, 3, 4), (2.0, 2, 8)])
def test_a_budget_is_non_zero_exactly_where_select_selects(seed, threshold, radius, min_samples):
    kmax = 16
    sums, n = random_state(seed, kmax, nan=seed % 2 == 1)
    for B, max_step in ((16, 0), (4, 0), (8, 3), (1, 0)):
        b = BS.budget(sums, n, kmax, B, threshold, 0.05, min_samples, radius, max_step)
        sel = SS.select(sums, n, kmax, threshold, 0.05, min_samples, radius)
        assert b.dtype == np.uint32 and np.array_equal(b != 0, sel == 1)
        cap = BS.cap_of(B, max_step)
        assert (b <= cap).all() and (b.astype(np.int64) <= kmax - np.minimum(n, kmax)).all()
        few = (n < min_samples) & (n < kmax)
        assert np.array_equal(b[few], np.minimum(np.minimum(min_samples - n[few], cap), kmax - n[few]))


def one_pixel(l_values, kmax=1 << 20):
    """a 1 x 1 state whose samples are the grey values l (luminance of (l, l, l) is l up to rounding)"""
    s = np.repeat(np.asarray(l_values, F)[:, None, None, None], 3, axis=3)
    return SS.fold(s), np.full((1, 1), len(l_values))


def test_an_error_of_exactly_the_threshold_gives_zero():
    sums, n = one_pixel([0.0, 1.0] * 8)
    e, _ = SS.error_variance(sums, n, 0.05)
    thr = float(e[0, 0])
    assert thr > 0
    assert BS.budget(sums, n, 1 << 20, 64, thr, 0.05, 8, 0)[0, 0] == 0
    below = float(np.nextafter(e[0, 0], F(0)))
    assert BS.budget(sums, n, 1 << 20, 64, below, 0.05, 8, 0)[0, 0] >= 1


def test_twice_the_threshold_asks_for_three_times_the_samples():
    sums, n = one_pixel([0.0, 1.0] * 8)  # n = 16
    e, _ = SS.error_variance(sums, n, 0.05)
    thr = float(e[0, 0] / F(2))  # (a division by two is exact: r = 2, t = 4 n, d = 3 n = 48)
    assert BS.budget(sums, n, 1 << 20, 64, thr, 0.05, 8, 0)[0, 0] == 48
    assert BS.budget(sums, n, 1 << 20, 32, thr, 0.05, 8, 0)[0, 0] == 32            # clamped by cap = B
    assert BS.budget(sums, n, 1 << 20, 64, thr, 0.05, 8, 0, max_step=5)[0, 0] == 5  # by cap = max_step
    assert BS.budget(sums, n, 1 << 20, 64, thr, 0.05, 8, 0, max_step=100)[0, 0] == 48  # max_step above B: B
    assert BS.budget(sums, n, 16 + 7, 64, thr, 0.05, 8, 0)[0, 0] == 7              # by kmax - n
    assert BS.budget(sums, n, 16, 64, thr, 0.05, 8, 0)[0, 0] == 0                  # finished


def test_nan_and_inf_sums():
    kmax, n = 64, np.full((1, 3), 16)
    sums = np.zeros((1, 3, 4), F)
    sums[0, 0] = [np.nan, 1, 1, 4]      # m1 NaN: v NaN -> 0, var 0, e = 0 / NaN = NaN: never wins
    sums[0, 1] = [8, 8, 8, np.inf]      # m2 inf: e = inf, r = inf, d = inf: cap
    sums[0, 2] = [8, 8, 8, 4]           # m1 = .5, m2 / n = .25: v = 0, e = 0
    b = BS.budget(sums, n, kmax, 8, 0.5, 0.05, 8, 0)
    assert b.tolist() == [[0, 8, 0]]
    # ... and within a window the NaN does not hide its neighbour's inf, nor select on its own
    b = BS.budget(sums, n, kmax, 8, 0.5, 0.05, 8, 1)
    assert b.tolist() == [[8, 8, 8]]
    only_nan = sums[:, :1].repeat(3, axis=1)
    assert not BS.budget(only_nan, n, kmax, 8, 0.5, 0.05, 8, 1).any()
    # a pixel with an inf sum: m1 inf, v = inf - inf = NaN -> 0, e = 0 / inf = 0
    sums[0, 1] = [np.inf, 8, 8, np.inf]
    assert BS.budget(sums, n, kmax, 8, 0.5, 0.05, 8, 0).tolist() == [[0, 0, 0]]


def test_a_zero_threshold_gives_the_cap_wherever_there_is_any_error():
    sums, n = one_pixel([0.0, 1.0] * 8)
    assert BS.budget(sums, n, 1 << 20, 64, 0.0, 0.05, 8, 0)[0, 0] == 64
    assert BS.budget(sums, n, 1 << 20, 64, 0.0, 0.05, 8, 0, max_step=3)[0, 0] == 3
    flat, n = one_pixel([0.5] * 16)  # no error at all: E = 0 is not above 0
    assert BS.budget(flat, n, 1 << 20, 64, 0.0, 0.05, 8, 0)[0, 0] == 0


def test_a_neighbour_without_an_estimate_asks_for_the_cap():
    """n < 2 next door is e = FLT_MAX: t overflows to inf"""
    sums, n = np.zeros((1, 2, 4), F), np.array([[16, 1]])
    sums[0, 0] = [8, 8, 8, 4]
    b = BS.budget(sums, n, 64, 8, 0.5, 0.05, 2, 1)
    assert b.tolist() == [[8, 1]]


def test_a_budgeted_step_folds_each_pixels_next_samples_in_order():
    kmax, B = 16, 8
    r = np.random.default_rng(3)
    samples = r.uniform(0, 2, (kmax, ROWS, W, 4)).astype(F)
    n0 = r.integers(0, kmax + 1, (ROWS, W))
    sums0 = np.zeros((ROWS, W, 4), F)
    for y in range(ROWS):
        for x in range(W):
            if n0[y, x]:
                sums0[y, x] = SS.fold(samples[:n0[y, x], y, x, :3][:, None])[0]
    budgets = r.choice([0, 0, 1, 2, 7, 8, 9, 1000], (ROWS, W))
    sums, n, take = BS.step(sums0, n0, budgets, kmax, B, samples)
    assert np.array_equal(take, np.where(n0 < kmax, np.minimum(np.minimum(budgets, B), kmax - n0), 0))
    assert np.array_equal(n, n0 + take) and (n <= kmax).all()
    for y in range(ROWS):
        for x in range(W):
            want = SS.fold(samples[:n[y, x], y, x, :3][:, None])[0] if n[y, x] else np.zeros(4, F)
            assert np.array_equal(sums[y, x].view(np.uint32), want.view(np.uint32))
    still = take == 0
    assert np.array_equal(sums[still].view(np.uint32), sums0[still].view(np.uint32))
    plain, _, _ = BS.step(sums0, n0, budgets, kmax, B, samples, moments=False)
    assert np.array_equal(plain[..., :3].view(np.uint32), sums[..., :3].view(np.uint32))
    assert np.array_equal(plain[..., 3].view(np.uint32), sums0[..., 3].view(np.uint32))
