"""The numpy restatement of the dropout / gradient-noise generator (tests/dropout_restatement.py) meets the statistical
conditions by itself, on the CPU, so that the GPU tests can simply demand bit equality with it.

n = 2^21 mask elements at steps {0, 5, 7, 12345} x salts {1, 2, 3, 11, 90210, 0x6e6f697365} x p {0.05, 0.1, 0.2, 0.5}:
  * keep rate within 5 sigma of P = (65536 - thr) / 65536, sigma = sqrt(P (1 - P) / n); the same for each lane i % 4
  * |autocorrelation of the mask| <= 0.01 at lags 1, 2, 3, 4, 256, 1024 (lowbias32 on counter input reaches -0.0044 at
    lag 256 for p = 0.5, 6.4 sigma: a known, harmless weakness; a repeated or lane-shared mask has correlation 1)
  * |cross-correlation| <= 0.01 between two salts at one step and between two steps at one salt (every pair)
  * gradient noise at n = 2^20: the cosine half and the sine half each have mean, variance and fourth moment within
    5 sigma of N(0, 1)'s (sigma = sqrt(1 / m), sqrt(2 / m), sqrt(96 / m) over m = n / 2 samples), their product a mean
    within 5 sigma of 0"""
import itertools
import math

import numpy as np
import pytest

import dropout_restatement as dr

N = 1 << 21
STEPS = (0, 5, 7, 12345)
SALTS = (1, 2, 3, 11, 90210, 0x6e6f697365)
PS = (0.05, 0.1, 0.2, 0.5)
LAGS = (1, 2, 3, 4, 256, 1024)
CORR_CAP = 0.01
NSIGMA = 5.0


@pytest.fixture(scope="module")
def bits():
    """the 16 hash bits of every (step, salt) stream, computed once"""
    return {(st, sa): dr.keep_bits(st, sa, N) for st in STEPS for sa in SALTS}


def corr(a, b):
    """Pearson correlation of two boolean arrays, from counts"""
    pa, pb, pab = a.mean(), b.mean(), np.count_nonzero(a & b) / a.size
    return float((pab - pa * pb) / math.sqrt(pa * (1 - pa) * pb * (1 - pb)))


def test_seed_and_hash_known_values():
    """spot values worked by hand from the definition (python integers, no numpy): the 64-bit wrap, the high word of the
    pair index and the lane split"""
    def lowbias32(h):
        h ^= h >> 16
        h = (h * 0x7feb352d) & 0xffffffff
        h ^= h >> 15
        h = (h * 0x846ca68b) & 0xffffffff
        h ^= h >> 16
        return h
    assert dr.drop_seed(0, 0) == 0
    for step, salt in ((5, 11), (1 << 33, (1 << 40) + 3), ((1 << 64) - 1, 7)):
        seed = dr.drop_seed(step, salt)
        assert 0 <= seed < 1 << 32
        for q in (0, 1, 12345, (1 << 32) - 1, 1 << 32, (3 << 32) + 9):
            want = lowbias32((((q & 0xffffffff) ^ seed) + (q >> 32) * 0x9E3779B1) & 0xffffffff)
            assert int(dr.drop_pair(seed, q)) == want
    # the array form agrees with the scalar form, and the lanes are low half / high half of one hash
    seed = dr.drop_seed(5, 11)
    h = dr.drop_pair(seed, np.arange(8, dtype=np.uint64))
    b = dr.keep_bits(5, 11, 16)
    assert np.array_equal(b[0::2], h & np.uint32(0xffff)) and np.array_equal(b[1::2], h >> np.uint32(16))
    assert np.array_equal(dr.keep_bits(5, 11, 6, first=5), b[5:11])


def test_threshold_and_scale():
    assert dr.drop_thr16(0.0) == 0 and dr.drop_thr16(1.0) == 65536 and dr.drop_thr16(0.99999) == 65535
    assert dr.drop_thr16(0.5) == 32768 and dr.drop_thr16(3 / 65536) == 3 and dr.drop_thr16(0.1) == 6554
    assert dr.drop_inv(0) == np.float32(1.0) and dr.drop_inv(32768) == np.float32(2.0) and dr.drop_inv(65536) == 0.0
    assert dr.drop_inv(65535) == np.float32(65536.0)
    assert dr.keep_mask(5, 11, 1000, 0.0).all()


@pytest.mark.parametrize("p", PS)
def test_keep_rate(bits, p):
    thr = dr.drop_thr16(p)
    P = (65536 - thr) / 65536
    worst = 0.0
    for key, b in bits.items():
        keep = b >= thr
        z = (keep.mean() - P) / math.sqrt(P * (1 - P) / N)
        worst = max(worst, abs(z))
        assert abs(z) <= NSIGMA, f"keep rate of {key} p={p}: z = {z:.2f}"
        for lane in range(4):
            kl = keep[lane::4]
            zl = (kl.mean() - P) / math.sqrt(P * (1 - P) / kl.size)
            worst = max(worst, abs(zl))
            assert abs(zl) <= NSIGMA, f"keep rate of {key} p={p} lane {lane}: z = {zl:.2f}"
    print(f"[dropout-restatement] keep rate p={p}: worst |z| {worst:.2f}")


@pytest.mark.parametrize("p", PS)
def test_autocorrelation(bits, p):
    thr = dr.drop_thr16(p)
    worst = (0.0, None)
    for key, b in bits.items():
        keep = b >= thr
        for lag in LAGS:
            c = corr(keep[:-lag], keep[lag:])
            worst = max(worst, (abs(c), (key, lag)))
            assert abs(c) <= CORR_CAP, f"autocorrelation of {key} p={p} at lag {lag}: {c:.4f}"
    print(f"[dropout-restatement] autocorrelation p={p}: worst {worst[0]:.5f} at {worst[1]}")


@pytest.mark.parametrize("p", PS)
def test_cross_correlation(bits, p):
    thr = dr.drop_thr16(p)
    keep = {k: b >= thr for k, b in bits.items()}
    worst = 0.0
    for st in STEPS:
        for a, b in itertools.combinations(SALTS, 2):
            c = corr(keep[(st, a)], keep[(st, b)])
            worst = max(worst, abs(c))
            assert abs(c) <= CORR_CAP, f"salts {a}, {b} at step {st} p={p}: {c:.4f}"
    for sa in SALTS:
        for a, b in itertools.combinations(STEPS, 2):
            c = corr(keep[(a, sa)], keep[(b, sa)])
            worst = max(worst, abs(c))
            assert abs(c) <= CORR_CAP, f"steps {a}, {b} at salt {sa} p={p}: {c:.4f}"
    print(f"[dropout-restatement] cross-correlation p={p}: worst {worst:.5f}")


@pytest.mark.parametrize("step", STEPS)
def test_gradient_noise_moments(step):
    n = 1 << 20
    m = n // 2
    worst = 0.0
    for salt in SALTS:
        z = dr.gradient_noise(step, salt, n)
        assert z.shape == (n,) and np.isfinite(z).all()
        halves = {"cos": z[0::2], "sin": z[1::2]}
        for name, h in halves.items():
            stats = {"mean": (h.mean(), 0.0, math.sqrt(1 / m)), "variance": ((h * h).mean(), 1.0, math.sqrt(2 / m)),
                     "fourth moment": ((h ** 4).mean(), 3.0, math.sqrt(96 / m))}
            for what, (got, want, sigma) in stats.items():
                zz = (got - want) / sigma
                worst = max(worst, abs(zz))
                assert abs(zz) <= NSIGMA, f"{name} half {what} at step {step} salt {salt}: z = {zz:.2f}"
        zz = (halves["cos"] * halves["sin"]).mean() / math.sqrt(1 / m)
        worst = max(worst, abs(zz))
        assert abs(zz) <= NSIGMA, f"cos * sin mean at step {step} salt {salt}: z = {zz:.2f}"
    print(f"[dropout-restatement] gradient noise step {step}: worst |z| {worst:.2f}")


def test_gradient_noise_odd_length_is_a_prefix():
    z = dr.gradient_noise(7, 0x6e6f697365, 8)
    for n in (1, 2, 7):
        assert np.array_equal(dr.gradient_noise(7, 0x6e6f697365, n), z[:n])
