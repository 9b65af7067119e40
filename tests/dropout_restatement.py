"""The counter-based dropout generator of csrc/common.h (eamd_drop_seed / eamd_drop_pair / eamd_drop_thr16 /
eamd_drop_inv / eamd_drop_keep) and the Box-Muller pair of csrc/optim.hip's grad_noise_kernel, restated in numpy: the
yardstick of eamd_dropout, of every fused dropout epilogue that takes eamd_dropout as its reference, and of
eamd_add_gradient_noise.  Test infrastructure only - the product tree never imports it, and no GPU is involved.

    seed    = fold32(murmur3 finaliser(step * 0x9E3779B97F4A7C15 + salt * 0xD1B54A32D192ED03))        (64-bit, wrapping)
    pair(q) = lowbias32(((uint32)q ^ seed) + (uint32)(q >> 32) * 0x9E3779B1)                          (32-bit, wrapping)
    element 2q takes the low 16 bits of pair(q), element 2q + 1 the high 16 bits; kept <=> bits >= thr,
    thr = min(floor(fp32(p * 65536 + 0.5)), 65535), survivors are scaled by fp32(65536 / (65536 - thr))."""
import numpy as np

M64 = (1 << 64) - 1
U32 = np.uint32
NOISE_SALT_XOR = 0x5bd1e995          # grad_noise_kernel's second seed: salt ^ this
TWO_M32 = np.float32(2.3283064365386963e-10)


def drop_seed(step, salt):
    """eamd_drop_seed: (device step counter, site salt) -> 32-bit launch seed.  Python ints, 64-bit wrapping."""
    x = ((int(step) & M64) * 0x9E3779B97F4A7C15 + (int(salt) & M64) * 0xD1B54A32D192ED03) & M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return (x ^ (x >> 32)) & 0xffffffff


def drop_pair(seed, pair_idx):
    """eamd_drop_pair: lowbias32 over (uint32)idx ^ seed + (idx >> 32) * 0x9E3779B1.  pair_idx: int or uint64 array."""
    q = np.asarray(pair_idx, dtype=np.uint64)
    lo = (q & np.uint64(0xffffffff)).astype(U32)
    hi = (q >> np.uint64(32)).astype(U32)
    with np.errstate(over="ignore"):
        h = (lo ^ U32(seed)) + hi * U32(0x9E3779B1)
        h = h ^ (h >> U32(16))
        h = h * U32(0x7feb352d)
        h = h ^ (h >> U32(15))
        h = h * U32(0x846ca68b)
        h = h ^ (h >> U32(16))
    return h


def drop_thr16(p):
    """eamd_drop_thr16: the 16-bit threshold, evaluated in float32 as on the device"""
    p = np.float32(p)
    if p >= np.float32(1.0):
        return 65536
    t = np.float32(max(p, np.float32(0.0))) * np.float32(65536.0) + np.float32(0.5)
    return int(min(np.float32(t), np.float32(65535.0)))


def drop_inv(thr):
    """eamd_drop_inv: the survivors' scale as a float32"""
    if thr >= 65536:
        return np.float32(0.0)
    return np.float32(65536.0) / np.float32(65536 - thr)


def keep_bits(step, salt, n, first=0):
    """the 16 hash bits of elements first .. first + n - 1 (uint32 array)"""
    seed = drop_seed(step, salt)
    i = np.arange(first, first + n, dtype=np.uint64)
    h = drop_pair(seed, i >> np.uint64(1))
    return np.where((i & np.uint64(1)).astype(bool), h >> U32(16), h & U32(0xffff))


def keep_mask(step, salt, n, p):
    """bool[n]: element i survives eamd_dropout(p) at (step, salt)"""
    return keep_bits(step, salt, n) >= U32(drop_thr16(p))


def gradient_noise(step, salt, n):
    """float64[n]: the N(0, 1) draws eamd_add_gradient_noise adds (times sigma) at (step, salt).  Pair q gives element
    2q = r cos(2 pi u1) and element 2q + 1 = r sin(2 pi u1), r = sqrt(-2 log u0); u0 and u1 are formed in float32 exactly as
    the kernel forms them (so is the angle), the logarithm, cosine and sine are float64."""
    s0, s1 = drop_seed(step, salt), drop_seed(step, int(salt) ^ NOISE_SALT_XOR)
    q = np.arange((n + 1) // 2, dtype=np.uint64)
    h0, h1 = drop_pair(s0, q), drop_pair(s1, q)
    u0 = (h0.astype(np.float32) + np.float32(1.0)) * TWO_M32
    u1 = h1.astype(np.float32) * TWO_M32
    ang = (np.float32(6.283185307179586) * u1).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u0.astype(np.float64)))
    out = np.empty(2 * q.size, dtype=np.float64)
    out[0::2] = r * np.cos(ang)
    out[1::2] = r * np.sin(ang)
    return out[:n]
