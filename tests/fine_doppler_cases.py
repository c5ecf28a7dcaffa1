"""Seeded synthetic inputs of the fine Doppler tests, and the comparisons they share.

A block holds SIX satellites at once -- random codes, one delay and one tone each -- so that one call of six requests covers the
delays {0, 1, 2, N/3, N/3 + 7, N - 1} and the coarse values {0, 500, +-2500, +-4500}: the windows of 0 and 500 straddle index 0 of
the spectrum.  Every tone lies on a fine bin inside its request's window and away from the window's ends (its neighbour is then 5 %
down at Z = 8 before noise).  Seeds are chosen on the restatement alone: tests/test_fine_doppler_ref.py asserts that every case of
MATRIX, and the N = 25000 block, has a top-two margin of at least MARGIN of the peak in every window, 10 x the engine's parity gate TOL, so that no comparison
of a bin rests on a near tie."""
import collections

import numpy as np

import fine_doppler_ref as ref

TOL = 1e-4     # |p - p_ref| <= TOL * the window's peak; |mean - mean_ref| <= TOL * mean_ref
MARGIN = 1e-3  # the restatement's top-two margin that every case must have
SIGMA = 0.5    # noise per component; every satellite has amplitude 1
COARSE = (0.0, 500.0, 2500.0, -2500.0, 4500.0, -4500.0)
SIZES = (2000, 4000, 6625)
PZ = ((1, 1), (4, 2), (10, 8))
ALIGNMENTS = (ref.REFERENCE, ref.EXACT)
# every size with every (P, Z) whose Next = P N Z is even: 6625 x 1 x 1 is odd, which the engine refuses
MATRIX = tuple((N, P, Z) for N in SIZES for P, Z in PZ if (N * P * Z) % 2 == 0)
# (N, P, Z) -> seed
SEEDS = {(2000, 1, 1): 1, (2000, 4, 2): 1, (2000, 10, 8): 1, (4000, 1, 1): 1, (4000, 4, 2): 1, (4000, 10, 8): 1, (6625, 4, 2): 1, (6625, 10, 8): 1,
    (25000, 10, 8): 1}

Block = collections.namedtuple("Block", "N fs P Z x codes requests tones")


def delays(N):
    return (0, 1, N // 3, N - 1, N // 3 + 7, 2)


def make_codes(N, n, rng):
    """n codes of 1023 random chips sampled N times; every other one complex ((+-1 +- j) / sqrt 2).  The block multiplies by the
    code itself, so a satellite's signal carries the conjugate."""
    idx = (np.arange(N) * 1023) // N
    out = []
    for i in range(n):
        c = (rng.integers(0, 2, 1023) * 2 - 1).astype(np.float64)
        if i % 2:
            c = (c + 1j * (rng.integers(0, 2, 1023) * 2 - 1)) / np.sqrt(2.0)
        out.append(c[idx].astype(np.complex64))
    return out


def block(N, P, Z, seed=None, n_sats=6, extra=0):
    """P N + extra samples of n_sats satellites in noise; requests[i] = (slot i, delay, coarse)."""
    fs = N * 1000
    rng = np.random.Generator(np.random.PCG64(SEEDS[(N, P, Z)] if seed is None else seed))
    next_size = P * N * Z
    table = ref.freq_table(fs, next_size)
    codes = make_codes(N, n_sats, rng)
    n = np.arange(P * N + extra)
    x = SIGMA * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
    requests, tones = [], []
    for i in range(n_sats):
        s, coarse = delays(N)[i], COARSE[i]
        first, count = ref.window(fs, next_size, coarse, 1000.0, table)
        at = count // 2 + int(rng.integers(-(count // 4), count // 4 + 1))
        k = (first + at) % next_size
        kk = k if k < next_size // 2 else k - next_size
        x = x + np.conj(codes[i])[(n - s) % N] * np.exp(2j * np.pi * ((kk * n) % next_size) / next_size + 1j * rng.uniform(0, 2 * np.pi))
        requests.append((i, s, coarse))
        tones.append(k)
    return Block(N, fs, P, Z, x.astype(np.complex64), codes, requests, tones)


def quantise(x, iq_format_bits):
    """The block as int16 / int8 [n, 2] and the complex64 values those integers are."""
    scale, dt = (12.0, np.int8) if iq_format_bits == 8 else (1500.0, np.int16)
    lim = np.iinfo(dt).max
    q = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -lim, lim).astype(dt)
    return q, (q[:, 0].astype(np.float32) + 1j * q[:, 1].astype(np.float32)).astype(np.complex64)


_REF = {}


def records(blk, alignment, key=None, x=None):
    """The restatement's record of every request of the block (computed once per key, read-only)."""
    key = (blk.N, blk.P, blk.Z, alignment, key)
    if key not in _REF:
        table = ref.freq_table(blk.fs, blk.P * blk.N * blk.Z)
        xs = blk.x if x is None else x
        recs = [ref.refine(xs, blk.codes[slot], blk.fs, blk.N, blk.P, blk.Z, s, coarse, 1000.0, alignment, table) for slot, s, coarse in blk.requests]
        for r in recs:
            r.p_window.setflags(write=False)
        _REF[key] = recs
    return _REF[key]


def f32_bits(v):
    return np.float32(v).tobytes()


def check(res, p_gpu, rec, next_size):
    """One result of the engine and its spectrum against the restatement's record.  Prints every figure before it asserts."""
    err = float(np.max(np.abs(p_gpu.astype(np.float64) - rec.p_window)) / rec.peak) if rec.peak > 0 else float(np.max(np.abs(p_gpu)))
    perr = abs(res.peak - rec.peak) / rec.peak if rec.peak > 0 else abs(res.peak)
    merr = abs(res.mean - rec.mean) / rec.mean if rec.mean > 0 else abs(res.mean)
    print("bin %d (ref %d) window (%d, %d) margin %.3g  spectrum err %.3g  peak err %.3g  mean err %.3g  status %d" % (res.bin, rec.bin,
        res.window_first_bin, res.window_bins, rec.margin, err, perr, merr, res.status))
    assert rec.margin >= MARGIN
    assert (res.window_first_bin, res.window_bins) == (rec.window_first_bin, rec.window_bins)
    assert p_gpu.size == rec.window_bins
    assert res.bin == rec.bin
    assert f32_bits(res.doppler_hz) == f32_bits(rec.doppler_hz) and float(np.float32(res.doppler_hz)) == res.doppler_hz
    assert err <= TOL and perr <= TOL and merr <= TOL
    assert res.status == rec.status
    assert f32_bits(res.peak) == f32_bits(p_gpu[(res.bin - res.window_first_bin) % next_size])
    assert np.all(np.isfinite(p_gpu)) and np.isfinite(res.peak) and np.isfinite(res.mean)


def result_bits(r):
    return (np.float64(r.doppler_hz).tobytes(), r.bin, r.status, np.float32(r.peak).tobytes(), np.float32(r.mean).tobytes(), r.window_first_bin,
        r.window_bins)
