"""CPU restatement of the signal conditioner (include/gnsscorr.h, gc_conditioner_*): float64 arithmetic with the same 64-bit
phase accumulator as the device kernel.  Test infrastructure only.

    y[m] = sum_k h[k] x[mD - k] exp(-j 2 pi phi(mD - k)),   phi(n) = ((n inc) mod 2^64) >> 32  [2^-32 turns],
    inc  = round(f / fs_in * 2^64) mod 2^64,   x[n] = 0 for n < 0
"""
import numpy as np


def phase_inc(translate_hz, fs_in):
    return int(round(float(translate_hz) / float(fs_in) * 2.0 ** 64)) % (1 << 64)


def to_complex(raw):
    """The plain cast of the data-type adapter: complex64 [n] stays, int16 / int8 [n, 2] becomes re + j im."""
    raw = np.asarray(raw)
    if np.iscomplexobj(raw):
        return raw.astype(np.complex128)
    return raw[:, 0].astype(np.float64) + 1j * raw[:, 1].astype(np.float64)


def mixer(n_first, n, translate_hz, fs_in):
    """exp(-j 2 pi phi(k)) for k = n_first .. n_first + n - 1 (complex128)."""
    inc = phase_inc(translate_hz, fs_in)
    if inc == 0:
        return np.ones(n, np.complex128)
    k = np.arange(n_first, n_first + n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        phi = (k * np.uint64(inc)) >> np.uint64(32)  # uint64 arithmetic wraps mod 2^64
    return np.exp(-2j * np.pi * (phi.astype(np.float64) / 2.0 ** 32))


def condition(raw, taps, decimation, translate_hz, fs_in, first_out=0, n_out=None):
    """Outputs y[first_out : first_out + n_out] (complex128) from the whole raw stream `raw` (sample 0 first)."""
    x = to_complex(raw)
    h = np.asarray(taps, np.float64)
    D, T = int(decimation), len(h)
    total = (len(x) + D - 1) // D
    if n_out is None:
        n_out = total - first_out
    assert first_out + n_out <= total
    z = x * mixer(0, len(x), translate_hz, fs_in)
    z = np.concatenate([np.zeros(T - 1, np.complex128), z])  # z[i] = mixed x[i - (T - 1)]
    m = np.arange(first_out, first_out + n_out)
    y = np.zeros(n_out, np.complex128)
    for k in range(T):
        y += h[k] * z[m * D - k + (T - 1)]
    return y


def decimate_from(origin, samples, taps, decimation, head=None):
    """The ring decimator (no mixer) on a source whose first sample `samples[0]` has the absolute number `origin`: (m0, y) with
    y[j] = sum_k h[k] x[(m0 + j) D - k] (complex128) for every output the source samples below `head` (an absolute number; all of
    `samples` by default) complete, from the first output m0 whose whole window lies at or above the origin on:
    m0 = ceil((origin + T - 1) / D).  Nothing in front of the origin is read.  Index arithmetic in Python integers."""
    x = to_complex(samples)
    h = np.asarray(taps, np.float64)
    D, T = int(decimation), len(h)
    origin = int(origin)
    head = origin + len(x) if head is None else int(head)
    m0 = -((-(origin + T - 1)) // D)
    m1 = max(m0, -((-head) // D))  # outputs m with m D < head
    rel = np.array([m * D - origin for m in range(m0, m1)], np.int64)
    assert rel.size == 0 or (rel[0] >= T - 1 and rel[-1] < len(x))
    y = np.zeros(len(rel), np.complex128)
    for k in range(T):
        y += h[k] * x[rel - k]
    return m0, y


def error_bound(taps, raw):
    """(T + 16) 2^-23 sum|h| max|x|: one float32 rounding per product and per sum, plus a few ulp for the mixer."""
    h = np.asarray(taps, np.float64)
    return (len(h) + 16) * 2.0 ** -23 * np.abs(h).sum() * np.abs(to_complex(raw)).max()


def fir_low_pass(gain, fs, cutoff_hz, transition_hz):
    """The formula gc_fir_low_pass states in the header, in float64."""
    n = int(53.0 * fs / (22.0 * transition_hz))
    n += 1 - (n & 1)
    M = (n - 1) // 2
    i = np.arange(n)
    k = (i - M).astype(np.float64)
    w0 = 2.0 * np.pi * cutoff_hz / fs
    win = 0.54 - 0.46 * np.cos(2.0 * np.pi * i / (n - 1)) if n > 1 else np.ones(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(k == 0, w0 / np.pi, np.sin(k * w0) / (k * np.pi))
    h = g * win
    return gain * h / h.sum()
