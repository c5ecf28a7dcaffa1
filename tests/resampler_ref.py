"""CPU restatement of the ring resampler (include/gnsscorr.h, gc_ring_resampler_*): exact integers for the index arithmetic, float64
for the polyphase filter.  Test infrastructure only.  With M = 2^32:

    direct, fs_in > fs_out    step = floor(M fs_out / fs_in)    n_m = ceil(m M / step)         outputs(H) = floor((H - 1) step / M) + 1
    direct, fs_in < fs_out    step = floor(M fs_in / fs_out)    n_m = floor((m + 1) step / M)  outputs(H) = ceil(H M / step) - 1
    direct, fs_in == fs_out   n_m = m                                                          outputs(H) = H
    polyphase                 INC = round(fs_in / fs_out * M)   n_m = (m INC) >> 32            outputs(H) = ceil(H M / INC)
                              p_m = ((m INC) & (M - 1)) >> (32 - log2 P)
                              y[m] = sum_k H[p_m][k] x[n_m - k],  x[n] = 0 for n < 0
"""
import math

import numpy as np

from conditioner_ref import to_complex

M = 1 << 32
IDENTITY, DOWN, UP, POLY = range(4)


def direct_ratio(fs_in, fs_out):
    """(kind, step) of direct mode."""
    if fs_in == fs_out:
        return IDENTITY, 0
    if fs_in > fs_out:
        return DOWN, int(math.floor(4294967296.0 * fs_out / fs_in))
    return UP, int(math.floor(4294967296.0 * fs_in / fs_out))


def poly_ratio(fs_in, fs_out):
    return POLY, int(round(fs_in / fs_out * 4294967296.0))


def available(kind, step, head):
    """Outputs whose source sample lies below the source head."""
    if head == 0:
        return 0
    if kind == DOWN:
        return ((head - 1) * step) // M + 1
    if kind == UP:
        return -((-head * M) // step) - 1
    if kind == POLY:
        return -((-head * M) // step)
    return head


def source_index(kind, step, m):
    """n_m for the output numbers m (array of Python-exact integers in, int64 out)."""
    m = [int(v) for v in np.atleast_1d(m)]
    if kind == DOWN:
        n = [-((-v * M) // step) for v in m]
    elif kind == UP:
        n = [((v + 1) * step) // M for v in m]
    elif kind == POLY:
        n = [(v * step) // M for v in m]
    else:
        n = m
    return np.array(n, np.int64)


def phase_index(step, phases, m):
    log2p = int(phases).bit_length() - 1
    return np.array([((int(v) * step) & (M - 1)) >> (32 - log2p) for v in np.atleast_1d(m)], np.int64)


def direct(raw, fs_in, fs_out, head=None):
    """Every output of direct mode the first `head` samples of `raw` complete (all of raw by default): raw[n_m], bits as they are."""
    raw = np.asarray(raw)
    kind, step = direct_ratio(fs_in, fs_out)
    n_out = available(kind, step, len(raw) if head is None else head)
    return raw[source_index(kind, step, np.arange(n_out))]


def polyphase(raw, bank, fs_in, fs_out, head=None):
    """Every output of polyphase mode the first `head` samples of `raw` complete (complex128)."""
    x = to_complex(raw)
    H = np.asarray(bank, np.float64)
    P, T = H.shape
    kind, inc = poly_ratio(fs_in, fs_out)
    n_out = available(kind, inc, len(x) if head is None else head)
    m = np.arange(n_out)
    n = source_index(kind, inc, m)
    p = phase_index(inc, P, m)
    z = np.concatenate([np.zeros(T - 1, np.complex128), x])  # z[i] = x[i - (T - 1)]
    y = np.zeros(n_out, np.complex128)
    for k in range(T):
        y += H[p, k] * z[n - k + (T - 1)]
    return y


def first_output(kind, step, origin, taps=1):
    """The first output m whose whole window -- source samples n_m - (taps - 1) .. n_m -- lies at or above `origin`: as many
    outputs as have their source sample below origin + taps - 1 come before it.  Python integers."""
    return available(kind, step, int(origin) + int(taps) - 1)


def _exact_source_index(kind, step, m):
    """n_m as Python integers, for output numbers of any size."""
    if kind == DOWN:
        return [-((-v * M) // step) for v in m]
    if kind == UP:
        return [((v + 1) * step) // M for v in m]
    if kind == POLY:
        return [(v * step) // M for v in m]
    return list(m)


def direct_from(origin, samples, fs_in, fs_out, head=None):
    """Direct mode on a source whose first sample `samples[0]` has the absolute number `origin`: (m0, outputs) with m0 the first
    output whose source sample lies at or above the origin and outputs[j] = sample number n_{m0 + j}, for every output the source
    samples below `head` (an absolute number; all of `samples` by default) complete.  Index arithmetic in Python integers."""
    samples = np.asarray(samples)
    origin = int(origin)
    kind, step = direct_ratio(fs_in, fs_out)
    head = origin + len(samples) if head is None else int(head)
    m0 = first_output(kind, step, origin)
    m1 = max(m0, available(kind, step, head))
    n = _exact_source_index(kind, step, range(m0, m1))
    assert all(origin <= v < head for v in n)
    return m0, samples[np.array([v - origin for v in n], np.int64)]


def polyphase_from(origin, samples, bank, fs_in, fs_out, head=None):
    """Polyphase mode on a source that starts at the absolute number `origin`: (m0, outputs as complex128) from the first output
    whose whole window of T samples lies at or above the origin on; nothing in front of the origin is read."""
    x = to_complex(samples)
    H = np.asarray(bank, np.float64)
    P, T = H.shape
    log2p = int(P).bit_length() - 1
    origin = int(origin)
    kind, inc = poly_ratio(fs_in, fs_out)
    head = origin + len(x) if head is None else int(head)
    m0 = first_output(kind, inc, origin, T)
    m1 = max(m0, available(kind, inc, head))
    ms = range(m0, m1)
    n = _exact_source_index(kind, inc, ms)
    assert all(origin + T - 1 <= v < head for v in n)
    rel = np.array([v - origin for v in n], np.int64)
    p = np.array([((v * inc) & (M - 1)) >> (32 - log2p) for v in ms], np.int64)
    y = np.zeros(len(rel), np.complex128)
    for k in range(T):
        y += H[p, k] * x[rel - k]
    return m0, y


def error_bound(bank, raw):
    """(T + 16) 2^-23 max_p sum_k |H[p][k]| max|x|: one float32 rounding per product and per sum over the worst phase row."""
    H = np.abs(np.asarray(bank, np.float64))
    return (H.shape[1] + 16) * 2.0 ** -23 * H.sum(axis=1).max() * np.abs(to_complex(raw)).max()
