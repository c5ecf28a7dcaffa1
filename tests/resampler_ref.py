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


def error_bound(bank, raw):
    """(T + 16) 2^-23 max_p sum_k |H[p][k]| max|x|: one float32 rounding per product and per sum over the worst phase row."""
    H = np.abs(np.asarray(bank, np.float64))
    return (H.shape[1] + 16) * 2.0 ** -23 * H.sum(axis=1).max() * np.abs(to_complex(raw)).max()
