"""Numpy restatement of the fine Doppler stage of pcps_acquisition_fine_doppler_cc (estimate_Doppler, :400-479), steps 1 to 6 of the
block in complex128 with a zero-padded np.fft.fft and the block's float32 frequency table.  Test infrastructure only: the engine
(gnsscorr.FineDoppler) computes the bins of the acceptance window alone and is compared with what this computes for all of them."""
import collections

import numpy as np

REFERENCE, EXACT = "reference", "exact"
REFINED, EDGE = 1, 2

Record = collections.namedtuple("Record", "bin doppler_hz peak mean status window_first_bin window_bins p_window margin full_bin accepted acq_doppler_hz")


def std_rotate(seq, first, middle, last):
    """std::rotate(first, middle, last) on a list, literally: the element at `middle` becomes the one at `first`."""
    out = list(seq)
    out[first:last] = seq[middle:last] + seq[first:middle]
    return out


def replica_index_map(N, s, alignment):
    """src with r'[i] = code[src[i]].  reference: std::rotate(r, r + (N - s), r + N - 1) when s != 0 (:405-409); exact: (i - s) mod N."""
    i = np.arange(N)
    if alignment == EXACT:
        return (i - s) % N
    assert alignment == REFERENCE
    if s == 0:
        return i
    src = np.where(i < s - 1, N - s + i, i - (s - 1))
    src[N - 1] = N - 1
    return src


def freq_table(fs, next_size):
    """d_grid_doppler-style table of estimate_Doppler: float32 entries from double arithmetic on float32 operands."""
    k = np.arange(next_size)
    fsf, nf = np.float64(np.float32(fs)), np.float64(np.float32(next_size))
    lo = (fsf / 2.0 * np.float32(k).astype(np.float64)) / (nf / 2.0)
    hi = (-fsf / 2.0 * np.float32(next_size - k).astype(np.float64)) / (nf / 2.0)
    return np.where(k < next_size // 2, lo, hi).astype(np.float32)


def window(fs, next_size, coarse_hz, window_hz=1000.0, table=None):
    """(first_bin, bins): {k : |(double)f[k] - coarse| < window_hz} by brute force over the whole table, as one circular run in
    ascending frequency."""
    f = freq_table(fs, next_size) if table is None else table
    inside = np.abs(f.astype(np.float64) - float(coarse_hz)) < float(window_hz)
    count = int(inside.sum())
    if count == 0:
        return None, 0
    # the run starts at the member whose circular predecessor is no member
    starts = np.flatnonzero(inside & ~np.roll(inside, 1))
    assert len(starts) == 1, "the window is one circular run"
    first = int(starts[0])
    run = (first + np.arange(count)) % next_size
    assert inside[run].all()
    return first, count


def wiped(x, code, N, P, s, alignment):
    r = np.asarray(code, np.complex128)[replica_index_map(N, s, alignment)]
    return np.asarray(x[:P * N], np.complex128) * np.tile(r, P)


def spectrum(x, code, N, P, Z, s, alignment):
    """p[k] = |FFT_Next(y)|^2 over all Next = P N Z bins, and sum |y|^2."""
    y = wiped(x, code, N, P, s, alignment)
    Y = np.fft.fft(y, P * N * Z)
    return Y.real ** 2 + Y.imag ** 2, float(np.sum(y.real ** 2 + y.imag ** 2))


def refine(x, code, fs, N, P, Z, s, coarse_hz, window_hz=1000.0, alignment=REFERENCE, table=None):
    next_size = P * N * Z
    f = freq_table(fs, next_size) if table is None else table
    p, energy = spectrum(x, code, N, P, Z, s, alignment)
    first, count = window(fs, next_size, coarse_hz, window_hz, f)
    run = (first + np.arange(count)) % next_size
    pw = p[run]
    # the first maximum in array-index order
    ks = np.sort(run)
    k = int(ks[np.argmax(p[ks])])
    top = np.sort(pw)[::-1]
    margin = 1.0 if count == 1 or top[0] == 0 else float((top[0] - top[1]) / top[0])
    at = int(np.flatnonzero(run == k)[0])
    status = EDGE if at in (0, count - 1) else REFINED
    # the block itself: the maximum of the whole spectrum, accepted within 1 kHz of the coarse value (:445-470)
    full = int(np.argmax(p))
    accepted = bool(abs(float(f[full]) - float(coarse_hz)) < 1000.0)
    return Record(k, float(f[k]), float(p[k]), energy, status, first, count, pw, margin, full, accepted, float(f[full]) if accepted else float(coarse_hz))
