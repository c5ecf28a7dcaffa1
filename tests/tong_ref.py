"""numpy restatement of the Tong detector (pcps_tong_acquisition_cc.cc:185-227, :303-419) on complex64 input: the yardstick of
tests/test_tong_gpu.py.  float32 wipe-off with the oracle's running phase, float64 transforms (oracle.fft) and a float64 grid; the
decision step is the block's, with its float32 product threshold * dwell_count and its unsigned counter."""
import numpy as np

from quicksync_ref import doppler_bins, wipeoffs  # the same inclusive grid and the same wipe-off rows

RUNNING, POSITIVE, NEGATIVE = 0, 1, 2


class Dwell:
    """What one dwell leaves: grid [bins][N] (accumulated, normalised), row_max [(value, index)], mag (d_mag) and its cell (indext,
    doppler_index, doppler_hz, acq_delay_samples), input_power, dwell_count, q = mag / dwell_count, and -- when the search was given a
    threshold -- tong_count and state after this dwell."""


def step(state, tong_count, dwell_count, stat, threshold, max_val, max_dwells):
    """:393-415 for a running detector whose dwell_count has been advanced already (:316).  Returns (state, tong_count)."""
    if np.float32(stat) > np.float32(threshold) * np.float32(dwell_count):
        tong_count = (tong_count + 1) & 0xFFFFFFFF
        if tong_count == max_val:
            state = POSITIVE
    else:
        tong_count = (tong_count - 1) & 0xFFFFFFFF
        if tong_count == 0:
            state = NEGATIVE
    if dwell_count >= max_dwells:
        state = NEGATIVE
    return state, tong_count


def walk(q, threshold, init_val, max_val, max_dwells):
    """The detector on the statistics q[d] * (d + 1) of consecutive dwells: a list of (state, tong_count, dwell_count) per dwell, ending
    with the dwell that decides (or with the last q while it still runs)."""
    state, count, out = RUNNING, init_val, []
    for d, qd in enumerate(q, 1):
        state, count = step(state, count, d, np.float32(qd) * np.float32(d), threshold, max_val, max_dwells)
        out.append((state, count, d))
        if state != RUNNING:
            break
    return out


def search(oracle, x, codes, fs, N, doppler_max, doppler_step, n_dwells, samples_per_code=None, n_bins=0, threshold=None, tong=(1, 2, 3)):
    """n_dwells consecutive blocks of N samples of x for every code in `codes` (N samples each).  Returns a list (per code) of lists
    (per dwell) of Dwell.  The grid goes on accumulating whatever the state: a caller reads a satellite's records up to its deciding
    dwell."""
    spc = int(samples_per_code if samples_per_code is not None else N)
    bins = doppler_bins(doppler_max, doppler_step, n_bins)
    w = wipeoffs(oracle, fs, bins, N)
    fnf = np.float32(N) * np.float32(N)
    X, power = [], []
    for d in range(n_dwells):
        xb = np.ascontiguousarray(x[d * N:(d + 1) * N], np.complex64)
        assert xb.size == N
        power.append(float(np.mean(np.abs(xb.astype(np.complex128)) ** 2)))
        X.append([oracle.fft((xb * wb).astype(np.complex64)) for wb in w])
    out = []
    for c in codes:
        C = np.conj(oracle.fft(np.ascontiguousarray(c[:N], np.complex64)))
        grid = np.zeros((len(bins), N))
        recs, last = [], (0, 0, bins[0] * 0, 0)
        state, count = RUNNING, tong[0]
        for d in range(n_dwells):
            with np.errstate(divide="ignore", invalid="ignore"):
                s = 1.0 / (float(fnf * fnf) * power[d])
                grid = grid + np.stack([np.abs(oracle.fft(Xb * C, inverse=True)) ** 2 * s for Xb in X[d]])
            r = Dwell()
            r.grid = grid.copy()
            r.row_max = []
            mag, cell = 0.0, None
            for b, row in enumerate(grid):
                if np.all(np.isnan(row)):
                    r.row_max.append((float("nan"), 0))
                    continue
                k = int(np.nanargmax(row))  # the first maximum; NaN never wins a comparison
                r.row_max.append((float(row[k]), k))
                if mag < row[k]:
                    mag, cell = float(row[k]), (k, b)
            if cell is not None:
                last = (cell[0], cell[1], bins[cell[1]], cell[0] % spc)
            r.indext, r.doppler_index, r.doppler_hz, r.acq_delay_samples = last
            r.mag = mag
            r.input_power = power[d]
            r.dwell_count = d + 1
            r.q = mag / (d + 1)
            if threshold is not None:
                if state == RUNNING:
                    state, count = step(state, count, d + 1, mag, threshold, tong[1], tong[2])
                r.state, r.tong_count = state, count
            recs.append(r)
        out.append(recs)
    return out


def place_threshold(qs, lo_ratio=1.05):
    """A threshold in the geometric middle of the widest gap between the sorted positive statistics `qs` (any iterable): returns
    (threshold, ratio of the gap).  The caller asserts the ratio it needs."""
    v = sorted(float(q) for q in qs if q > 0)
    best = max(range(len(v) - 1), key=lambda i: v[i + 1] / v[i])
    return float(np.sqrt(v[best] * v[best + 1])), v[best + 1] / v[best]
