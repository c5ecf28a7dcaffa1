"""numpy restatement of the QuickSync search (pcps_quicksync_acquisition_cc.cc:178-201, 204-245, 315-527) on complex64 input:
the yardstick of tests/test_quicksync_gpu.py.  float32 wipe-off with the oracle's running phase (oracle.sincos), float32 products
and sums in the fold (i ascending), float64 transforms (oracle.fft).  Two deviations from the block, both the engine's: the
candidate accumulators start at zero (the block never initialises `complex_acumulator[100]`, :442) and a candidate correlation
stops at the end of the block of L samples (the block reads on; that only happens for f = 1)."""
import numpy as np

TWO_PI = 6.283185307179586  # GPS_TWO_PI


def doppler_bins(doppler_max, doppler_step, n_bins=0):
    """init() (:219-231): a step of 0 means 250; every bin <= +doppler_max counts (inclusive grid).  n_bins > 0 overrides the count."""
    step = doppler_step if doppler_step else 250
    count = n_bins if n_bins > 0 else len(range(-int(doppler_max), int(doppler_max) + 1, step))
    return [-int(doppler_max) + step * b for b in range(count)]


def wipeoffs(oracle, fs, bins, L):
    """d_grid_doppler_wipeoffs (:235-243): phase step -(float)(GPS_TWO_PI * doppler / (float)fs), running float32 phase from 0."""
    rows = []
    for d in bins:
        step = np.float32(TWO_PI * d / float(np.float32(fs)))
        rows.append(oracle.sincos(float(-step), L))
    return rows


def fold(v, M, terms):
    """std::plus chain of :190-195 / :389-396: pieces of M samples added in complex64, first piece first, onto zeros."""
    acc = np.zeros(M, np.complex64)
    for i in range(terms):
        acc = (acc + v[i * M:(i + 1) * M]).astype(np.complex64)
    return acc


class Result:
    pass


def search(oracle, x, codes, fs, N, f, doppler_max, doppler_step, n_bins=0):
    """One dwell for every code in `codes` (one period of N samples each).  Returns a list of Result with grid [bins][M] (float64),
    row_max [(value, index)], indext, doppler_index, doppler_hz, mag, input_power, test_statistics, possible_delay, corr_output_f,
    acq_delay_samples."""
    M, L = N // f, f * N
    x = np.ascontiguousarray(x[:L], np.complex64)
    bins = doppler_bins(doppler_max, doppler_step, n_bins)
    w = wipeoffs(oracle, fs, bins, L)
    power = float(np.mean(np.abs(x.astype(np.complex128)) ** 2))
    wiped = [(x * wb).astype(np.complex64) for wb in w]
    X = [oracle.fft(fold(xb, M, f * f)) for xb in wiped]
    out = []
    for c in codes:
        c = np.ascontiguousarray(c[:N], np.complex64)
        C = np.conj(oracle.fft(fold(c, M, f)))
        grid = np.stack([np.abs(oracle.fft(Xb * C, inverse=True)) ** 2 for Xb in X])
        r = Result()
        r.grid = grid
        r.row_max = [(float(row.max()), int(np.argmax(row))) for row in grid]
        b, k = np.unravel_index(int(np.argmax(grid)), grid.shape)  # first maximum, bins then samples ascending
        r.doppler_index, r.indext = int(b), int(k)
        r.doppler_hz = bins[r.doppler_index]
        r.mag = float(grid[b, k])
        r.input_power = power
        r.test_statistics = r.mag / float(M) ** 4 / power
        r.possible_delay = [r.indext + i * M for i in range(f)]
        vals = []
        for p in r.possible_delay:
            n = min(N, L - p)
            a = np.sum(wiped[b][p:p + n].astype(np.complex128) * c[:n].astype(np.complex128))  # plain product: the code is not conjugated (:462)
            vals.append(float(abs(a) ** 2))
        r.corr_output_f = vals
        r.acq_delay_samples = r.possible_delay[int(np.argmax(vals))]
        out.append(r)
    return out
