"""Signals, restatements and the two preconditions of tests/test_tong_gpu.py, free of any GPU call so that seeds and thresholds are
chosen -- and checked -- on the restatement (tests/tong_ref.py) alone.  GPS L1 C/A at fs = 1000 N: a block is one code period of N
samples.  A restatement is computed once per case, shared and read-only."""
import numpy as np

import tong_ref

TOL = 1e-4  # tests/test_acquisition_gpu.py
DMAX, DSTEP = 1000, 500  # five bins, both ends included


def signal(oracle, N, prns, cn0_db_hz, n_blocks, seed):
    """sum of the PRNs at their C/N0 (random Doppler within +-900 Hz, delay and phase from `seed`) plus CN(0, 1) noise."""
    from helpers import synth_stream
    fs, n = N * 1000, n_blocks * N
    x = np.zeros(n, np.complex128)
    for i, (prn, cn0) in enumerate(zip(prns, cn0_db_hz)):
        xi, _ = synth_stream([oracle.gps_l1_ca_code(prn).astype(np.float32)], fs, n, seed=1000 * seed + i, cn0_db_hz=(cn0, cn0), doppler_max=900.0, noise=False)
        x += xi
    rng = np.random.Generator(np.random.PCG64(seed))
    x += (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    out = x.astype(np.complex64)
    out.setflags(write=False)
    return out


def codes(oracle, N, prns):
    return [oracle.gps_l1_ca_code_sampled(p, N * 1000)[:N] for p in prns]


def conf(N, dmax=DMAX, dstep=DSTEP, **kw):
    from test_acquisition_gpu import _conf
    return _conf(N * 1000, 1, 1, float(N), dmax, dstep, **kw)


def thresholds(recs_per_sat, min_ratio=1.05):
    """Every threshold the decision-margin condition allows: the geometric middle of each gap of ratio >= min_ratio between the sorted
    positive q_d of all satellites and dwells, as (threshold, ratio), lowest first."""
    v = sorted({float(r.q) for recs in recs_per_sat for r in recs if r.q > 0})
    return [(float(np.sqrt(a * b)), b / a) for a, b in zip(v, v[1:]) if b / a >= min_ratio]


def decision_margin(recs_per_sat, threshold):
    """Condition 1: the smallest relative distance of a q_d from the threshold (asserted >= 1e-2: the engine's mag may be 2 TOL off)."""
    return min(abs(float(r.q) - threshold) / threshold for recs in recs_per_sat for r in recs)


def top_cell_margin(rec):
    """Condition 2: (top cell - runner-up) / top cell of a dwell's grid; above 10 TOL the cell is compared exactly."""
    flat = rec.grid.ravel()
    flat = flat[~np.isnan(flat)]
    if flat.size < 2:
        return 0.0
    top2 = np.partition(flat, flat.size - 2)[-2:]
    return float((top2[1] - top2[0]) / top2[1]) if top2[1] > 0 else 0.0


def outcome(recs, threshold, tong):
    """(state, tong_count, dwell_count) per dwell of one satellite under `threshold`, ending with its deciding dwell."""
    return tong_ref.walk([r.q for r in recs], threshold, *tong)


def check_dwell(acq, sat, rec, status, result, want_status, bins, spc):
    """One satellite of an engine against the restatement's record of the same dwell: grid, row maxima, result, status."""
    grid = acq.grid(sat)
    peak = float(np.nanmax(rec.grid))
    assert grid.shape == rec.grid.shape
    err = float(np.max(np.abs(grid - rec.grid)) / peak)
    print("sat %d dwell %d: grid error %.3g of the peak, top-cell margin %.3g, q %.6g" % (sat, rec.dwell_count, err, top_cell_margin(rec), rec.q))
    assert err <= TOL
    rows = acq.peek(acq.PEEK_ROW_MAX, sat)
    for b, (val, idx) in enumerate(rec.row_max):
        assert abs(rows[b, 0] - val) <= TOL * peak, b
        assert int(rows[b, 1]) == idx or abs(rec.grid[b, int(rows[b, 1])] - val) <= TOL * peak, b
    r = result
    assert abs(r.mag - rec.mag) <= 2 * TOL * rec.mag and r.test_statistics == r.mag
    assert abs(r.input_power - rec.input_power) <= 2 * TOL * rec.input_power
    assert r.second_peak == 0.0 and r.second_peak_full_row == 0.0
    if top_cell_margin(rec) > 10 * TOL:
        assert (r.indext, r.doppler_index) == (rec.indext, rec.doppler_index)
    else:
        # any cell the restatement holds within TOL of its maximum
        assert rec.grid[r.doppler_index, r.indext] >= rec.mag - TOL * peak
    assert (r.doppler_hz, r.acq_doppler_hz, r.acq_delay_samples) == (bins[r.doppler_index], float(bins[r.doppler_index]), float(r.indext % spc))
    assert (status.state, status.tong_count, status.dwell_count) == want_status
