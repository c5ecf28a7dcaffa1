"""Signals, cases and preconditions of tests/test_caf_gpu.py, free of any GPU call so that seeds are chosen -- and checked -- on the
restatement (tests/caf_ref.py) alone.  Galileo E5a codes from gc_galileo_e5_a_code_gen_complex_sampled at fs = 1000 * samples_per_ms
("5I" is (I, 0), "5Q" is (0, Q)); a block is sampled_ms code periods of samples_per_ms samples.  A restatement is computed once per
case, shared and read-only.

The seeds below were found by `python tests/caf_cases.py` (a scan on the CPU): the first seed of each case under which EVERY choice
of hypothesis has a relative margin >= 1e-2 -- where the arithmetic is REFERENCE, whichever near-maximal index of the QB row
addresses the IB plane (:523) -- and the CAF argmax a margin >= 1e-2.  The margins recorded are those of that seed (under
REFERENCE the CAF argmax sits in the tail section, the only one without a wrapped weight: its margin is of the order of 2^32 wf)."""
import numpy as np

import caf_ref
from tong_cases import top_cell_margin  # the rule that governs exact cell comparison

TOL = 1e-4  # tests/test_acquisition_gpu.py
DMAX, DSTEP = 1000, 500  # five bins, both ends included
WINDOW = 1000  # H = 1
PRN = 11


class Case:
    def __init__(self, name, spm, ms, both, hyp, arithmetic, seed, zero_pad=False, signs=(1, 1, 1), min_choice_margin=None, caf_margin=None):
        self.name, self.spm, self.ms, self.both, self.hyp, self.arithmetic, self.seed = name, spm, ms, both, hyp, arithmetic, seed
        self.zero_pad, self.signs = zero_pad, signs
        self.N = spm * ms
        self.R = (1 + both) * hyp
        self.recorded = (min_choice_margin, caf_margin)


# (samples_per_ms, sampled_ms, R) of the issue's table, plus I only with two hypotheses
MATRIX = [
    Case("2000x1-R2", 2000, 1, 1, 1, caf_ref.REFERENCE, 1, min_choice_margin=None, caf_margin=1.0e8),
    Case("2000x2-R4", 2000, 2, 1, 2, caf_ref.EXACT, 1, signs=(-1, 1), min_choice_margin=0.230, caf_margin=0.0127),
    Case("2000x3-R4", 2000, 3, 1, 2, caf_ref.REFERENCE, 1, signs=(-1, 1, 1), min_choice_margin=0.0538, caf_margin=2.06e8),  # over QB's indices 0.0773
    Case("2000x2-R2-zero-padded", 2000, 2, 1, 1, caf_ref.EXACT, 1, zero_pad=True, signs=(1, -1), min_choice_margin=None, caf_margin=0.0377),
    Case("6625x2-R4", 6625, 2, 1, 2, caf_ref.REFERENCE, 1, signs=(1, 1), min_choice_margin=0.740, caf_margin=7.5e7),
    Case("10000x3-R4", 10000, 3, 1, 2, caf_ref.EXACT, 1, signs=(-1, 1, 1), min_choice_margin=0.0477, caf_margin=0.187),
    Case("2000x2-R2-I-only", 2000, 2, 0, 2, caf_ref.REFERENCE, 1, signs=(-1, 1), min_choice_margin=0.447, caf_margin=2.6e8),
]


def codes_1ms(prn, spm):
    import gnsscorr
    fs = 1000 * spm
    ci = gnsscorr.galileo_e5_a_code_gen_complex_sampled("5I", prn, fs)[:spm]
    cq = gnsscorr.galileo_e5_a_code_gen_complex_sampled("5Q", prn, fs)[:spm]
    return np.ascontiguousarray(ci, np.complex64), np.ascontiguousarray(cq, np.complex64)


def local_codes(prn, spm, ms, zero_pad=False):
    """codeI_ / codeQ_ of the adapter's set_local_code() (:245-270): sampled_ms code periods, or one period and zeros behind it."""
    ci, cq = codes_1ms(prn, spm)
    if zero_pad:
        z = np.zeros(spm * (ms - 1), np.complex64)
        return np.concatenate([ci, z]), np.concatenate([cq, z])
    return np.tile(ci, ms), np.tile(cq, ms)


def signal(prn, spm, n_samples, seed, amp=(0.25, 0.25), doppler=380.0, delay=None, signs_i=(1,), signs_q=None, noise=True):
    """amp[0] * s_i[p] * I + amp[1] * s_q[p] * Q (p the code period, the sign patterns repeating), delayed, on a carrier, in CN(0, 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fs = 1000 * spm
    ci, cq = codes_1ms(prn, spm)
    n = np.arange(n_samples)
    p = n // spm
    si = np.asarray(signs_i, np.float64)[p % len(signs_i)]
    sq = si if signs_q is None else np.asarray(signs_q, np.float64)[p % len(signs_q)]
    base = amp[0] * si * ci[n % spm].astype(np.complex128) + amp[1] * sq * cq[n % spm].astype(np.complex128)
    if delay is None:
        delay = int(rng.integers(0, spm))
    phase = float(rng.uniform(0, 2 * np.pi))
    x = np.roll(base, delay) * np.exp(1j * (2 * np.pi * doppler * n / fs + phase))
    if noise:
        x = x + (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)) * np.sqrt(0.5)
    out = x.astype(np.complex64)
    out.setflags(write=False)
    return out


def conf(spm, ms, dmax=DMAX, dstep=DSTEP, **kw):
    from test_acquisition_gpu import _conf
    return _conf(spm * 1000, ms, 1, float(spm), dmax, dstep, **kw)


def caf_kw(case, window=WINDOW):
    return dict(both_components=case.both, hypotheses=case.hyp, window_hz=window, arithmetic="reference" if case.arithmetic == caf_ref.REFERENCE else "exact")


def freeze(recs):
    for rs in recs:
        for r in rs:
            for a in [r.grid, r.caf, r.caf_i, r.caf_q, r.choice] + list(r.planes.values()):
                a.setflags(write=False)


_REF = {}


def matrix_reference(oracle, case, seed=None):
    key = (case.name, case.seed if seed is None else seed)
    if key not in _REF:
        amp = (0.25, 0.25) if case.both else (0.3, 0.0)
        x = signal(PRN, case.spm, case.N, key[1], amp=amp, signs_i=case.signs)
        ci, cq = local_codes(PRN, case.spm, case.ms, case.zero_pad)
        recs = caf_ref.search(oracle, x, [(ci, cq if case.both else None)], 1000 * case.spm, case.N, DMAX, DSTEP, case.both, case.hyp, WINDOW,
            case.arithmetic, samples_per_code=case.spm)
        freeze(recs)
        _REF[key] = (x, ci, cq, recs[0][0])
    return _REF[key]


def min_choice_margin(rec):
    """The smallest relative margin of any choice of the dwell (None: the case makes no choice)."""
    return min((m for _, _, m in rec.margins), default=None)


def qb_index_margin(rec, arithmetic):
    """REFERENCE reads IB at QB's argmax: the smallest margin of the Q choice over the indices that argmax may be (None where nothing
    depends on it, 0 where the choice would turn)."""
    if arithmetic != caf_ref.REFERENCE or "QB" not in rec.planes:
        return None
    out = []
    for b, row in enumerate(rec.planes["QB"]):
        # every index an engine within TOL of the restatement may take for QB's maximum (a 2 ms block holds each B maximum twice, one
        # code period apart, and IB repeats with it): the choice must stand, with its margin, whichever of them is read
        near = np.nonzero(row >= row.max() * (1 - 10 * TOL))[0]
        n_qa = float(rec.planes["QA"][b].max())
        picked_b = bool(rec.choice[b] & 2)
        for k in near:
            n_qb = float(rec.planes["IB"][b][k])
            out.append(abs(n_qa - n_qb) / max(n_qa, n_qb) if (not n_qa >= n_qb) == picked_b else 0.0)
    return min(out)


def preconditions(rec, case):
    """(ok, text): every choice margin >= 1e-2 -- under REFERENCE also for every index QB's maximum may be read at -- and the CAF
    argmax margin >= 1e-2."""
    cm, qm, fm = min_choice_margin(rec), qb_index_margin(rec, case.arithmetic), rec.caf_margin
    ok = (cm is None or cm >= 1e-2) and (qm is None or qm >= 1e-2) and (fm is None or fm >= 1e-2)
    return ok, "min choice margin %s, min margin over QB's near-maximal indices %s, CAF argmax margin %s" % (cm, qm, fm)


def check_dwell(acq, sat, rec, result, bins, spc, compare_doppler=True, cell_of_this_dwell=True):
    """One satellite of an engine against the restatement's record of the same dwell: grid (the chosen planes), row maxima, CAF_I,
    CAF_Q, choice bytes, result fields.  compare_doppler: the caller has asserted the margin of whatever decides the Doppler (the CAF
    argmax, or the top cell without a filter).  cell_of_this_dwell: the keep rule took this dwell's cell (else the kept index is an
    earlier dwell's: only its delay within the code period is compared here)."""
    grid = acq.grid(sat)
    peak = float(np.nanmax(rec.grid))
    assert grid.shape == rec.grid.shape
    err = float(np.max(np.abs(grid - rec.grid)) / peak)
    caf, caf_i, caf_q, choice = acq.caf_vectors(sat)
    err_i = float(np.max(np.abs(caf_i - rec.caf_i)) / peak)
    err_q = float(np.max(np.abs(caf_q - rec.caf_q)) / peak)
    print("sat %d: grid error %.3g, CAF_I error %.3g, CAF_Q error %.3g of the peak, top-cell margin %.3g, choices %s" % (sat, err, err_i, err_q,
        top_cell_margin(rec), list(choice)))
    assert err <= TOL and err_i <= TOL and err_q <= TOL
    assert list(choice) == list(rec.choice)
    rows = acq.peek(acq.PEEK_ROW_MAX, sat)
    for b, (val, idx) in enumerate(rec.row_max):
        assert abs(rows[b, 0] - val) <= TOL * peak, b
        assert int(rows[b, 1]) == idx or abs(rec.grid[b, int(rows[b, 1])] - val) <= TOL * peak, b
    r = result
    assert abs(r.mag - rec.mag) <= 2 * TOL * rec.mag
    assert abs(r.input_power - rec.input_power) <= 2 * TOL * rec.input_power
    assert abs(r.test_statistics - rec.test_statistics) <= 2 * TOL * rec.test_statistics
    assert r.second_peak == 0.0 and r.second_peak_full_row == 0.0
    if cell_of_this_dwell:
        if top_cell_margin(rec) > 10 * TOL:
            assert r.indext == rec.indext
        else:
            # any cell the restatement holds within TOL of its maximum
            assert float(np.max(rec.grid[:, r.indext])) >= float(np.max(rec.grid)) - TOL * peak
    assert r.indext % spc == rec.indext % spc
    assert r.acq_delay_samples == float(r.indext % spc)
    if compare_doppler:
        assert (r.doppler_index, r.doppler_hz, r.acq_doppler_hz) == (rec.doppler_index, bins[rec.doppler_index], float(bins[rec.doppler_index]))
    return caf


if __name__ == "__main__":
    # the scan that chose the seeds: python tests/caf_cases.py
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "gnss-sdr-1_amd"), os.path.join(root, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        sys.path.insert(0, p)
    from oracle import Oracle
    orc = Oracle()
    for case in MATRIX:
        for seed in range(1, 60):
            rec = matrix_reference(orc, case, seed)[3]
            ok, text = preconditions(rec, case)
            if ok:
                print("%-24s seed %d: %s, top-cell margin %.3g, choices %s" % (case.name, seed, text, top_cell_margin(rec), list(rec.choice)))
                break
            _REF.clear()
        else:
            print("%-24s no seed below 60" % case.name)
