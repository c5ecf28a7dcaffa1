"""Case tables of tests/test_acq_kind_matrix_gpu.py, free of any GPU call: the Tong and the QuickSync engine at every instantiated
column size of the acquisition planner (tests/acq_plan_ref.py).  Sizes, seeds and thresholds are chosen -- and checked, by
tests/test_acq_kind_matrix_inputs.py -- on the numpy restatements alone (tests/tong_ref.py, tests/quicksync_ref.py).  A restatement
is computed once per case, shared and read-only."""
import numpy as np

import tong_cases as tc
import tong_ref
from acq_plan_ref import DWELL_SIZES, MATRIX_SIZES, plan
from test_quicksync_gpu import DMAX as QS_DMAX, DSTEP as QS_DSTEP, PRN as QS_PRN, _signal as qs_signal, preconditions as qs_preconditions
import quicksync_ref

TOL = tc.TOL

# ---- Tong: one size per N1, two satellites, three dwells ------------------------------------------------------------------------------
# Slot 0 holds the code of a PRN the signal does not carry, slot 1 the one it does (50 dB-Hz).  With init 1 the absent satellite's first
# miss ends its search: its workgroups leave at the frozen flag in dwells 2 and 3, while the present one runs ACQ_EPI_TONG once and
# ACQ_EPI_TONG_ACC twice.  tong_max_val and tong_max_dwells of 8 keep it running past dwell 3.
TONG_SIZES = DWELL_SIZES
TONG = (1, 8, 8)
TONG_ABSENT_PRN, TONG_PRN, TONG_CN0, TONG_SEED, TONG_DWELLS = 19, 7, 50.0, 5, 3
TONG_WALK_ABSENT = [(tong_ref.NEGATIVE, 0, 1)]
TONG_WALK_PRESENT = [(tong_ref.RUNNING, 2, 1), (tong_ref.RUNNING, 3, 2), (tong_ref.RUNNING, 4, 3)]
TONG_IDS = ["%d-n1_%d" % (n, plan(n)[0]) for n in TONG_SIZES]


class TongCase:
    """x (3 N samples), codes [absent, present], recs [sat][dwell] of tong_ref.search, threshold and the ratio of the gap it sits in."""


_TONG = {}


def tong_case(oracle, N):
    if N not in _TONG:
        c = TongCase()
        c.N = N
        c.x = tc.signal(oracle, N, (TONG_PRN,), (TONG_CN0,), TONG_DWELLS, seed=TONG_SEED)
        c.codes = tc.codes(oracle, N, (TONG_ABSENT_PRN, TONG_PRN))
        c.recs = tong_ref.search(oracle, c.x, c.codes, N * 1000, N, tc.DMAX, tc.DSTEP, TONG_DWELLS)
        # the geometric middle between the only decision of the absent satellite and the weakest of the present one
        lo, hi = float(c.recs[0][0].q), min(float(r.q) for r in c.recs[1])
        c.threshold, c.ratio = float(np.sqrt(lo * hi)), hi / lo
        for rs in c.recs:
            for r in rs:
                r.grid.setflags(write=False)
        _TONG[N] = c
    return _TONG[N]


def tong_deciding(c):
    """The dwells whose statistic a detector compares: the absent satellite's first, all three of the present one."""
    return [c.recs[0][:1], c.recs[1]]


def tong_preconditions(c):
    """(walk of the absent, walk of the present, gap ratio, decision margin, smallest top-cell margin) on the restatement alone."""
    absent = tc.outcome(c.recs[0], c.threshold, TONG)
    present = tc.outcome(c.recs[1], c.threshold, TONG)
    margin = tc.decision_margin(tong_deciding(c), c.threshold)
    top = min(tc.top_cell_margin(r) for rs in tong_deciding(c) for r in rs)
    return absent, present, c.ratio, margin, top


# ---- QuickSync: (M, f) -> seed ---------------------------------------------------------------------------------------------------------
# The folded transform has M = N / f points: the fold kernel writes the row-permuted layout of the plan of M, the forward epilogue
# stores with that plan's map.  Seeds are those of helpers.synth_stream under which the restatement meets
# test_quicksync_gpu.preconditions; they are written down, not searched for.
QS_ODD_SIZES = (3069, 5115, 9207, 15345, 25575)  # N1 = 3, 5, 9, 15, 25: the 8-byte fold path with a gather across several columns
QS_SEED_2 = (20000, 64000, 19200)
QS_CASES = {}
for _m in MATRIX_SIZES + QS_ODD_SIZES:
    QS_CASES[(_m, 2)] = 2 if _m in QS_SEED_2 else 1
QS_CASES[(3000, 3)] = 1
QS_CASES[(10230, 4)] = 2
QS_CASES[(24000, 4)] = 1
QS_KEYS = list(QS_CASES)
QS_IDS = ["M%d-f%d-n1_%d-%s" % (m, f, plan(m)[0], "perm" if plan(m)[3] else "plain") for m, f in QS_KEYS]
# the block again from a device buffer that is 8 but not 16 bytes aligned: the 8-byte fold path with M even as well
QS_ODD_OFFSET = tuple((m, 2) for m in QS_ODD_SIZES + (24000, 32000, 64000))


def qs_truth_checked(M, f):
    """Whether the restatement's delay is held to the signal's own.  With four periods integrated coherently a Doppler between two bins
    costs most of the peak: (24000, 4) passes both preconditions and still lies 36 samples from the truth, so f = 4 compares with
    the restatement alone."""
    return f == 2 or (M, f) == (3000, 3)


_QS = {}


def qs_reference(oracle, M, f):
    """As test_quicksync_gpu.reference, for a code period of N = f M samples: (x, truth, code, restatement's result)."""
    if (M, f) not in _QS:
        N = f * M
        x, truth = qs_signal(oracle, N, f, QS_CASES[(M, f)])
        code = oracle.gps_l1_ca_code_sampled(QS_PRN, N * 1000)[:N]
        (r,) = quicksync_ref.search(oracle, x, [code], N * 1000, N, f, QS_DMAX, QS_DSTEP)
        r.grid.setflags(write=False)
        x.setflags(write=False)
        _QS[(M, f)] = (x, truth[0], code, r)
    return _QS[(M, f)]


def qs_delay_error(M, f, truth, ref):
    """Distance of the restatement's delay from the signal's, in samples, round the code period."""
    N = f * M
    expect = (-truth["tau0"] * N * 1000 / 1.023e6) % N
    d = abs(ref.acq_delay_samples - expect)
    return min(d, N - d)
