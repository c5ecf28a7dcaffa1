"""CPU tests (no GPU) of the numpy restatement of the Tong detector (tests/tong_ref.py) and of gc_tong_threshold: the first dwell's
grid is the plain oracle's grid times 1 / (N^4 P), the state machine on hand-made q sequences (the ones
tests/acq_tong_decide_selftest.cpp runs through the shared C++ step), the adapters' threshold in closed form."""
import math

import numpy as np
import pytest

import tong_ref
from tong_ref import NEGATIVE as N, POSITIVE as P, RUNNING as R


def test_first_dwell_is_the_plain_grid_normalised(oracle):
    from helpers import synth_stream
    fs, n = 2000000, 2000
    x, _ = synth_stream([oracle.gps_l1_ca_code(3).astype(np.float32)], fs, 2 * n, seed=77, cn0_db_hz=(47.0, 47.0), doppler_max=900.0)
    code = oracle.gps_l1_ca_code_sampled(3, fs)[:n]
    # the plain search has four bins (-1000 .. 500); the Tong grid is inclusive and holds a fifth
    assert len(tong_ref.doppler_bins(1000, 500)) == 5 and len(tong_ref.doppler_bins(5000, 250)) == 41
    (recs,) = tong_ref.search(oracle, x, [code], fs, n, 1000, 500, 2)
    p = oracle.pcps(fs_in=fs, sampled_ms=1, ms_per_code=1, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=float(n), samples_per_chip=2,
        doppler_max=1000, doppler_step=500)
    p.set_local_code(code)
    q = p.core(x[:n])
    plain = p.grid().astype(np.float64)
    power = float(np.mean(np.abs(x[:n].astype(np.complex128)) ** 2))
    want = plain / (float(n) ** 4 * power)
    got = recs[0].grid[:4]
    assert np.max(np.abs(got - want)) <= 1e-4 * want.max()
    assert (recs[0].indext, recs[0].doppler_hz) == (q.indext, q.doppler)
    assert recs[0].acq_delay_samples == q.indext % n and recs[0].dwell_count == 1 and recs[0].q == recs[0].mag
    assert abs(recs[0].input_power - power) <= 1e-12 * power
    # the second dwell adds its own block normalised by its own power: not a multiple of the summed raw grid
    p.reset_grid()
    p.core(x[n:2 * n])
    plain2 = p.grid().astype(np.float64)
    power2 = float(np.mean(np.abs(x[n:2 * n].astype(np.complex128)) ** 2))
    want2 = want + plain2 / (float(n) ** 4 * power2)
    assert np.max(np.abs(recs[1].grid[:4] - want2)) <= 1e-4 * want2.max()
    assert recs[1].q == recs[1].mag / 2 and recs[1].row_max[recs[1].doppler_index] == (recs[1].mag, recs[1].indext)


SEQUENCES = [
    # (init, max, max_dwells), q in units of the threshold, [(state, count, dwell)]
    ((1, 2, 3), [1.5], [(P, 2, 1)]),
    ((1, 2, 3), [0.5], [(N, 0, 1)]),  # init 1 goes negative on the first miss
    ((2, 4, 8), [1.2, 1.3], [(R, 3, 1), (P, 4, 2)]),
    ((2, 4, 8), [0.9, 0.8], [(R, 1, 1), (N, 0, 2)]),
    ((2, 4, 8), [1.1, 0.9, 1.1, 0.7, 1.2, 1.2], [(R, 3, 1), (R, 2, 2), (R, 3, 3), (R, 2, 4), (R, 3, 5), (P, 4, 6)]),
    ((2, 4, 8), [1.32, 0.68, 0.49, 0.41], [(R, 3, 1), (R, 2, 2), (R, 1, 3), (N, 0, 4)]),
    ((2, 4, 4), [1.1, 0.9, 1.1, 0.9], [(R, 3, 1), (R, 2, 2), (R, 3, 3), (N, 2, 4)]),  # negative by tong_max_dwells
    ((2, 4, 2), [1.1, 1.1], [(R, 3, 1), (N, 4, 2)]),  # a positive overridden at tong_max_dwells
    ((1, 2, 1), [5.0], [(N, 2, 1)]),  # tong_max_dwells = 1
    ((1, 2, 1), [0.1], [(N, 0, 1)]),
    ((2, 4, 8), [1.0, 1.0], [(R, 1, 1), (N, 0, 2)]),  # equality is no hit
    ((2, 4, 8), [float("nan"), 0.0], [(R, 1, 1), (N, 0, 2)]),
]


@pytest.mark.parametrize("tong, q, want", SEQUENCES, ids=[str(i) for i in range(len(SEQUENCES))])
def test_state_machine_on_hand_made_sequences(tong, q, want):
    assert tong_ref.walk(q, 1.0, *tong) == want
    # the same walk with another threshold and the statistics scaled with it
    assert tong_ref.walk([v * 3.0 for v in q], 3.0, *tong) == want


def test_infinite_threshold_counts_down():
    assert tong_ref.walk([1e30] * 5, float("inf"), 3, 5, 10) == [(R, 2, 1), (R, 1, 2), (N, 0, 3)]


def test_place_threshold():
    t, ratio = tong_ref.place_threshold([1.0, 1.02, 2.0, 2.1, 0.0])
    assert t == pytest.approx(math.sqrt(1.02 * 2.0)) and ratio == pytest.approx(2.0 / 1.02)


@pytest.mark.parametrize("pfa, vector_length, dmax, dstep", [
    (0.01, 4000, 5000, 250),   # GpsL1CaPcpsTongAcquisition at 4 Msps: 1 ms, 41 bins
    (0.01, 16000, 5000, 250),  # GalileoE1PcpsTongAmbiguousAcquisition at 4 Msps: 4 ms
    (1e-4, 2000, 1000, 500), (0.001, 4000, 5000, 333)])
def test_threshold_follows_the_adapters_formula(pfa, vector_length, dmax, dstep):
    import gnsscorr
    bins = len(range(-dmax, dmax + 1, dstep))
    ncells = vector_length * bins
    val = (1.0 - float(np.float32(pfa))) ** (1.0 / ncells)
    want = -math.log(1.0 - val) / float(vector_length)  # quantile of Exp(lambda = vector_length)
    got = gnsscorr.tong_threshold(pfa, vector_length, dmax, dstep)
    assert got == pytest.approx(want, rel=1e-6)
    assert got == np.float32(want) or abs(got - want) <= 2e-7 * want
