"""CPU check of the inputs of tests/test_acq_kind_matrix_gpu.py (tests/acq_kind_matrix_cases.py): the Tong sizes reach every
instantiated column size, the QuickSync table every column size with every store map and an odd M under more than one column, and
every case meets, on the restatement alone, the preconditions its GPU comparison rests on.  A later edit of a seed or a size cannot
then hollow out the GPU tests unnoticed; when the planner's preferences change, the guards fail and the sizes have to be picked again."""
import pytest

import acq_kind_matrix_cases as K
import acq_plan_ref as P
from acq_kind_matrix_cases import TOL


def test_tong_sizes_reach_every_column_kernel():
    """acq_cols_tong_kernel<N1, ACQ_EPI_TONG | ACQ_EPI_TONG_ACC>: 17 N1, and the walk of every case runs both epilogues."""
    assert len(K.TONG_SIZES) == 17 and {P.plan(n)[0] for n in K.TONG_SIZES} == set(P.N1_CANDIDATES)
    assert sum(P.plan(n)[0] > 25 for n in K.TONG_SIZES) == 3  # the one-wave launch bounds
    assert len(set(K.TONG_IDS)) == 17


def test_quicksync_table_reaches_every_column_size_and_store_map():
    # the 43 sizes of the plain engine's matrix and five odd ones at f = 2, three cases at f = 3 and 4
    assert len(K.QS_KEYS) == len(P.MATRIX_SIZES) + 5 + 3 == 51 and len(set(K.QS_IDS)) == 51
    f2 = [m for m, f in K.QS_KEYS if f == 2]
    assert set(P.MATRIX_SIZES) <= set(f2)
    reached = {}
    for m in f2:
        n1, _, _, perm = P.plan(m)
        reached.setdefault(n1, set()).add(perm)
    assert set(reached) == set(P.N1_CANDIDATES)
    for n1, (plain, perm) in P.MATRIX.items():
        assert reached[n1] == ({False} if plain else set()) | ({True} if perm else set()), n1
    # the fold's LDS tile of 64 x N1 values stays under what acq_qs_launch_fold allows
    assert max(reached) * 64 * 8 <= 48 * 1024
    odd = [(m, f) for m, f in K.QS_KEYS if m % 2 == 1 and P.plan(m)[0] > 1]
    assert len(odd) >= 5 and {P.plan(m)[0] for m, _ in odd} >= {3, 5, 9, 15, 25}
    # the odd-offset runs: every odd M with several columns, and even M under the three largest column sizes
    assert set(K.QS_ODD_OFFSET) <= set(K.QS_KEYS)
    assert {P.plan(m)[0] for m, _ in K.QS_ODD_OFFSET if m % 2 == 0} == {25, 32, 50}
    assert [P.plan(m)[0] for m in K.QS_ODD_SIZES] == [3, 5, 9, 15, 25]
    # a plan for the other folding factors too
    assert [P.plan(m)[0] for m, f in K.QS_KEYS if f != 2] == [3, 10, 25]


@pytest.mark.parametrize("N", K.TONG_SIZES, ids=K.TONG_IDS)
def test_tong_case_meets_its_preconditions(oracle, N):
    c = K.tong_case(oracle, N)
    assert c.x.size == K.TONG_DWELLS * N and [len(rs) for rs in c.recs] == [K.TONG_DWELLS] * 2
    absent, present, ratio, margin, top = K.tong_preconditions(c)
    print("threshold %.6g in a gap of ratio %.3f, decision margin %.3g, smallest top-cell margin %.3g" % (c.threshold, ratio, margin, top))
    # the absent satellite is frozen from dwell 2 on; the present one runs the storing epilogue once, the accumulating one twice
    assert absent == K.TONG_WALK_ABSENT and present == K.TONG_WALK_PRESENT
    # the project's bars (tests/test_tong_gpu.py) ...
    assert ratio >= 1.05 and margin >= 1e-2
    # ... and what these cases were chosen to have: every cell of a result is compared exactly
    assert 4.6 <= ratio <= 8.8 and margin >= 0.53
    assert top > 1.6e-3 and top > 10 * TOL


@pytest.mark.parametrize("M, f", K.QS_KEYS, ids=K.QS_IDS)
def test_quicksync_case_meets_its_preconditions(oracle, M, f):
    x, truth, code, ref = K.qs_reference(oracle, M, f)
    assert x.size == f * f * M and code.size == f * M and ref.grid.shape == (5, M)
    margin, ratio = K.qs_preconditions(ref)
    err = K.qs_delay_error(M, f, truth, ref)
    print("seed %d: margin %.3g, candidate ratio %.3g, delay %.1f samples from the truth" % (K.QS_CASES[(M, f)], margin, ratio, err))
    assert margin > 10 * TOL and ratio >= 2.0
    if K.qs_truth_checked(M, f):
        assert err <= f * M / 1023.0 + 1
        assert abs(ref.doppler_hz - truth["doppler"]) <= K.QS_DSTEP / 2
