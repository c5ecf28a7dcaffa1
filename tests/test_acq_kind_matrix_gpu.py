"""GPU parity of the Tong and the QuickSync engine at every instantiated column size of the acquisition planner, the counterpart of
tests/test_acquisition_matrix_gpu.py for the two engines with size-dependent device code of their own: the 34 instances of
acq_cols_tong_kernel (its frozen-satellite exit, the prev[] prefetch of the accumulating epilogue, the one-wave launch bounds above
N1 = 25) and acq_qs_fold_kernel's LDS gather into the row-permuted layout (16-byte and 8-byte loads) with the forward epilogue's
store maps behind it.  Cases, seeds and thresholds: tests/acq_kind_matrix_cases.py, held to their preconditions without a GPU by
tests/test_acq_kind_matrix_inputs.py.  Bars are the project's: indices and Doppler exact, magnitudes within TOL = 1e-4 of the peak."""
import numpy as np
import pytest

import acq_kind_matrix_cases as K
import tong_cases as tc
import tong_ref
from test_quicksync_gpu import _fields, check_against_the_restatement
from test_tong_gpu import snapshot

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", K.TONG_SIZES, ids=K.TONG_IDS)
def test_tong_at_every_column_size(gctx, oracle, N):
    """Two satellites, three dwells.  The present one against the restatement after every dwell (ACQ_EPI_TONG, then ACQ_EPI_TONG_ACC
    twice); the absent one against it after dwell 1, where it goes negative, and byte for byte the same after dwells 2 and 3: a
    frozen workgroup that got past its exit, or a frozen[] read at the wrong index, changes its grid or row maxima.  Then the same
    three blocks enqueued back to back with one fetch: every bit as in the per-call run."""
    import gnsscorr
    import torch
    c = K.tong_case(oracle, N)
    absent, present, ratio, margin, top = K.tong_preconditions(c)
    print("restatement: threshold %.6g in a gap of ratio %.3f, decision margin %.3g, smallest top-cell margin %.3g" % (c.threshold, ratio, margin, top))
    assert absent == K.TONG_WALK_ABSENT and present == K.TONG_WALK_PRESENT
    assert ratio >= 1.05 and margin >= 1e-2 and top > 10 * tc.TOL
    bins = tong_ref.doppler_bins(tc.DMAX, tc.DSTEP)
    acq = gnsscorr.PcpsAcquisition(gctx, 2, tong=K.TONG, **tc.conf(N))
    assert (acq.fft_size, acq.consumed_samples, acq.num_doppler_bins) == (N, N, 5)
    for s_, code in enumerate(c.codes):
        acq.set_local_code(s_, code)
    acq.set_threshold(c.threshold)
    frozen = per_call = None
    for d in range(K.TONG_DWELLS):
        res = acq.dwell(c.x[d * N:(d + 1) * N])
        status = acq.tong_status()
        tc.check_dwell(acq, 1, c.recs[1][d], status[1], res[1], present[d], bins, N)
        per_call = snapshot(acq, res, status)
        if d == 0:
            tc.check_dwell(acq, 0, c.recs[0][0], status[0], res[0], absent[0], bins, N)
            frozen = per_call[0]
        else:
            assert per_call[0] == frozen, "dwell %d changed the frozen satellite" % (d + 1)
    d_x = torch.from_numpy(np.array(c.x).view(np.float32)).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    acq.reset()
    for d in range(K.TONG_DWELLS):
        acq.dwell_enqueue(d_x.data_ptr() + 8 * N * d, st.cuda_stream)
    res = acq.fetch_results(st.cuda_stream)
    back_to_back = snapshot(acq, res, acq.tong_status())
    for s_ in range(2):
        assert back_to_back[s_] == per_call[s_], s_
    acq.close()


def _qs_snapshot(acq, res):
    """Everything a caller can read of a QuickSync dwell, for bit-exact comparisons."""
    return (_fields(res[0]), acq.grid(0).tobytes(), acq.peek(acq.PEEK_ROW_MAX, 0).tobytes(), tuple(v.tolist() for v in acq.candidates(0)))


@pytest.mark.parametrize("M, f", K.QS_KEYS, ids=K.QS_IDS)
def test_quicksync_at_every_column_size(gctx, oracle, M, f):
    """The matrix check of tests/test_quicksync_gpu.py for a transform of M points.  Cases of K.QS_ODD_OFFSET run the block once more
    from a device buffer at an odd sample offset: the fold takes its 8-byte path whatever M, and the bits do not depend on it."""
    import torch
    N = f * M
    case = K.qs_reference(oracle, M, f)
    acq = check_against_the_restatement(gctx, oracle, N, f, case, K.qs_truth_checked(M, f))
    if (M, f) in K.QS_ODD_OFFSET:
        x = case[0]
        L = f * N
        aligned = _qs_snapshot(acq, acq.dwell(x))
        buf = torch.zeros(2 * (L + 1), dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        buf[2:] = torch.from_numpy(np.array(x[:L]).view(np.float32))
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        acq.dwell_enqueue(buf.data_ptr() + 8, st.cuda_stream)
        assert _qs_snapshot(acq, acq.fetch_results(st.cuda_stream)) == aligned
    acq.close()
