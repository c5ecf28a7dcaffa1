"""CPU check of the closed-loop matrix's inputs (tests/closed_loop_matrix_cases.py): every reference configuration of
tests/test_closed_loop_matrix_gpu.py through the restatement alone.  The matrix compares kernels on these signals with tight gates
and no allowance for a forked block length, which only means something while the loop is locked, every period is valid, the window
start visits every 16-byte phase and no block length sits on the edge of a sample."""
import numpy as np
import pytest

import closed_loop_matrix_cases as M


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("key", M.REFERENCED, ids=str)
def test_reference_configuration_is_a_fair_input(oracle, key, fmt):
    taps, pilot, hd, L, spc = M.shape(key)
    ref = M.reference(oracle, key, fmt)
    assert len(ref) == M.N_EP
    assert all(r["valid"] == 1 and r["integrating"] == 0 for r in ref)
    # data channels never leave state 2 (no synchronisation data); a pilot channel with one symbol per bit and no secondary code hands
    # over to narrow tracking at its first loop update
    want = 4 if pilot else 2
    assert all(r["state"] == want for r in ref), [r["state"] for r in ref]
    # the prompt sits on the peak: a sample's amplitude times the block length (times the quantiser's scale)
    prompt = np.mean([abs(r["corr"][taps // 2]) for r in ref[-8:]])
    assert prompt >= 0.5 * M.AMP * M.N * M.SCALE[fmt], (prompt, M.AMP * M.N * M.SCALE[fmt])
    # the window start walks through every residue mod 8 samples: every 16-byte phase of 8-, 4- and 2-byte samples
    assert {r["pos"] % 8 for r in ref} == set(range(8))
    # block length floor(K): K never within 1e-3 samples of a whole one, where the device's libm and numpy could round it to different
    # sides (the one-sample fork the loop fuzz allows for sits ~1e-9 from the edge)
    margin = min(min(r["rem_code_samples"], 1.0 - r["rem_code_samples"]) for r in ref)
    assert margin >= 1e-3, margin
    if hd:
        # the rate smoothers fill after 2 * smoother_length periods: the later periods run with a carrier rate
        assert any(float(r["args"][5]) != 0.0 for r in ref[2 * M.HD_SMOOTHER:])


def test_quantised_streams_use_their_range():
    """int16 at scale 300 never clips; int8 at scale 25 sits well inside +-127 (7 sigma of the noise) and clips next to nothing."""
    for key in M.REFERENCED:
        q16, f16 = M.samples(key, "i16")
        q8, f8 = M.samples(key, "i8")
        assert q16.dtype == np.int16 and q8.dtype == np.int8 and f16.dtype == np.complex64 and f8.size == M.N * (M.N_EP + 3)
        assert np.abs(q16.astype(np.int32)).max() < 32767 and np.abs(q16.astype(np.int32)).max() > 600
        assert np.abs(q8.astype(np.int32)).max() <= 127 and np.mean(np.abs(q8.astype(np.int32)) == 127) < 1e-4
        assert np.array_equal(f8.view(np.float32).reshape(-1, 2), q8.astype(np.float32))
