"""CPU tests (no GPU) of the fine Doppler restatement (tests/fine_doppler_ref.py) and of the inputs the GPU tests use
(tests/fine_doppler_cases.py): a tone on a fine bin is found, the rotate map is std::rotate's, the window rule of the library
(gc_fine_doppler_window, csrc/acq_fine_window.h) is the brute-force one, and every case keeps a top-two margin of 1e-3 of its peak."""
import numpy as np
import pytest

import fine_doppler_cases as fc
import fine_doppler_ref as ref


def test_a_tone_on_a_fine_bin_is_found_with_exact_alignment():
    N, P, Z, s = 2000, 10, 8, 777
    fs, next_size = N * 1000, P * N * Z
    rng = np.random.Generator(np.random.PCG64(11))
    code = fc.make_codes(N, 1, rng)[0]
    n = np.arange(P * N)
    for k in (0, 37, next_size - 141):  # 0 Hz, +462.5 Hz, -1762.5 Hz
        kk = k if k < next_size // 2 else k - next_size
        x = code[(n - s) % N] * np.exp(2j * np.pi * ((kk * n) % next_size) / next_size + 0.3j)
        coarse = 500.0 * round(kk * fs / next_size / 500.0)
        r = ref.refine(x, code, fs, N, P, Z, s, coarse, alignment=ref.EXACT)
        assert (r.bin, r.full_bin, r.accepted, r.status) == (k, k, True, ref.REFINED)
        assert r.doppler_hz == r.acq_doppler_hz == kk * 12.5
        assert abs(r.peak - (P * N) ** 2) <= 1e-9 * (P * N) ** 2 and abs(r.mean - P * N) <= 1e-9 * P * N
        # the neighbour of a tone on a fine bin is 5 % down at Z = 8
        assert 0.04 < r.margin < 0.06
        # the block's own rotate is one sample late for s >= 2: the peak stays, lower
        q = ref.refine(x, code, fs, N, P, Z, s, coarse, alignment=ref.REFERENCE)
        assert q.bin == k and 0.1 * r.peak < q.peak < 0.9 * r.peak


@pytest.mark.parametrize("N", [16, 2000])
def test_rotate_map_is_std_rotate(N):
    code = list(range(N))
    for s in (0, 1, 2, N // 3, N - 1):
        want = code if s == 0 else ref.std_rotate(code, 0, N - s, N - 1)
        got = [code[i] for i in ref.replica_index_map(N, s, ref.REFERENCE)]
        assert got == want, s
        assert got[N - 1] == N - 1
        exact = [code[i] for i in ref.replica_index_map(N, s, ref.EXACT)]
        assert exact == code[N - s:] + code[:N - s] if s else exact == code
    # s = 1 is a no-op; from s = 2 on the reference is the exact rotation by s - 1 of the first N - 1 elements
    assert list(ref.replica_index_map(N, 1, ref.REFERENCE)) == code


@pytest.mark.parametrize("N", fc.SIZES)
def test_window_rule_is_the_brute_force_one(N):
    import gnsscorr
    fs, next_size = N * 1000, 80 * N
    table = ref.freq_table(fs, next_size)
    assert table.dtype == np.float32 and table[0] == 0 and table[next_size // 2] == -fs / 2
    for coarse in (0.0, 500.0, -500.0, 4500.0, -4500.0, 2500.0, -2500.0, 1762.5, -0.001, 12.5, 6.25, 993.75, -1006.25):
        first, count = ref.window(fs, next_size, coarse, 1000.0, table)
        assert gnsscorr.fine_doppler_window(fs, next_size, coarse, 1000.0) == (first, count), coarse
        if coarse in (0.0, 500.0, -500.0, 4500.0, -4500.0):
            assert count == 159
        if abs(coarse) < 1000.0 - 12.5:
            assert first + count > next_size  # the run crosses from index Next - 1 to 0
    # other widths and table sizes, among them windows of one and two bins
    for nxt, coarse, w in ((N, 0.0, 1000.0), (N, 500.0, 1000.0), (8 * N, -2500.0, 1000.0), (8 * N, 4500.0, 333.0), (2 * N, 0.0, 100.0), (80 * N, 0.0, 12.5),
            (80 * N, 6.0, 6.5), (2 * N, 250.0, 100.0)):
        if nxt % 2:
            # an odd table has no Nyquist entry to split at: refused (6625 x 1 x 1)
            with pytest.raises(gnsscorr.GnsscorrError):
                gnsscorr.fine_doppler_window(fs, nxt, coarse, w)
            continue
        first, count = ref.window(fs, nxt, coarse, w)
        got = gnsscorr.fine_doppler_window(fs, nxt, coarse, w)
        assert got[1] == count and (count == 0 or got[0] == first), (nxt, coarse, w)
    assert ref.window(fs, 2 * N, 250.0, 100.0)[1] == 0 and ref.window(fs, 80 * N, 6.0, 6.5)[1] == 1


CASES = list(fc.MATRIX) + [(25000, 10, 8)]


@pytest.mark.parametrize("N,P,Z", CASES)
def test_every_case_has_its_top_two_margin(N, P, Z):
    """A condition on the inputs: the GPU tests compare bins exactly, so no window of theirs may hold a near tie."""
    blk = fc.block(N, P, Z)
    assert blk.x.dtype == np.complex64 and blk.x.size == P * N
    for alignment in fc.ALIGNMENTS:
        recs = fc.records(blk, alignment)
        print(N, P, Z, alignment, ["%.3g" % r.margin for r in recs])
        for r in recs:
            assert r.margin >= fc.MARGIN
            assert r.peak > 0 and r.mean > 0
    if (N, P, Z) == (2000, 10, 8):
        # the variants the GPU tests derive from this block: the quantised rings, and a slot asked twice with two coarse values
        for bits in (16, 8):
            _, xq = fc.quantise(blk.x, bits)
            for r in fc.records(blk, ref.EXACT, key="i%d" % bits, x=xq):
                assert r.margin >= fc.MARGIN
        slot, s, coarse = blk.requests[2]
        table = ref.freq_table(blk.fs, P * N * Z)
        for other in (coarse + 500.0, coarse - 487.5):
            assert ref.refine(blk.x, blk.codes[slot], blk.fs, N, P, Z, s, other, 1000.0, ref.EXACT, table).margin >= fc.MARGIN
