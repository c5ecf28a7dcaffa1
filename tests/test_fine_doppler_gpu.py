"""GPU tests of the fine Doppler stage (gnsscorr.FineDoppler, gc_fine_doppler_*) against the numpy restatement
tests/fine_doppler_ref.py.  In every comparison bin, window_first_bin and window_bins are equal, doppler_hz is equal as float32 bits,
spectrum() and peak lie within TOL = 1e-4 of the window's peak and mean within 1e-4 relative (fine_doppler_cases.check).  Inputs come
from tests/fine_doppler_cases.py: six satellites per block, whose six requests cover the delays {0, 1, 2, N/3, N/3 + 7, N - 1} and
the coarse values {0, 500, +-2500, +-4500}; tests/test_fine_doppler_ref.py asserts their top-two margins on the restatement.
N = 6625 with (P, Z) = (1, 1) gives an odd Next, which the engine refuses: it is tested as a refusal."""
import numpy as np
import pytest

import fine_doppler_cases as fc
import fine_doppler_ref as ref

pytestmark = pytest.mark.gpu


def engine(gctx, blk, alignment, n_slots=None, **kw):
    import gnsscorr
    fd = gnsscorr.FineDoppler(gctx, len(blk.codes) if n_slots is None else n_slots, blk.fs, blk.N, prn_replicas=blk.P, zero_padding_factor=blk.Z,
        alignment=alignment, **kw)
    for slot, c in enumerate(blk.codes[:fd.n_slots]):
        fd.set_code(slot, c)
    return fd


def ring_of(gctx, samples, lead=0, capacity=None, max_window=256, iq_format=None):
    """A ring that holds `lead` other samples in front of the block; returns (ring, first_index of the block)."""
    import gnsscorr
    n = len(samples)
    kw = {} if iq_format is None else dict(iq_format=iq_format)
    ring = gnsscorr.IqStream(gctx, capacity_samples=capacity or (n + lead + 64), max_window_samples=max_window, **kw)
    if lead:
        ring.push(samples[:lead])
    return ring, ring.push(samples)


def check_all(fd, res, recs):
    for i, (r, rec) in enumerate(zip(res, recs)):
        fc.check(r, fd.spectrum(i), rec, fd.next_size)


# ---- 1. the matrix against the restatement ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("alignment", fc.ALIGNMENTS)
@pytest.mark.parametrize("N,P,Z", fc.MATRIX)
def test_matrix_against_the_restatement(gctx, N, P, Z, alignment):
    """Every size, (P, Z), delay, coarse value and alignment; the block lies at an odd first_index, is longer than the ring's
    max_window (256) and, for P = 10, longer than one tile of the kernel by far."""
    blk = fc.block(N, P, Z)
    recs = fc.records(blk, alignment)
    fd = engine(gctx, blk, alignment)
    ring, first = ring_of(gctx, blk.x, lead=37)
    assert first == 37 and fd.block_samples == P * N > 256
    res = fd.estimate_stream(ring, first, blk.requests)
    assert len(res) == 6
    check_all(fd, res, recs)
    # the windows of 0 and 500 Hz straddle index 0 of the spectrum
    for r in res[:2]:
        assert r.window_first_bin + r.window_bins > fd.next_size or (P, Z) == (1, 1)
    fd.close()
    ring.close()


def test_an_odd_transform_size_is_refused(gctx):
    import gnsscorr
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.FineDoppler(gctx, 1, 6625000, 6625, prn_replicas=1, zero_padding_factor=1)
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "even" in str(e.value)


def test_large_block_two_requests(gctx):
    """N = 25000 (25 Msps): Next = 2 000 000, 245 tiles per request."""
    blk = fc.block(25000, 10, 8)
    two = fc.Block(blk.N, blk.fs, blk.P, blk.Z, blk.x, blk.codes, [blk.requests[3], blk.requests[1]], None)
    recs = [fc.records(blk, ref.REFERENCE)[3], fc.records(blk, ref.REFERENCE)[1]]
    fd = engine(gctx, blk, ref.REFERENCE)
    ring, first = ring_of(gctx, blk.x, lead=5)
    res = fd.estimate_stream(ring, first, two.requests)
    check_all(fd, res, recs)
    fd.close()
    ring.close()


# ---- 2. requests ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small(gctx):
    """The N = 2000, P = 10, Z = 8 block in a ring, with an engine of six slots (exact alignment)."""
    blk = fc.block(2000, 10, 8)
    fd = engine(gctx, blk, ref.EXACT)
    ring, first = ring_of(gctx, blk.x, lead=1)
    yield blk, fd, ring, first
    fd.close()
    ring.close()


def test_request_counts_and_bit_identity(small):
    blk, fd, ring, first = small
    recs = fc.records(blk, ref.EXACT)
    # n_slots requests
    full = fd.estimate_stream(ring, first, blk.requests)
    check_all(fd, full, recs)
    full_spec = [fd.spectrum(i).tobytes() for i in range(6)]
    # two calls in a row give identical bits
    again = fd.estimate_stream(ring, first, blk.requests)
    assert [fc.result_bits(r) for r in again] == [fc.result_bits(r) for r in full]
    assert [fd.spectrum(i).tobytes() for i in range(6)] == full_spec
    # one request alone, and the same request at another place of a batch of five: identical bits
    alone = fd.estimate_stream(ring, first, [blk.requests[4]])
    assert len(alone) == 1
    fc.check(alone[0], fd.spectrum(0), recs[4], fd.next_size)
    alone_spec = fd.spectrum(0).tobytes()
    five = [blk.requests[i] for i in (2, 0, 5, 4, 1)]
    batch = fd.estimate_stream(ring, first, five)
    assert len(batch) == 5
    check_all(fd, batch, [recs[i] for i in (2, 0, 5, 4, 1)])
    assert fc.result_bits(batch[3]) == fc.result_bits(alone[0]) == fc.result_bits(full[4])
    assert fd.spectrum(3).tobytes() == alone_spec == full_spec[4]
    with pytest.raises(Exception):
        fd.spectrum(5)  # the last call had five requests


def test_a_slot_twice_with_two_coarse_values(small):
    blk, fd, ring, first = small
    slot, s, coarse = blk.requests[2]
    table = ref.freq_table(blk.fs, fd.next_size)
    others = (coarse + 500.0, coarse - 487.5)
    res = fd.estimate_stream(ring, first, [(slot, s, others[0]), (slot, s, others[1]), (slot, s, coarse)])
    for i, c in enumerate(others + (coarse,)):
        rec = ref.refine(blk.x, blk.codes[slot], blk.fs, blk.N, blk.P, blk.Z, s, c, 1000.0, ref.EXACT, table)
        fc.check(res[i], fd.spectrum(i), rec, fd.next_size)
    # the tone is inside all three windows: one bin, three different runs
    assert res[0].bin == res[1].bin == res[2].bin and len({r.window_first_bin for r in res}) == 3


def test_request_checks(small):
    import gnsscorr
    blk, fd, ring, first = small
    ok = blk.requests[0]
    lone = gnsscorr.FineDoppler(fd._ctx, 2, blk.fs, blk.N)
    lone.set_code(1, blk.codes[0])
    before = fd.estimate_stream(ring, first, [ok])
    spec = fd.spectrum(0).tobytes()
    bad = ((fd, []), (fd, [ok] * 7),                                   # 1 <= n_requests <= n_slots
        (fd, [(6, 0, 0.0)]), (lone, [(0, 0, 0.0)]),                      # a slot outside the handle, a slot without a code
        (fd, [(0, blk.N, 0.0)]), (fd, [ok, (1, blk.N + 5, 0.0)]),        # delay_samples >= N
        (fd, [(0, 0, blk.fs / 2 - 1000.0)]), (fd, [(0, 0, -blk.fs / 2 + 999.0)]), (fd, [(0, 0, float("nan"))]), (fd, [(0, 0, float("inf"))]))
    for h, reqs in bad:
        with pytest.raises(gnsscorr.GnsscorrError) as e:
            h.estimate_stream(ring, first, reqs)
        assert e.value.status == gnsscorr.GC_ERR_INVALID, reqs
        with pytest.raises(gnsscorr.GnsscorrError) as e:
            h.estimate(blk.x, reqs)
        assert e.value.status == gnsscorr.GC_ERR_INVALID, reqs
    # nothing ran: the last call's spectrum is still there, and the same call gives the same bits
    assert fd.spectrum(0).tobytes() == spec
    assert fc.result_bits(fd.estimate_stream(ring, first, [ok])[0]) == fc.result_bits(before[0])
    assert lone.estimate_stream(ring, first, [(1, 0, 0.0)])[0].window_bins == 159
    lone.close()


# ---- 3. rings ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [16, 8])
def test_integer_rings(gctx, small, bits):
    import gnsscorr
    blk, fd, _, _ = small
    q, xq = fc.quantise(blk.x, bits)
    recs = fc.records(blk, ref.EXACT, key="i%d" % bits, x=xq)
    ring, first = ring_of(gctx, q, lead=3, iq_format=gnsscorr.GC_IQ_I16 if bits == 16 else gnsscorr.GC_IQ_I8)
    assert first == 3
    res = fd.estimate_stream(ring, first, blk.requests)
    check_all(fd, res, recs)
    spec = [fd.spectrum(i).tobytes() for i in range(6)]
    # the same values as float32 samples: the same bits
    ring_f, first_f = ring_of(gctx, xq, lead=2)
    res_f = fd.estimate_stream(ring_f, first_f, blk.requests)
    assert [fc.result_bits(r) for r in res_f] == [fc.result_bits(r) for r in res]
    assert [fd.spectrum(i).tobytes() for i in range(6)] == spec
    ring.close()
    ring_f.close()


def test_block_that_wraps_the_rings_end(gctx, small):
    blk, fd, ring0, first0 = small
    want = fd.estimate_stream(ring0, first0, blk.requests)
    want_spec = [fd.spectrum(i).tobytes() for i in range(6)]
    n = fd.block_samples
    # capacity n + 101, 12345 samples in front: the block starts at 12345 and its last 12244 samples lie at the ring's start
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=n + 101, max_window_samples=64)
    lead = np.zeros(12345, np.complex64)
    ring.push(lead)
    first = ring.push(blk.x)
    assert first == 12345 and first + n > n + 101
    res = fd.estimate_stream(ring, first, blk.requests)
    check_all(fd, res, fc.records(blk, ref.EXACT))
    assert [fc.result_bits(r) for r in res] == [fc.result_bits(r) for r in want]
    assert [fd.spectrum(i).tobytes() for i in range(6)] == want_spec
    ring.close()


def test_block_that_is_not_resident_is_refused(gctx, small):
    import gnsscorr
    blk, fd, ring0, first0 = small
    before = fd.estimate_stream(ring0, first0, blk.requests[:2])
    spec = fd.spectrum(1).tobytes()
    n = fd.block_samples
    ring = gnsscorr.IqStream(gctx, capacity_samples=n + 100, max_window_samples=64)
    first = ring.push(blk.x)
    # its end has not been pushed yet
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        fd.estimate_stream(ring, first + 1, blk.requests[:2])
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "resident" in str(e.value)
    # its first samples have been evicted
    ring.push(np.zeros(200, np.complex64))
    oldest, head, cap = ring.info()
    assert oldest == 100 and head == n + 200
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        fd.estimate_stream(ring, first, blk.requests[:2])
    assert e.value.status in (gnsscorr.GC_ERR_STATE, gnsscorr.GC_ERR_INVALID)
    # nothing was enqueued and no read of the ring is left reserved: the last results are untouched, the ring takes a push that evicts
    # everything, and a resident block is served
    assert fd.spectrum(1).tobytes() == spec
    ring.push(np.zeros(n + 100, np.complex64))
    at = ring.push(blk.x[:n // 2])
    ring.push(blk.x[n // 2:])
    res = fd.estimate_stream(ring, at, blk.requests[:2])
    assert [fc.result_bits(r) for r in res] == [fc.result_bits(r) for r in before]
    ring.close()


def test_host_pointer_call_equals_the_stream_call(small):
    blk, fd, ring, first = small
    a = fd.estimate_stream(ring, first, blk.requests)
    spec = [fd.spectrum(i).tobytes() for i in range(6)]
    b = fd.estimate(blk.x, blk.requests)
    check_all(fd, b, fc.records(blk, ref.EXACT))
    assert [fc.result_bits(r) for r in a] == [fc.result_bits(r) for r in b]
    assert [fd.spectrum(i).tobytes() for i in range(6)] == spec


def test_all_zero_block(gctx, small):
    import gnsscorr
    blk, fd, _, _ = small
    res = fd.estimate(np.zeros(fd.block_samples, np.complex64), blk.requests)
    for r, (slot, s, coarse) in zip(res, blk.requests):
        first, count = ref.window(blk.fs, fd.next_size, coarse)
        run = (first + np.arange(count)) % fd.next_size
        assert (r.window_first_bin, r.window_bins) == (first, count)
        assert r.peak == 0.0 and r.mean == 0.0 and r.bin == run.min()
        assert np.isfinite(r.doppler_hz) and fc.f32_bits(r.doppler_hz) == fc.f32_bits(ref.freq_table(blk.fs, fd.next_size)[r.bin])
    assert res[0].bin == 0 and res[0].doppler_hz == 0.0 and res[0].status == gnsscorr.FINE_REFINED
    assert res[2].bin == res[2].window_first_bin and res[2].status == gnsscorr.FINE_EDGE
    for i in range(6):
        p = fd.spectrum(i)
        assert p.size == res[i].window_bins and not np.any(p) and np.all(np.isfinite(p))
