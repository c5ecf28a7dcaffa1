"""GPU tests of the ring decimator (gc_ring_decimator_*): the FIR decimator that derives a GC_IQ_F32 ring from another ring on the
device -- the acquisition resampler.  Its definition is the conditioner's with translate_hz = 0; tests/conditioner_ref.py restates
it in float64 and error_bound is the (T + 16) 2^-23 sum|h| max|x| DESIGN.md derives."""
import numpy as np
import pytest

import conditioner_ref
from helpers import synth_stream

pytestmark = pytest.mark.gpu
FS_IN = 16e6
SRC_CAP = 4099  # prime: a multiple of neither 8 samples nor any decimation
PIECES = [1000, 37, 2500, 1, 811, 1999]  # each piece + T - 1 + D stays below the source ring's capacity


def _taps(T, D, seed=5):
    """A low-pass for the decimated band with a little seeded asymmetry (a symmetric filter would hide a reversed tap order)."""
    if T == 1:
        return np.ones(1, np.float32)
    k = np.arange(T) - (T - 1) / 2.0
    h = np.sinc(k * 0.8 / D) * np.hamming(T)
    h = h / h.sum() + np.random.Generator(np.random.PCG64(seed)).standard_normal(T) * 1e-3
    return h.astype(np.float32)


def _raw(n, fmt, seed, tone_hz=1.3e6):
    """Seeded noise plus a tone, in the ring's layout: complex64 [n] or int16 / int8 [n, 2]."""
    import gnsscorr
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5) + 2.0 * np.exp(2j * np.pi * tone_hz * np.arange(n) / FS_IN + 0.3j)
    if fmt == gnsscorr.GC_IQ_F32:
        return x.astype(np.complex64)
    scale, dt, lim = (1000.0, np.int16, 32767) if fmt == gnsscorr.GC_IQ_I16 else (20.0, np.int8, 127)
    return np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -lim, lim).astype(dt)


def _fmt(name):
    import gnsscorr
    return getattr(gnsscorr, "GC_IQ_" + name)


def _run(gctx, raw, fmt, D, taps, sizes, src_cap=SRC_CAP, out_cap=1 << 14, out_win=64, update_each=True):
    """Pushes `raw` into a plain ring in pieces of `sizes` (repeated), updates the decimator after every piece (or once at the end)
    and reads every resident output back."""
    import gnsscorr
    src = gnsscorr.IqStream(gctx, capacity_samples=src_cap, max_window_samples=64, iq_format=fmt)
    out = gnsscorr.IqStream(gctx, capacity_samples=out_cap, max_window_samples=out_win)
    dec = gnsscorr.RingDecimator(gctx, src, D, taps, out)
    pos, k, made = 0, 0, 0
    while pos < len(raw):
        m = min(sizes[k % len(sizes)], len(raw) - pos)
        k += 1
        src.push(raw[pos:pos + m])
        pos += m
        if update_each or pos == len(raw):
            first, n_out = dec.update()
            assert first == made and first + n_out == (pos + D - 1) // D
            made += n_out
            assert dec.info() == (pos, made) and out.info()[1] == made
    oldest, head, _ = out.info()
    y = out.read(oldest, head - oldest)
    dec.close()
    out.close()
    src.close()
    return oldest, y


def _check(y, ref, bound, what):
    err = max(np.abs(y.real - ref.real).max(), np.abs(y.imag - ref.imag).max())
    print("%s: max component error %.3e, bound %.3e (%.4f of it)" % (what, err, bound, err / bound if bound > 0 else 0.0))
    assert err <= bound


@pytest.mark.parametrize("D, T", [(1, 1), (4, 97), (5, 32), (25, 603), (64, 1024)])
@pytest.mark.parametrize("fmt_name", ["F32", "I16", "I8"])
def test_values_against_the_float64_restatement(gctx, fmt_name, D, T):
    """A source ring of 4099 samples that wraps twice, pushed in uneven pieces with an update after each; the outputs before
    m = ceil((T - 1) / D) see x[n] = 0 for n < 0.  D = 1, h = {1} is a bit-exact copy of the converted source."""
    fmt = _fmt(fmt_name)
    raw = _raw(9001, fmt, seed=300 + D)
    taps = _taps(T, D)
    oldest, y = _run(gctx, raw, fmt, D, taps, PIECES)
    assert oldest == 0 and len(y) == (len(raw) + D - 1) // D and y.dtype == np.complex64
    ref = conditioner_ref.condition(raw, taps, D, 0.0, FS_IN)
    _check(y, ref, conditioner_ref.error_bound(taps, raw), "ring decimator %s D=%d T=%d" % (fmt_name, D, T))
    if (D, T) == (1, 1):
        assert np.array_equal(y, conditioner_ref.to_complex(raw).astype(np.complex64))


@pytest.mark.parametrize("D, T", [(4, 97), (25, 603)])
@pytest.mark.parametrize("fmt_name", ["F32", "I16", "I8"])
def test_bits_equal_the_conditioner_without_translation(gctx, fmt_name, D, T):
    import gnsscorr
    fmt = _fmt(fmt_name)
    raw = _raw(9001, fmt, seed=41)
    taps = _taps(T, D)
    ring = gnsscorr.IqStream(gctx, capacity_samples=1 << 14, max_window_samples=64)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, D, taps, fmt)
    cond.push(raw)
    n = (len(raw) + D - 1) // D
    want = ring.read(0, n)
    cond.close()
    ring.close()
    oldest, got = _run(gctx, raw, fmt, D, taps, PIECES)
    assert oldest == 0 and len(got) == n
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("fmt_name, D, T", [("F32", 5, 32), ("I16", 25, 603)])
def test_bits_do_not_depend_on_how_the_source_is_cut(gctx, fmt_name, D, T):
    """One update after everything has been pushed against an update after every push of 1, 7, 333 or 1000 samples; with pushes of
    1 or 7 samples most updates complete no output."""
    fmt = _fmt(fmt_name)
    raw = _raw(3001, fmt, seed=77)
    taps = _taps(T, D)
    _, whole = _run(gctx, raw, fmt, D, taps, [1000], src_cap=1 << 13, update_each=False)
    assert len(whole) == (len(raw) + D - 1) // D
    for size in (1, 7, 333, 1000):
        _, cut = _run(gctx, raw, fmt, D, taps, [size], src_cap=1 << 13)
        assert cut.tobytes() == whole.tobytes(), size


def test_output_ring_wrap(gctx):
    """An output ring of 257 samples (max_window 64) that wraps three times: every resident window, read across the wrap, equals
    the restatement; and one update that completes more than 257 outputs leaves the newest 257 correct."""
    import gnsscorr
    D, T, fmt = 4, 97, _fmt("I16")
    raw = _raw(3701, fmt, seed=9)
    taps = _taps(T, D)
    ref = conditioner_ref.condition(raw, taps, D, 0.0, FS_IN)
    bound = conditioner_ref.error_bound(taps, raw)
    src = gnsscorr.IqStream(gctx, capacity_samples=SRC_CAP, max_window_samples=64, iq_format=fmt)
    out = gnsscorr.IqStream(gctx, capacity_samples=257, max_window_samples=64)
    dec = gnsscorr.RingDecimator(gctx, src, D, taps, out)
    pos = 0
    for m in (700, 333, 1000, 68, 900, 700):
        src.push(raw[pos:pos + m])
        pos += m
        dec.update()
        oldest, head, _ = out.info()
        assert head == (pos + D - 1) // D and oldest == max(0, head - 257)
        _check(out.read(oldest, head - oldest), ref[oldest:head], bound, "output ring [%d, %d)" % (oldest, head))
    assert pos == len(raw) and head > 3 * 257
    dec.close()
    out.close()
    src.close()
    src = gnsscorr.IqStream(gctx, capacity_samples=1 << 13, max_window_samples=64, iq_format=fmt)
    out = gnsscorr.IqStream(gctx, capacity_samples=257, max_window_samples=64)
    dec = gnsscorr.RingDecimator(gctx, src, D, taps, out)
    src.push(raw)
    assert dec.update() == (0, len(ref)) and len(ref) > 3 * 257
    oldest, head, _ = out.info()
    assert (oldest, head) == (len(ref) - 257, len(ref))
    _check(out.read(oldest, 257), ref[oldest:head], bound, "one update of %d outputs into 257" % len(ref))
    dec.close()
    out.close()
    src.close()


def _chain(gctx, raw, h1, h2, f, sizes):
    import gnsscorr
    mid = gnsscorr.IqStream(gctx, capacity_samples=SRC_CAP, max_window_samples=64)
    cond = gnsscorr.Conditioner(gctx, mid, FS_IN, f, 5, h1, gnsscorr.GC_IQ_I16)
    out = gnsscorr.IqStream(gctx, capacity_samples=1 << 12, max_window_samples=64)
    dec = gnsscorr.RingDecimator(gctx, mid, 5, h2, out)
    pos, k = 0, 0
    while pos < len(raw):
        m = min(sizes[k % len(sizes)], len(raw) - pos)
        k += 1
        cond.push(raw[pos:pos + m])
        pos += m
        dec.update()
    n = -(-(-(-len(raw) // 5)) // 5)
    assert out.info()[:2] == (0, n)
    y = out.read(0, n)
    dec.close()
    cond.close()
    out.close()
    mid.close()
    return y


def test_chained_behind_a_conditioner(gctx):
    """cshort conditioner (D = 5, translation) -> ring -> decimator (D = 5): condition() of condition() within the sum of the two
    bounds, and the same bits for other push sizes."""
    import gnsscorr
    f = -3.1e6
    raw = _raw(30011, gnsscorr.GC_IQ_I16, seed=13)
    h1, h2 = _taps(64, 5), _taps(32, 5, seed=6)
    y = _chain(gctx, raw, h1, h2, f, [3001, 17, 5000, 1, 4999])
    mid_ref = conditioner_ref.condition(raw, h1, 5, f, FS_IN)
    ref = conditioner_ref.condition(mid_ref, h2, 5, 0.0, FS_IN)
    bound = conditioner_ref.error_bound(h1, raw) + conditioner_ref.error_bound(h2, mid_ref)
    _check(y, ref, bound, "conditioner -> ring -> decimator")
    assert _chain(gctx, raw, h1, h2, f, [4000, 333]).tobytes() == y.tobytes()


def test_eviction_and_state(gctx):
    import ctypes as C
    import gnsscorr
    lib = gnsscorr.load_library()
    fmt = _fmt("I16")
    raw = _raw(3 * 1024, fmt, seed=3)
    taps = _taps(33, 4)
    src = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=fmt)
    out = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    dec = gnsscorr.RingDecimator(gctx, src, 4, taps, out)
    src.push(raw[:1000])
    assert dec.update() == (0, 250) and dec.info() == (1000, 250)
    # a push to the output ring is refused
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        out.push(np.zeros(8, np.complex64))
    assert e.value.status == gnsscorr.GC_ERR_STATE
    # the source runs more than its capacity ahead: sample 250 * 4 - 32 is gone
    src.push(raw[1000:2000])
    src.push(raw[2000:3000])
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        dec.update()
    assert e.value.status == gnsscorr.GC_ERR_STATE
    assert dec.info() == (1000, 250) and out.info()[:2] == (0, 250)
    # a decimator on a ring that has lost sample 0
    out2 = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.RingDecimator(gctx, src, 4, taps, out2)
    assert e.value.status == gnsscorr.GC_ERR_STATE
    # host-side argument checks with live handles
    fresh = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=fmt)
    out_i16 = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=fmt)  # empty, but not GC_IQ_F32
    h = C.c_void_p()
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    # each call is wrong in ONE way, and the message names the check that refused it
    for args in ((0, tp, 33, out2, "decimation 0"), (65, tp, 33, out2, "decimation 65"), (4, tp, 0, out2, "0 taps"), (4, tp, 1025, out2, "1025 taps"),
            (4, None, 33, out2, "NULL taps"), (4, tp, 33, out_i16, "must be GC_IQ_F32"), (4, tp, 33, out, "pushed into the output ring already"),
            (4, tp, 33, fresh, "the same ring")):
        D, t, n, ring, word = args
        assert lib.gc_ring_decimator_create(gctx._h, fresh._h, D, t, n, ring._h, C.byref(h)) == gnsscorr.GC_ERR_INVALID, args[:3]
        assert word in lib.gc_last_error().decode(), (word, lib.gc_last_error().decode())
        assert not h.value
    out_i16.close()
    # out2 is still a plain ring: nothing above made it kernel-fed
    out2.push(np.zeros(8, np.complex64))
    dec.close()
    for r in (fresh, out2, out, src):
        r.close()


def _numpy_pcps(block, code, fs, doppler_max, step):
    """(delay, doppler) of the PCPS peak of one code period, float64."""
    n = np.arange(len(block))
    cf = np.conj(np.fft.fft(code))
    best = (-1.0, 0, 0)
    for fd in range(-doppler_max, doppler_max, step):
        g = np.abs(np.fft.ifft(np.fft.fft(block * np.exp(-2j * np.pi * fd * n / fs)) * cf)) ** 2
        i = int(np.argmax(g))
        if g[i] > best[0]:
            best = (float(g[i]), i, fd)
    return best[1], best[2]


def _wrap(d, period):
    return (d + period / 2.0) % period - period / 2.0


def test_acquisition_on_the_derived_ring(gctx):
    """GPS L1 at 4 Msps, three satellites at 52-55 dB-Hz: the 1 Msps search (N = 1000) on the derived ring finds each of them, the
    Doppler within one step of the full-rate search and delay * D - latency within D source samples of the full-rate delay (the
    derived grid's spacing is D source samples; the group delay of the odd symmetric filter is exactly (T - 1) / 2).  The float64
    restatement (condition() + a numpy PCPS) must detect all three within D / 2 of the truth first.  The derived ring holds 2048
    samples and the searched window [3600, 4600) crosses its end (4096): the search reads the mirror the decimator's kernel wrote."""
    import gnsscorr
    fs, prns, step = 4_000_000, [3, 11, 27], 250
    codes = [gnsscorr.gps_l1_ca_code_gen_float(p) for p in prns]
    x, truth = synth_stream(codes, fs, 20000, seed=2024, cn0_db_hz=(52.0, 55.0))
    D, rfs, taps, latency = gnsscorr.acq_resampler_plan(fs, 1_000_000)
    assert (D, rfs, len(taps), latency) == (4, 1_000_000, 97, 48)
    first = 14400  # source index of the searched block; derived index 3600
    true_delay = [((1023.0 - t["tau0"]) / (t["code_rate"] / fs) - first) % 4000.0 for t in truth]
    # replicas sampled the way synth_stream samples the signal, chip floor(i * chip_rate / fs): the reference's generator takes chip
    # ceil((i + 1) chip_rate / fs) - 1, which advances a replica by up to one sample OF ITS RATE (one at 4 Msps, four source samples at
    # 1 Msps) and would add that difference to the comparison below, on top of the grid spacing the bound is derived from
    def replica(code, rate, n):
        return np.asarray(code, np.float32)[np.floor(np.arange(n) * (1.023e6 / rate)).astype(np.int64) % 1023].astype(np.complex64)
    sampled = [replica(c, rfs, 1000) for c in codes]
    y64 = conditioner_ref.condition(x, taps, D, 0.0, fs)
    for s in range(3):
        delay, fd = _numpy_pcps(y64[first // D:first // D + 1000], sampled[s][:1000], rfs, 5000, step)
        off = _wrap(delay * D - latency - true_delay[s], 4000.0)
        print("restatement PRN %d: delay %d -> %.1f source samples from the truth, Doppler %d (truth %.0f)" % (prns[s], delay, off, fd, truth[s]["doppler"]))
        assert abs(off) <= D / 2 and abs(fd - truth[s]["doppler"]) <= step

    src = gnsscorr.IqStream(gctx, capacity_samples=1 << 15, max_window_samples=4000)
    out = gnsscorr.IqStream(gctx, capacity_samples=2048, max_window_samples=1000)
    dec = gnsscorr.RingDecimator(gctx, src, D, taps, out)
    src.push(x[:7001])
    dec.update()
    src.push(x[7001:])
    assert dec.update() == (1751, 5000 - 1751)
    full = gnsscorr.PcpsAcquisition(gctx, 3, fs, 1, 1, np.float32(fs) * np.float32(0.001), 4000.0, 4, 5000, step)
    res = gnsscorr.PcpsAcquisition(gctx, 3, rfs, 1, 1, np.float32(rfs) * np.float32(0.001), 1000.0, 1, 5000, step)
    assert res.fft_size == 1000
    for s, p in enumerate(prns):
        full.set_local_code(s, replica(codes[s], fs, 4000))
        res.set_local_code(s, sampled[s])
    rf = full.dwell_stream(src, first)
    rr = res.dwell_stream(out, first // D)
    # the same block handed over from the host: what the search read through the mirror is what the ring holds
    res.reset()
    rh = res.dwell(out.read(first // D, 1000))
    for s in range(3):
        print("PRN %d: full rate delay %.0f Doppler %d stat %.4f; derived delay %.0f Doppler %d stat %.4f" % (prns[s], rf[s].acq_delay_samples,
            rf[s].doppler_hz, rf[s].test_statistics, rr[s].acq_delay_samples, rr[s].doppler_hz, rr[s].test_statistics))
        assert abs(_wrap(rf[s].acq_delay_samples - true_delay[s], 4000.0)) <= 1.0
        assert rr[s].test_statistics > 20.0 / 1000.0  # noise cells average 1 / N, the largest of 40 x 1000 about ln(40000) / N = 11 / N
        assert abs(rr[s].doppler_hz - rf[s].doppler_hz) <= step
        assert abs(_wrap(rr[s].acq_delay_samples * D - latency - rf[s].acq_delay_samples, 4000.0)) <= D
        assert (rh[s].indext, rh[s].doppler_hz) == (rr[s].indext, rr[s].doppler_hz)
        assert abs(rh[s].test_statistics - rr[s].test_statistics) <= 1e-5 * rr[s].test_statistics
    # What a user of PcpsAcquisition does: the library's own generator at both rates (the reference's, chip
    # ceil((i + 1) chip_rate / fs) - 1).  It advances the 1 Msps replica by up to one derived sample (D source samples) and the
    # 4 Msps replica by up to one source sample, so the bound is the D of above plus that D: 2 D.
    for s, p in enumerate(prns):
        full.set_local_code(s, gnsscorr.gps_l1_ca_code_gen_complex_sampled(p, fs))
        res.set_local_code(s, gnsscorr.gps_l1_ca_code_gen_complex_sampled(p, rfs))
    full.reset()
    res.reset()
    rf = full.dwell_stream(src, first)
    rr = res.dwell_stream(out, first // D)
    for s in range(3):
        diff = _wrap(rr[s].acq_delay_samples * D - latency - rf[s].acq_delay_samples, 4000.0)
        print("PRN %d, the library's replicas: full rate delay %.0f, derived delay %.0f -> %.0f source samples apart, stat %.4f" % (prns[s],
            rf[s].acq_delay_samples, rr[s].acq_delay_samples, diff, rr[s].test_statistics))
        assert rr[s].test_statistics > 20.0 / 1000.0 and abs(rr[s].doppler_hz - rf[s].doppler_hz) <= step
        assert abs(diff) <= 2 * D
    for h in (full, res, dec, out, src):
        h.close()


@pytest.mark.parametrize("fs, ms, n_fft", [(1_000_000, 1, 1000), (2_500_000, 4, 10000), (12_500_000, 1, 12500)])
def test_acquisition_engine_accepts_the_transform_sizes_of_the_plans(gctx, fs, ms, n_fft):
    """gc_acq_create itself at the rates the plans lead to: GPS L1 at 1 Msps, Galileo E1 (4 ms) at 2.5 Msps, L5 / E5a at 12.5 Msps."""
    import gnsscorr
    acq = gnsscorr.PcpsAcquisition(gctx, 1, fs, ms, ms, np.float32(fs) * np.float32(0.001), float(n_fft), max(1, -(-fs // 1_023_000)), 5000, 250)
    assert (acq.fft_size, acq.consumed_samples) == (n_fft, n_fft)
    acq.close()
