"""GPU tests of the ring resampler (gc_ring_resampler_*): a ring derived on the device from another ring at an arbitrary rate ratio,
in direct mode (the reference's Direct_Resampler: nearest earlier sample, bits as they are) and in polyphase mode (one of P tap
rows per output).  tests/resampler_ref.py restates both -- exact integers for the picks and the head counts, float64 for the filter
-- and error_bound is the (T + 16) 2^-23 max_p sum_k |H[p][k]| max|x| DESIGN.md section 3.3 derives for this accumulation."""
import numpy as np
import pytest

import conditioner_ref
import resampler_ref

pytestmark = pytest.mark.gpu
SRC_CAP = 4099  # prime: a multiple of neither 8 samples nor any ratio
PIECES = [1000, 37, 2500, 1, 811, 1999]  # each piece + T - 1 stays below the source ring's capacity
N_RAW = 9001
DIRECT_PAIRS = [(25e6, 10e6), (6.625e6, 2.5e6), (64e6, 1e6), (4e6, 4e6), (4e6, 5e6), (2.5e6, 6.625e6)]
POLY_CASES = ["25-10", "6.625-4", "4-5", "64-1", "4-4"]


def _fmt(name):
    import gnsscorr
    return getattr(gnsscorr, "GC_IQ_" + name)


def _raw(n, fmt, seed, fs=16e6, tone_hz=1.3e6):
    """Seeded noise plus a tone, in the ring's layout: complex64 [n] or int16 / int8 [n, 2]."""
    import gnsscorr
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5) + 2.0 * np.exp(2j * np.pi * tone_hz * np.arange(n) / fs + 0.3j)
    if fmt == gnsscorr.GC_IQ_F32:
        return x.astype(np.complex64)
    scale, dt, lim = (1000.0, np.int16, 32767) if fmt == gnsscorr.GC_IQ_I16 else (20.0, np.int8, 127)
    return np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -lim, lim).astype(dt)


_BANKS = {}


def _poly_case(name):
    """(fs_in, fs_out, bank [P, T]) of a polyphase case; made once."""
    import gnsscorr
    if name not in _BANKS:
        rng = np.random.Generator(np.random.PCG64(1234))
        if name == "25-10":
            case = (25e6, 10e6, gnsscorr.resampler_design(25e6, 10e6, 32))
        elif name == "6.625-4":
            case = (6.625e6, 4e6, gnsscorr.resampler_design(6.625e6, 4e6, 64))
        elif name == "4-5":
            # seeded and asymmetric: a reversed tap order or a swapped phase index shows
            case = (4e6, 5e6, (rng.standard_normal((16, 12)) / 4.0).astype(np.float32))
        elif name == "64-1":
            case = (64e6, 1e6, (rng.standard_normal((4, 1024)) / 32.0).astype(np.float32))
        else:
            case = (4e6, 4e6, np.ones((1, 1), np.float32))
        _BANKS[name] = case
    return _BANKS[name]


def _ratio(mode, fs_in, fs_out):
    return resampler_ref.direct_ratio(fs_in, fs_out) if mode == "direct" else resampler_ref.poly_ratio(fs_in, fs_out)


def _run(gctx, raw, fmt, fs_in, fs_out, mode, bank, sizes, src_cap=SRC_CAP, out_cap=1 << 15, out_win=64, update_each=True):
    """Pushes `raw` into a plain ring in pieces of `sizes` (repeated), updates the resampler after every piece (or once at the end),
    checks first / n_out / info() against the head-count formula and reads every resident output back."""
    import gnsscorr
    kind, step = _ratio(mode, fs_in, fs_out)
    src = gnsscorr.IqStream(gctx, capacity_samples=src_cap, max_window_samples=64, iq_format=fmt)
    out = gnsscorr.IqStream(gctx, capacity_samples=out_cap, max_window_samples=out_win, iq_format=fmt if mode == "direct" else gnsscorr.GC_IQ_F32)
    res = gnsscorr.RingResampler(gctx, src, fs_in, fs_out, out, mode, bank)
    assert res.update() == (0, 0) and res.info() == (0, 0)  # an empty source completes nothing
    pos, k, made = 0, 0, 0
    while pos < len(raw):
        m = min(sizes[k % len(sizes)], len(raw) - pos)
        k += 1
        src.push(raw[pos:pos + m])
        pos += m
        if update_each or pos == len(raw):
            before = out.info()
            first, n_out = res.update()
            want = resampler_ref.available(kind, step, pos)
            assert (first, first + n_out) == (made, want), (pos, first, n_out, want)
            if n_out == 0:
                assert out.info() == before
            made += n_out
            assert res.info() == (pos, made) and out.info()[1] == made
    oldest, head, _ = out.info()
    y = out.read(oldest, head - oldest)
    res.close()
    out.close()
    src.close()
    return oldest, y


def _check(y, ref, bound, what):
    err = max(np.abs(y.real - ref.real).max(), np.abs(y.imag - ref.imag).max())
    print("%s: max component error %.3e, bound %.3e (%.4f of it)" % (what, err, bound, err / bound if bound > 0 else 0.0))
    assert err <= bound


@pytest.mark.parametrize("fs_in, fs_out", DIRECT_PAIRS)
@pytest.mark.parametrize("fmt_name", ["F32", "I16", "I8"])
def test_direct_outputs_are_the_picked_source_samples(gctx, fmt_name, fs_in, fs_out):
    """A source ring of 4099 samples that wraps twice, pushed in uneven pieces with an update after each: the output bytes are
    raw[n_m] for every available m, and every update's first / n_out / info() are the head-count formula's.  With 64 -> 1 the
    one-sample piece (head 3537 -> 3538) completes nothing and changes nothing."""
    fmt = _fmt(fmt_name)
    raw = _raw(N_RAW, fmt, seed=500 + int(fs_in / 1e5))
    oldest, y = _run(gctx, raw, fmt, fs_in, fs_out, "direct", None, PIECES)
    want = resampler_ref.direct(raw, fs_in, fs_out)
    assert oldest == 0 and y.dtype == raw.dtype and y.shape == want.shape and len(want) > 0
    assert y.tobytes() == want.tobytes()
    if (fs_in, fs_out) == (64e6, 1e6):
        kind, step = resampler_ref.direct_ratio(fs_in, fs_out)
        assert resampler_ref.available(kind, step, 3537) == resampler_ref.available(kind, step, 3538)


def test_direct_refuses_an_output_ring_of_another_format(gctx):
    import gnsscorr
    src = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=gnsscorr.GC_IQ_I16)
    for fmt in (gnsscorr.GC_IQ_F32, gnsscorr.GC_IQ_I8):
        out = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=fmt)
        with pytest.raises(gnsscorr.GnsscorrError) as e:
            gnsscorr.RingResampler(gctx, src, 25e6, 10e6, out)
        assert e.value.status == gnsscorr.GC_ERR_INVALID and "source ring's format" in str(e.value)
        out.push(np.zeros((8, 2), np.int8) if fmt == gnsscorr.GC_IQ_I8 else np.zeros(8, np.complex64))  # still a plain ring
        out.close()
    # polyphase mode: GC_IQ_F32 only, whatever the source
    out = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=gnsscorr.GC_IQ_I16).accept_quantised_output()
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.RingResampler(gctx, src, 25e6, 10e6, out, "polyphase", np.ones((2, 4), np.float32))
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "GC_IQ_F32 output ring only" in str(e.value)
    out.close()
    src.close()


@pytest.mark.parametrize("case", POLY_CASES)
@pytest.mark.parametrize("fmt_name", ["F32", "I16", "I8"])
def test_polyphase_values_against_the_float64_restatement(gctx, fmt_name, case):
    """The same pushes; the outputs whose window starts before sample 0 see zeros there.  P = T = 1, H = {1} at equal rates is a
    bit-exact copy of the converted source."""
    fmt = _fmt(fmt_name)
    fs_in, fs_out, bank = _poly_case(case)
    raw = _raw(N_RAW, fmt, seed=700 + len(case))
    oldest, y = _run(gctx, raw, fmt, fs_in, fs_out, "polyphase", bank, PIECES)
    ref = resampler_ref.polyphase(raw, bank, fs_in, fs_out)
    assert oldest == 0 and y.dtype == np.complex64 and len(y) == len(ref) > 0
    _check(y, ref, resampler_ref.error_bound(bank, raw), "ring resampler %s %s P=%d T=%d" % (fmt_name, case, bank.shape[0], bank.shape[1]))
    if case == "4-4":
        assert np.array_equal(y, conditioner_ref.to_complex(raw).astype(np.complex64))


@pytest.mark.parametrize("mode, case", [("direct", "25-10"), ("direct", "4-5"), ("polyphase", "25-10"), ("polyphase", "4-5")])
@pytest.mark.parametrize("fmt_name", ["F32", "I16"])
def test_bits_do_not_depend_on_how_the_source_is_cut(gctx, fmt_name, mode, case):
    """The uneven pieces with an update after each, one push and one update, and pushes of 1 .. 7 samples (most of whose updates
    complete nothing, or one output) leave byte-equal output rings."""
    fmt = _fmt(fmt_name)
    fs_in, fs_out, bank = _poly_case(case)
    bank = bank if mode == "polyphase" else None
    raw = _raw(N_RAW, fmt, seed=77)
    _, pieces = _run(gctx, raw, fmt, fs_in, fs_out, mode, bank, PIECES)
    _, whole = _run(gctx, raw, fmt, fs_in, fs_out, mode, bank, [N_RAW], src_cap=1 << 14, update_each=False)
    _, small = _run(gctx, raw, fmt, fs_in, fs_out, mode, bank, [1, 2, 3, 4, 5, 6, 7])
    assert len(whole) == resampler_ref.available(*_ratio(mode, fs_in, fs_out), N_RAW)
    assert pieces.tobytes() == whole.tobytes()
    assert small.tobytes() == whole.tobytes()


@pytest.mark.parametrize("mode", ["direct", "polyphase"])
def test_output_ring_wrap_and_mirror(gctx, mode):
    """An output ring of 1024 samples (max_window 64) receives about 3600 outputs in ONE update: the resident 1024 equal the restatement; a
    window read across the ring's end equals one that does not cross it; and a correlator with an all-ones replica, whose window
    [wrap - 30, wrap + 30) is contiguous only through the mirror, sums what the ring holds -- the kernel stored the mirror."""
    import gnsscorr
    fs_in, fs_out, bank = _poly_case("25-10")
    fmt = gnsscorr.GC_IQ_F32
    raw = _raw(N_RAW, fmt, seed=9)
    if mode == "direct":
        ref, bound, bank = resampler_ref.direct(raw, fs_in, fs_out).astype(np.complex128), 0.0, None
    else:
        ref, bound = resampler_ref.polyphase(raw, bank, fs_in, fs_out), resampler_ref.error_bound(bank, raw)
    cap = 1024
    src = gnsscorr.IqStream(gctx, capacity_samples=1 << 14, max_window_samples=64, iq_format=fmt)
    out = gnsscorr.IqStream(gctx, capacity_samples=cap, max_window_samples=64)
    res = gnsscorr.RingResampler(gctx, src, fs_in, fs_out, out, mode, bank)
    src.push(raw)
    assert res.update() == (0, len(ref)) and len(ref) > 3 * cap
    oldest, head, _ = out.info()
    assert (oldest, head) == (len(ref) - cap, len(ref))
    _check(out.read(oldest, cap), ref[oldest:head], bound, "%s: one update of %d outputs into %d" % (mode, len(ref), cap))
    wrap = 3 * cap  # absolute output 3072 sits at ring position 0
    assert oldest < wrap - 100 and wrap + 100 < head
    across, inside = out.read(wrap - 30, 60), out.read(wrap, 30)
    _check(across, ref[wrap - 30:wrap + 30], bound, "%s: window across the wrap" % mode)
    assert across[30:].tobytes() == inside.tobytes()
    b = gnsscorr.TrackingBatch(gctx, 1, 3, 8)
    b.set_code(0, np.ones(8, np.float32), np.zeros(3, np.float32))
    b.set_input_stream(0, out)
    got = complex(b.run(1, gnsscorr.epoch_params_array([gnsscorr.epoch_params(wrap - 30, 0.0, 0.0, 0.0, 0.001, 60)]))[0, 0, 1])
    want = across.astype(np.complex128).sum()
    tol = (60 + 8) * 2.0 ** -24 * np.abs(across).sum() * np.sqrt(2.0)  # the correlator's own float32 sum of 60 stored values
    print("%s: window sum through the mirror: |diff| %.3e, tolerance %.3e, |sum| %.3e" % (mode, abs(got - want), tol, abs(want)))
    assert abs(got.real - want.real) <= tol and abs(got.imag - want.imag) <= tol
    assert np.abs(across[30:]).sum() > 100 * tol  # a stale or missing mirror (zeros) would be far outside
    b.close()
    res.close()
    out.close()
    src.close()


@pytest.mark.parametrize("mode", ["direct", "polyphase"])
def test_eviction_and_state(gctx, mode):
    """A source that runs more than its capacity ahead: GC_ERR_STATE with info() unchanged; a rebuilt resampler (fresh rings) works
    again.  The output ring refuses pushes while the resampler lives and takes them again afterwards."""
    import gnsscorr
    fs_in, fs_out, bank = _poly_case("25-10")
    bank = bank if mode == "polyphase" else None
    fmt = gnsscorr.GC_IQ_F32
    raw = _raw(3 * 1024, fmt, seed=3)
    kind, step = _ratio(mode, fs_in, fs_out)
    src = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=fmt)
    out = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    res = gnsscorr.RingResampler(gctx, src, fs_in, fs_out, out, mode, bank)
    src.push(raw[:1000])
    n0 = resampler_ref.available(kind, step, 1000)
    assert res.update() == (0, n0) and res.info() == (1000, n0)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        out.push(np.zeros(8, np.complex64))
    assert e.value.status == gnsscorr.GC_ERR_STATE
    # a second producer on the same output ring, and an output ring that already holds samples
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.RingResampler(gctx, src, fs_in, fs_out, out, mode, bank)
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "pushed into the output ring already" in str(e.value)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.RingResampler(gctx, src, fs_in, fs_out, src, mode, bank)
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "the same ring" in str(e.value)
    src.push(raw[1000:2000])
    src.push(raw[2000:3000])
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        res.update()
    assert e.value.status == gnsscorr.GC_ERR_STATE
    assert res.info() == (1000, n0) and out.info()[:2] == (0, n0)
    # a resampler on a ring that has lost sample 0
    out2 = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        gnsscorr.RingResampler(gctx, src, fs_in, fs_out, out2, mode, bank)
    assert e.value.status == gnsscorr.GC_ERR_STATE
    out2.push(np.zeros(8, np.complex64))  # nothing above made out2 kernel-fed
    res.close()
    out.push(np.zeros(8, np.complex64))  # released for pushes again
    for r in (out2, out, src):
        r.close()
    # rebuilt on fresh rings
    src = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=fmt)
    out = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    res = gnsscorr.RingResampler(gctx, src, fs_in, fs_out, out, mode, bank)
    src.push(raw[:1000])
    assert res.update() == (0, n0)
    want = resampler_ref.direct(raw[:1000], fs_in, fs_out) if mode == "direct" else resampler_ref.polyphase(raw[:1000], bank, fs_in, fs_out)
    _check(out.read(0, n0), want, 0.0 if mode == "direct" else resampler_ref.error_bound(bank, raw), "%s: rebuilt resampler" % mode)
    for r in (res, out, src):
        r.close()


def test_chained_behind_a_conditioner(gctx):
    """cshort conditioner (D = 5) -> ring -> polyphase resampler 25 -> 10: the derived ring equals the restatement applied to the
    conditioner's OWN output, read back with gc_stream_read, within the bound for that input."""
    import gnsscorr
    fs_raw = 125e6
    fs_in, fs_out, bank = _poly_case("25-10")
    raw = _raw(30011, gnsscorr.GC_IQ_I16, seed=13, fs=fs_raw, tone_hz=-24e6)
    k = np.arange(64) - 31.5
    h1 = (np.sinc(k * 0.8 / 5) * np.hamming(64)).astype(np.float32)
    h1 /= h1.sum()
    mid = gnsscorr.IqStream(gctx, capacity_samples=1 << 13, max_window_samples=64)
    cond = gnsscorr.Conditioner(gctx, mid, fs_raw, -23.1e6, 5, h1, gnsscorr.GC_IQ_I16)
    out = gnsscorr.IqStream(gctx, capacity_samples=1 << 12, max_window_samples=64)
    res = gnsscorr.RingResampler(gctx, mid, fs_in, fs_out, out, "polyphase", bank)
    pos, i, sizes = 0, 0, [3001, 17, 5000, 1, 4999]
    while pos < len(raw):
        m = min(sizes[i % len(sizes)], len(raw) - pos)
        i += 1
        cond.push(raw[pos:pos + m])
        pos += m
        res.update()
    n_mid = -(-len(raw) // 5)
    assert mid.info()[:2] == (0, n_mid)
    x = mid.read(0, n_mid)
    ref = resampler_ref.polyphase(x, bank, fs_in, fs_out)
    assert res.info() == (n_mid, len(ref)) and out.info()[:2] == (0, len(ref))
    _check(out.read(0, len(ref)), ref, resampler_ref.error_bound(bank, x), "conditioner -> ring -> polyphase resampler")
    for h in (res, cond, out, mid):
        h.close()


def test_acquisition_on_the_resampled_ring(gctx, oracle):
    """One strong GPS L1 C/A satellite at 6.625 Msps, resampled polyphase to 4 Msps on the device, searched at N = 4000 on the derived
    ring, next to the same engine on a PUSHED ring that holds the float64 restatement's outputs cast to complex64: the same cell,
    the same Doppler, the statistic within the 1e-4 relative smoke() uses.  First the oracle's grid of the restatement: its peak
    must stand clear -- every cell outside the peak's own correlation lobe (the +-4 samples = one chip around it in its Doppler row,
    where a C/A code sampled 3.9 times per chip keeps (1 - 1/3.9)^2 = 0.55 of the peak by construction) below half the peak, and the
    lobe's own runner-up below 0.8 of it -- so that float32 against float64 cannot move the maximum."""
    import gnsscorr
    fs_in, fs_out, P, prn, doppler, step = 6.625e6, 4e6, 64, 9, 1500.0, 500
    _, _, bank = _poly_case("6.625-4")
    n_src = 16000
    code = np.asarray(gnsscorr.gps_l1_ca_code_gen_float(prn), np.float64)
    # the prototype delays by (L - 1) / (2 P) source samples: a code period is made to start on derived sample 600 exactly
    proto_len = len(gnsscorr.fir_low_pass(float(P), P * fs_in, fs_out / 2.1, fs_out / 10.0))
    start = 600.0 * fs_in / fs_out - (proto_len - 1) / (2.0 * P)
    t = np.arange(n_src, dtype=np.float64)
    chips = np.floor((t - start) * (1.023e6 / fs_in)).astype(np.int64) % 1023
    rng = np.random.Generator(np.random.PCG64(2025))
    x = (0.4 * code[chips] * np.exp(2j * np.pi * doppler * t / fs_in + 0.4j)
        + (rng.standard_normal(n_src) + 1j * rng.standard_normal(n_src)) * np.sqrt(0.5)).astype(np.complex64)
    y64 = resampler_ref.polyphase(x, bank, fs_in, fs_out)
    pushed = y64.astype(np.complex64)
    first = 1000
    assert len(pushed) >= first + 4000
    sampled = oracle.gps_l1_ca_code_sampled(prn, int(fs_out))
    p = oracle.pcps(fs_in=int(fs_out), sampled_ms=1, ms_per_code=1, samples_per_ms=np.float32(fs_out) * np.float32(0.001), samples_per_code=4000.0,
        samples_per_chip=4, doppler_max=5000, doppler_step=step)
    p.set_local_code(sampled)
    q = p.core(pushed[first:first + 4000])
    grid = np.asarray(p.grid(), np.float64)
    row, col = np.unravel_index(int(np.argmax(grid)), grid.shape)
    peak = grid[row, col]
    lobe = (col + np.arange(-4, 5)) % grid.shape[1]
    inside = grid[row, lobe].copy()
    inside[4] = 0.0
    outside = grid.copy()
    outside[row, lobe] = 0.0
    print("oracle: peak at bin %d, delay %d (Doppler %d Hz); runner-up of the grid %.3f of the peak, outside the peak's lobe %.3f" % (row, col, q.doppler,
        inside.max() / peak, outside.max() / peak))
    assert q.doppler == doppler and min((q.indext - (600 - first)) % 4000, (600 - first - q.indext) % 4000) <= 1
    assert outside.max() < 0.5 * peak and inside.max() < 0.8 * peak

    src = gnsscorr.IqStream(gctx, capacity_samples=1 << 15, max_window_samples=64)
    out = gnsscorr.IqStream(gctx, capacity_samples=1 << 14, max_window_samples=4000)
    res = gnsscorr.RingResampler(gctx, src, fs_in, fs_out, out, "polyphase", bank)
    src.push(x[:7001])
    res.update()
    src.push(x[7001:])
    res.update()
    assert out.info()[:2] == (0, len(y64))
    ring = gnsscorr.IqStream(gctx, capacity_samples=1 << 14, max_window_samples=4000)
    ring.push(pushed)
    acq = gnsscorr.PcpsAcquisition(gctx, 1, int(fs_out), 1, 1, np.float32(fs_out) * np.float32(0.001), 4000.0, 4, 5000, step)
    assert acq.fft_size == 4000
    acq.set_local_code(0, sampled)
    rd = acq.dwell_stream(out, first)[0]
    acq.reset()
    rp = acq.dwell_stream(ring, first)[0]
    print("derived ring: cell %d, Doppler %d Hz, statistic %.6f; pushed ring: cell %d, Doppler %d Hz, statistic %.6f; truth: delay %d, Doppler %.0f Hz"
        % (rd.indext, rd.doppler_hz, rd.test_statistics, rp.indext, rp.doppler_hz, rp.test_statistics, (600 - first) % 4000, doppler))
    assert (rd.indext, rd.doppler_hz) == (rp.indext, rp.doppler_hz) == (q.indext, q.doppler)
    assert abs(rd.test_statistics - rp.test_statistics) <= 1e-4 * rp.test_statistics
    for h in (acq, res, ring, out, src):
        h.close()
