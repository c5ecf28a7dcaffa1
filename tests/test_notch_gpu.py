"""GPU tests of the notch filter ring stage (gc_ring_notch_*): a GC_IQ_F32 ring derived on the device from another at the same rate,
with the segments that carry continuous-wave interference filtered (the reference's Notch_Filter / Notch_Filter_Lite).
tests/notch_ref.py restates it: decisions in float32, the filter in float64.  Every test first asserts, on the restatement, that its
input keeps a decision margin above 1e-4 and an exclusion margin above 1e-3 dB, so that a flipped flag is a defect and not a rounding
effect.  Flags, counters and n are exact, the noise floor is within 1e-5 relative, unflagged segments are the input's bits, filtered
samples are within 8 eps / (1 - p) max|x| of the float64 recursion, and the bits do not depend on pushes, updates or the wrap."""
import numpy as np
import pytest

import notch_ref

pytestmark = pytest.mark.gpu
P = 0.9
N = 16384
TONE = 0.0837
# name: (L, est, reset, mode, coeff, floor, threshold (None: from pfa = 1e-3))
CASES = {
    "full": (32, 10, 5000000, "full", 1, "linear", 1000.0),
    "lite3": (32, 10, 5000000, "lite", 3, "linear", 1000.0),
    "lite1-reset": (32, 10, 40, "lite", 1, "linear", 1000.0),
    "full-reference": (32, 10, 60, "full", 1, "reference", None),
    "full-33": (33, 3, 7, "full", 1, "linear", 1000.0),
    "lite-100": (100, 4, 5000000, "lite", 2, "linear", 1000.0),
}
_SCENES = {}


def _threshold(L, threshold):
    import gnsscorr
    return np.float32(gnsscorr.chi2_upper_quantile(2.0 * L, 1e-3) if threshold is None else threshold)


def _args(name):
    L, est, reset, mode, coeff, floor, thr = CASES[name]
    return dict(L=L, threshold=_threshold(L, thr), p_c_factor=P, segments_est=est, segments_reset=reset, mode=mode, segments_coeff=coeff, noise_floor=floor)


def _scene(name):
    """(x, restatement) of a case, made once: unit noise and a tone 30 dB above it in three bursts behind the first estimate; the
    first seed from the case's own on that keeps the margins."""
    if name not in _SCENES:
        args = _args(name)
        L, est = args["L"], args["segments_est"]
        spans = [((est + 6) * L, (est + 90) * L + 5), ((est + 140) * L + L // 2, (est + 141) * L + 3), ((est + 200) * L, (est + 330) * L)]
        first = 100 + 50 * sorted(CASES).index(name)
        for seed in range(first, first + 50):
            x = (notch_ref.noise(N, seed) + notch_ref.tone(N, TONE, np.sqrt(1000.0), spans)).astype(np.complex64)
            ref = notch_ref.notch(x, **args)
            if ref["decision_margin"] > 1e-4 and ref["exclusion_margin_db"] > 1e-3:
                break
        _SCENES[name] = (x, ref)
    x, ref = _SCENES[name]
    assert ref["decision_margin"] > 1e-4 and ref["exclusion_margin_db"] > 1e-3, (ref["decision_margin"], ref["exclusion_margin_db"])
    return x, ref


def _make(gctx, src, out, args):
    import gnsscorr
    return gnsscorr.RingNotch(gctx, src, out, pfa=1e-3, p_c_factor=P, length=args["L"], segments_est=args["segments_est"],
        segments_reset=args["segments_reset"], mode=args["mode"], segments_coeff=args["segments_coeff"], noise_floor=args["noise_floor"],
        threshold=float(args["threshold"]))


def _run(gctx, x, args, pushes, update_every=1, src_cap=1 << 15, out_cap=1 << 15, out_win=64):
    """Pushes x in pieces of `pushes` (cycled) with an update after every update_every-th push and one at the end; checks first /
    n_out / info() against floor(head / L) * L; returns (oldest, the resident outputs, state)."""
    import gnsscorr
    L = args["L"]
    src = gnsscorr.IqStream(gctx, capacity_samples=src_cap, max_window_samples=64)
    out = gnsscorr.IqStream(gctx, capacity_samples=out_cap, max_window_samples=out_win)
    f = _make(gctx, src, out, args)
    assert f.update() == (0, 0) and f.info() == (0, 0)
    pos, k, made = 0, 0, 0
    while pos < len(x):
        m = min(pushes[k % len(pushes)], len(x) - pos)
        k += 1
        src.push(x[pos:pos + m])
        pos += m
        if k % update_every == 0 or pos == len(x):
            first, n_out = f.update()
            want = pos // L * L
            assert (first, first + n_out) == (made, want), (pos, first, n_out, want)
            made = want
            assert f.info() == (pos, made) and out.info()[1] == made
    oldest, head, _ = out.info()
    y = out.read(oldest, head - oldest)
    st = f.state()
    for h in (f, out, src):
        h.close()
    return oldest, y, st


def _compare(x, ref, y, st, L, what):
    flags = ref["flags"]
    assert (st["segments_decided"], st["segments_filtered"], st["n_segments"], st["active"]) == (ref["decided"], ref["filtered"], ref["n"], ref["active"]), st
    assert abs(st["noise_power"] - float(ref["noise"])) <= 1e-5 * float(ref["noise"]), (st["noise_power"], ref["noise"])
    keep = np.repeat(~flags, L)
    assert len(y) == len(keep)
    # a flag that differs shows here: a filtered segment is not the input's bits, and an unfiltered one is far from the recursion
    assert y[keep].tobytes() == x[:len(y)][keep].tobytes()
    bound = notch_ref.error_bound(P, x)
    err = y[~keep].astype(np.complex128) - ref["out"][~keep]
    worst = float(max(np.abs(err.real).max(), np.abs(err.imag).max()))
    print("%s: %d of %d segments filtered, noise %.6g; filtered samples deviate by %.3e, bound %.3e (%.3f of it)" % (what, flags.sum(), len(flags),
        st["noise_power"], worst, bound, worst / bound))
    assert flags.any() and worst <= bound
    assert abs(st["last"] - ref["last"]) <= 2.0 * bound


@pytest.mark.parametrize("name", sorted(CASES))
def test_outputs_flags_and_state_against_the_restatement(gctx, name):
    x, ref = _scene(name)
    args = _args(name)
    # the 33-sample case reads a source ring of 4099 samples that wraps three times
    src_cap, pushes = (4099, [1000, 37, 2500, 1, 811, 1999]) if name == "full-33" else (1 << 15, [len(x)])
    oldest, y, st = _run(gctx, x, args, pushes, src_cap=src_cap)
    assert oldest == 0 and st["threshold"] == float(args["threshold"])
    if args["segments_reset"] < 1000:
        assert ref["estimated"].sum() > args["segments_est"]  # a second estimate ran
    assert ref["starts"].sum() >= 2
    _compare(x, ref, y, st, args["L"], name)


@pytest.mark.parametrize("name", ["full", "lite3", "full-33", "full-reference"])
def test_bits_do_not_depend_on_pushes_and_updates(gctx, name):
    x, _ = _scene(name)
    args = _args(name)
    L = args["L"]
    _, y0, st0 = _run(gctx, x, args, [len(x)])
    ragged = [1, 7, L - 1, L + 1, 1000]
    for what, pushes, every in (("an update after every push", ragged, 1), ("an update after every third push", ragged, 3)):
        _, y, st = _run(gctx, x, args, pushes, update_every=every)
        assert y.tobytes() == y0.tobytes(), what
        assert st == st0, (what, st, st0)


@pytest.mark.parametrize("name", ["full", "lite3"])
def test_output_ring_wrap_and_mirror(gctx, name):
    """An output ring of 1000 samples -- no multiple of L = 32 -- so that the wrap cuts segments in two: the resident outputs are
    bit-equal to those of a ring that never wraps, and a correlator with an all-ones replica whose window is contiguous only
    through the mirror sums what the ring holds."""
    import gnsscorr
    x, ref = _scene(name)
    args = _args(name)
    L, cap = args["L"], 1000
    _, y0, st0 = _run(gctx, x, args, [len(x)])
    for pushes in ([len(x)], [1500, 333]):
        oldest, y, st = _run(gctx, x, args, pushes, out_cap=cap)
        assert oldest == len(y0) - cap and y.tobytes() == y0[oldest:].tobytes() and st == st0, pushes
    # the mirror: a window across the ring's end, inside a filtered run
    src = gnsscorr.IqStream(gctx, capacity_samples=1 << 15, max_window_samples=64)
    out = gnsscorr.IqStream(gctx, capacity_samples=cap, max_window_samples=64)
    f = _make(gctx, src, out, args)
    src.push(x[:9 * cap + 17 * L])
    f.update()
    wrap = 9 * cap
    assert ref["flags"][wrap // L - 1] and ref["flags"][wrap // L + 1] and out.info()[1] > wrap + 60
    across = out.read(wrap - 30, 60)
    assert across.tobytes() == y0[wrap - 30:wrap + 30].tobytes()
    b = gnsscorr.TrackingBatch(gctx, 1, 3, 8)
    b.set_code(0, np.ones(8, np.float32), np.zeros(3, np.float32))
    b.set_input_stream(0, out)
    got = complex(b.run(1, gnsscorr.epoch_params_array([gnsscorr.epoch_params(wrap - 30, 0.0, 0.0, 0.0, 0.001, 60)]))[0, 0, 1])
    want = across.astype(np.complex128).sum()
    tol = (60 + 8) * 2.0 ** -24 * np.abs(across).sum() * np.sqrt(2.0)  # the correlator's own float32 sum of 60 stored values
    print("%s: window sum through the mirror: |diff| %.3e, tolerance %.3e, |sum| %.3e" % (name, abs(got - want), tol, abs(want)))
    assert abs(got.real - want.real) <= tol and abs(got.imag - want.imag) <= tol
    assert np.abs(across[30:]).sum() > 100 * tol  # a stale or missing mirror (zeros) would be far outside
    for h in (b, f, out, src):
        h.close()


def test_eviction_leaves_the_state_untouched(gctx):
    import gnsscorr
    x, ref = _scene("full")
    args = _args("full")
    src = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    out = gnsscorr.IqStream(gctx, capacity_samples=4096, max_window_samples=64)
    f = _make(gctx, src, out, args)
    src.push(x[:1000])
    assert f.update() == (0, 992) and f.info() == (1000, 992)
    st = f.state()
    assert st["segments_decided"] == 31 and st["segments_filtered"] == int(ref["flags"][:31].sum()) > 0
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        out.push(np.zeros(8, np.complex64))
    assert e.value.status == gnsscorr.GC_ERR_STATE
    src.push(x[1000:2000])
    src.push(x[2000:3000])  # sample 991 is gone
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        f.update()
    assert e.value.status == gnsscorr.GC_ERR_STATE
    assert f.info() == (1000, 992) and out.info()[:2] == (0, 992) and f.state() == st
    f.close()
    out.push(np.zeros(8, np.complex64))  # released for pushes again
    for h in (out, src):
        h.close()


def test_create_refusals(gctx):
    import gnsscorr
    args = _args("full")
    src = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    out = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    f = _make(gctx, src, out, args)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        _make(gctx, src, out, args)  # a second producer on the output ring
    assert e.value.status == gnsscorr.GC_ERR_STATE and "already has a producer" in str(e.value)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        _make(gctx, src, src, args)
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "the same ring" in str(e.value)
    for fmt in (gnsscorr.GC_IQ_I16, gnsscorr.GC_IQ_I8):
        ring = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=fmt)
        free = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
        for a, b in ((ring, free), (src, ring.accept_quantised_output())):
            with pytest.raises(gnsscorr.GnsscorrError) as e:
                _make(gctx, a, b, args)
            assert e.value.status == gnsscorr.GC_ERR_INVALID and "must be GC_IQ_F32" in str(e.value)
        free.push(np.zeros(8, np.complex64))  # still a plain ring
        for h in (free, ring):
            h.close()
    for h in (f, out, src):
        h.close()


def test_chained_behind_a_conditioner_and_in_front_of_a_ring_decimator(gctx):
    """conditioner (D = 2) -> ring -> notch -> ring -> ring decimator (one tap, D = 2): the notched ring equals the restatement
    applied to the conditioner's OWN output, and the decimator's outputs are every second notched sample, bit for bit."""
    import gnsscorr
    n = 2 * 8192
    raw = (notch_ref.noise(n, 31) + notch_ref.tone(n, TONE / 2.0, np.sqrt(1000.0), [(2 * 40 * 32, 2 * 150 * 32 + 9)])).astype(np.complex64)
    k = np.arange(16) - 7.5
    h = (np.sinc(k * 0.45) * np.hamming(16)).astype(np.float32)
    h /= h.sum()
    args = _args("full")
    mid = gnsscorr.IqStream(gctx, capacity_samples=1 << 14, max_window_samples=64)
    cond = gnsscorr.Conditioner(gctx, mid, 8e6, 0.0, 2, h)
    out = gnsscorr.IqStream(gctx, capacity_samples=1 << 14, max_window_samples=64)
    f = _make(gctx, mid, out, args)
    half = gnsscorr.IqStream(gctx, capacity_samples=1 << 13, max_window_samples=64)
    dec = gnsscorr.RingDecimator(gctx, out, 2, np.ones(1, np.float32), half)
    pos, i, sizes = 0, 0, [3001, 17, 5000, 1, 4999]
    while pos < n:
        m = min(sizes[i % len(sizes)], n - pos)
        i += 1
        cond.push(raw[pos:pos + m])
        pos += m
        f.update()
        dec.update()
    x = mid.read(0, n // 2)
    ref = notch_ref.notch(x, **args)
    assert ref["decision_margin"] > 1e-4 and ref["exclusion_margin_db"] > 1e-3
    assert f.info() == (n // 2, n // 2) and out.info()[:2] == (0, n // 2)
    y = out.read(0, n // 2)
    _compare(x, ref, y, f.state(), args["L"], "conditioner -> notch")
    assert dec.info() == (n // 2, n // 4)
    assert half.read(0, n // 4).tobytes() == y[::2].tobytes()
    for hd in (dec, f, cond, half, out, mid):
        hd.close()


def _search(x, code, fs, blocks=4, n=4000, doppler_max=5000, doppler_step=250):
    """4 x 1 ms non-coherent PCPS search in numpy: (Doppler, delay, peak / median) of the accumulated grid."""
    fc = np.conj(np.fft.fft(code[:n].astype(np.complex128)))
    dopplers = np.arange(-doppler_max, doppler_max + 1, doppler_step)
    grid = np.zeros((len(dopplers), n))
    t = np.arange(n)
    for b in range(blocks):
        blk = x[b * n:(b + 1) * n].astype(np.complex128)
        for i, d in enumerate(dopplers):
            grid[i] += np.abs(np.fft.ifft(np.fft.fft(blk * np.exp(-2j * np.pi * d * t / fs)) * fc)) ** 2
    i, k = np.unravel_index(np.argmax(grid), grid.shape)
    return int(dopplers[i]), int(k), float(grid[i, k] / np.median(grid))


def test_acquisition_finds_the_satellite_behind_the_notch_and_not_in_front_of_it(gctx, oracle):
    """GPS L1 C/A PRN 1 at 4 Msps, C/N0 50 dB-Hz, code delay 1234 samples, Doppler 1500 Hz, unit noise, and a tone 30 dB above the
    noise from sample 16 L on.  On the raw stream a 4 x 1 ms non-coherent search picks a wrong cell; on the notched ring
    PcpsAcquisition.dwell_stream returns (1500 Hz, 1234)."""
    import gnsscorr
    fs, n, L = 4_000_000, 16000, 32
    code = oracle.gps_l1_ca_code_sampled(1, fs)
    t = np.arange(n)
    sat = np.sqrt(10.0 ** 5.0 / fs) * code[(t - 1234) % 4000] * np.exp(2j * np.pi * 1500.0 * t / fs + 0.4j)
    args = dict(L=L, threshold=np.float32(1000.0), p_c_factor=P, segments_est=10, segments_reset=5000000, mode="full", segments_coeff=1, noise_floor="linear")
    for seed in range(2024, 2034):
        x = (notch_ref.noise(n, seed) + sat + notch_ref.tone(n, TONE, np.sqrt(1000.0), [(16 * L, n)])).astype(np.complex64)
        ref = notch_ref.notch(x, **args)
        raw_cell, ref_cell = _search(x, code, fs), _search(ref["out"], code, fs)
        if ref["decision_margin"] > 1e-4 and ref["exclusion_margin_db"] > 1e-3 and raw_cell[:2] != (1500, 1234) and ref_cell[:2] == (1500, 1234):
            break
    print("raw stream: %s; restated notch: %s" % (raw_cell, ref_cell))
    assert ref["decision_margin"] > 1e-4 and ref["exclusion_margin_db"] > 1e-3
    assert raw_cell[:2] != (1500, 1234) and ref_cell[:2] == (1500, 1234)
    assert ref["flags"][16:].all() and not ref["flags"][:16].any()

    src = gnsscorr.IqStream(gctx, capacity_samples=1 << 15, max_window_samples=4000)
    out = gnsscorr.IqStream(gctx, capacity_samples=1 << 15, max_window_samples=4000)
    f = _make(gctx, src, out, args)
    src.push(x)
    assert f.update() == (0, n)
    y = out.read(0, n)
    _compare(x, ref, y, f.state(), L, "tone behind the estimate")
    # the tone, 30 dB above the noise, is attenuated by more than 100 dB: what is left of it is far below the noise
    k = np.arange(8000, 16000)
    left = abs(np.vdot(np.exp(2j * np.pi * TONE * k), y[k].astype(np.complex128))) / len(k)
    print("tone amplitude %.1f in, %.3e left of it after the notch" % (np.sqrt(1000.0), left))
    for ring, want in ((src, None), (out, (1234, 1500))):
        acq = gnsscorr.PcpsAcquisition(gctx, 1, fs, 1, 1, np.float32(fs) * np.float32(0.001), 4000.0, 4, 5000, 250, max_dwells=4)
        acq.set_local_code(0, code)
        for b in range(4):
            r = acq.dwell_stream(ring, 4000 * b)[0]
        got = (int(r.indext), int(r.doppler_hz))
        print("%s ring: peak at delay %d, %d Hz, statistic %.4f" % ("notched" if want else "raw", got[0], got[1], r.test_statistics))
        if want:
            assert got == want
        else:
            assert got != (1234, 1500)
        acq.close()
    for h in (f, out, src):
        h.close()
