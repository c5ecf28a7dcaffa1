"""GPU tests of the conditioner's real raw formats (gc_raw_real_format): one real channel at an intermediate frequency as float32,
int16, int8 or 2 bits packed four to a byte.  The main yardstick is the complex kernel itself: a real sample x is defined to give
what the matching complex format gives for (x, 0), equal under == (include/gnsscorr.h); tests/conditioner_ref.py's float64
restatement guards the pair against being wrong together."""
import functools
import os
import subprocess

import numpy as np
import pytest

import conditioner_ref
from helpers import synth_stream
from test_conditioner_gpu import _taps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_IN = 16e6
CASES = [(1, 1, 0.0), (1, 33, 0.0), (4, 63, FS_IN / 4), (5, 64, -3.1e6), (7, 129, 10.0)]
RAGGED = [1, 3, 70, 2, 5000, 6, 17, 64, 12345, 4, 1, 1, 128, 9973, 33, 5, 20000]  # tests/test_conditioner_gpu.py's


def _fmt(name):
    import gnsscorr
    return getattr(gnsscorr, "GC_RAW_REAL_" + name)


def as_complex_layout(x):
    """A real stream in the layout of the matching complex format with a zero imaginary part: complex64 [n] or int [n, 2]."""
    x = np.asarray(x)
    if x.dtype == np.float32:
        return x.astype(np.complex64)
    return np.stack([x, np.zeros_like(x)], axis=1)


@functools.lru_cache(maxsize=None)
def _real(n, name, seed):
    """Seeded noise plus a tone at 1.3 MHz, real, scaled to the format as tests/test_conditioner_gpu.py::_raw does."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal(n) + 2.0 * np.cos(2 * np.pi * 1.3e6 * np.arange(n) / FS_IN + 0.3)
    if name == "F32":
        out = x.astype(np.float32)
    else:
        scale, dt, lim = (1000.0, np.int16, 32767) if name == "I16" else (20.0, np.int8, 127)
        out = np.clip(np.round(x * scale), -lim, lim).astype(dt)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _two_bit(n, seed):
    v = np.random.Generator(np.random.PCG64(seed)).integers(-2, 2, n).astype(np.int8)
    assert np.bincount(v + 2, minlength=4).all()  # all four values present
    v.setflags(write=False)
    return v


def _run(gctx, raw, fmt, D, taps, f, sizes=None, capacity=1 << 17, per=1):
    """Pushes `raw` (in blocks of `sizes` SAMPLES, repeated; one block when None; `per` samples per array element) and reads every
    resident output back."""
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=capacity, max_window_samples=4096)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, f, D, taps, fmt)
    n = len(raw) * per
    pos, k, total = 0, 0, 0
    while pos < n:
        m = n - pos if sizes is None else min(sizes[k % len(sizes)], n - pos)
        k += 1
        first, n_out = cond.push(raw[pos // per:(pos + m) // per])
        assert first == total == (pos + D - 1) // D
        pos += m
        total += n_out
        assert cond.info() == (pos, (pos + D - 1) // D) and ring.info()[1] == total
    oldest, head, _ = ring.info()
    y = ring.read(oldest, head - oldest)
    cond.close()
    ring.close()
    return oldest, y


@functools.lru_cache(maxsize=None)
def _complex_run_cached(gctx, n, name, seed, D, T, f):
    """The reference of the equality tests, made by the complex kernel from (x, 0).  Computed once per case; nobody changes it."""
    import gnsscorr
    x = _two_bit(n, seed) if name == "2BIT" else _real(n, name, seed)
    cname = "I8" if name == "2BIT" else name
    first, y = _run(gctx, as_complex_layout(x), getattr(gnsscorr, "GC_IQ_" + cname), D, _taps(T, D), f)
    y.setflags(write=False)
    return first, y


@pytest.mark.parametrize("D, T, f", CASES)
@pytest.mark.parametrize("name", ["F32", "I16", "I8"])
def test_equal_to_the_complex_kernel(gctx, name, D, T, f):
    """The ring of a real-format conditioner equals (==, so up to the sign of a zero) the ring of a conditioner with the matching
    complex format fed (x, 0)."""
    n = 50021
    x = _real(n, name, 100 + D)
    first_c, want = _complex_run_cached(gctx, n, name, 100 + D, D, T, f)
    first, y = _run(gctx, x, _fmt(name), D, _taps(T, D), f)
    assert first == first_c == 0 and len(y) == (n + D - 1) // D and y.dtype == np.complex64
    bad = np.flatnonzero(y != want)
    print("real %s D=%d T=%d f=%g: %d of %d outputs differ from the complex kernel%s" % (name, D, T, f, bad.size, len(y),
        "" if bad.size == 0 else "; first at %d: %r vs %r" % (bad[0], y[bad[0]], want[bad[0]])))
    assert np.array_equal(y, want)
    assert np.abs(want).max() > 0
    if (D, T, f) == (1, 1, 0.0):
        assert np.array_equal(y, x.astype(np.float32).astype(np.complex64))


@pytest.mark.parametrize("D, T, f", CASES)
def test_two_bit_equals_eight_bit(gctx, D, T, f):
    """GC_RAW_REAL_2BIT fed pack_2bit(v) equals GC_RAW_REAL_I8 fed v; 50024 samples: a multiple of 4, not of 64."""
    import gnsscorr
    n = 50024
    v = _two_bit(n, 300 + D)
    taps = _taps(T, D)
    _, want = _run(gctx, v, gnsscorr.GC_RAW_REAL_I8, D, taps, f)
    _, y = _run(gctx, gnsscorr.pack_2bit(v), gnsscorr.GC_RAW_REAL_2BIT, D, taps, f, per=4)
    assert len(y) == len(want) == (n + D - 1) // D
    bad = np.flatnonzero(y != want)
    print("2-bit D=%d T=%d f=%g: %d of %d outputs differ from the 8-bit run" % (D, T, f, bad.size, len(y)))
    assert np.array_equal(y, want) and np.abs(want).max() > 0
    # and the 8-bit run is the complex kernel's, so the pair is not wrong together
    _, want_c = _complex_run_cached(gctx, n, "2BIT", 300 + D, D, T, f)
    assert np.array_equal(want, want_c)


def test_two_bit_layout_with_every_byte_value(gctx):
    """The 256 byte values in order, in the copy configuration: the ring is unpack_2bit's samples as complex64."""
    import gnsscorr
    packed = np.arange(256, dtype=np.uint8)
    want = gnsscorr.unpack_2bit(packed)
    assert want[:8].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and want[4 * 0x9C:4 * 0x9C + 4].tolist() == [0, -1, 1, -2]
    for block in (packed, packed.view(np.int8)):
        _, y = _run(gctx, block, gnsscorr.GC_RAW_REAL_2BIT, 1, np.ones(1, np.float32), 0.0, per=4)
        assert np.array_equal(y, want.astype(np.float32).astype(np.complex64))


@pytest.mark.parametrize("name, D, T, f", [("F32", 5, 64, -3.1e6), ("I16", 4, 63, FS_IN / 4), ("I8", 7, 129, 10.0), ("2BIT", 5, 64, -3.1e6)])
def test_parity_with_the_float64_restatement(gctx, name, D, T, f):
    """Each output component within conditioner_ref.error_bound of the float64 restatement fed (x, 0)."""
    import gnsscorr
    n = 50024
    x = _two_bit(n, 41) if name == "2BIT" else _real(n, name, 41)
    raw = gnsscorr.pack_2bit(x) if name == "2BIT" else x
    taps = _taps(T, D)
    _, y = _run(gctx, raw, _fmt(name), D, taps, f, per=4 if name == "2BIT" else 1)
    as_complex = as_complex_layout(x)
    ref = conditioner_ref.condition(as_complex, taps, D, f, FS_IN)
    bound = conditioner_ref.error_bound(taps, as_complex)
    err = max(np.abs(y.real - ref.real).max(), np.abs(y.imag - ref.imag).max())
    print("real parity %s D=%d T=%d f=%g: max component error %.3e, bound %.3e (%.4f of it)" % (name, D, T, f, err, bound, err / bound))
    assert len(y) == len(ref) and err <= bound


@pytest.mark.parametrize("name, D, T, f", [("I8", 7, 129, 10.0), ("2BIT", 5, 64, -3.1e6)])
def test_outputs_do_not_depend_on_the_push_sizes(gctx, name, D, T, f):
    import gnsscorr
    n = 120012
    packed = name == "2BIT"
    x = _two_bit(n, 7) if packed else _real(n, name, 7)
    raw = gnsscorr.pack_2bit(x) if packed else x
    per = 4 if packed else 1
    sizes = [(s + 3) // 4 * 4 for s in RAGGED] if packed else RAGGED  # whole bytes; some below D, some below T
    assert min(sizes) < D and sorted(sizes)[3] < T
    taps = _taps(T, D)
    _, whole = _run(gctx, raw, _fmt(name), D, taps, f, per=per)
    _, ragged = _run(gctx, raw, _fmt(name), D, taps, f, sizes=sizes, per=per)
    assert len(whole) == len(ragged) == (n + D - 1) // D
    assert whole.tobytes() == ragged.tobytes()


def test_two_bit_push_of_a_partial_byte_is_refused(gctx):
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, -3.1e6, 5, _taps(64, 5), gnsscorr.GC_RAW_REAL_2BIT)
    block = gnsscorr.pack_2bit(_two_bit(64, 1))
    assert cond.push(block[:2]) == (0, 2) and cond.info() == (8, 2)
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        cond.push(block[2:4], n_samples=6)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    assert cond.info() == (8, 2) and ring.info()[:2] == (0, 2)
    assert cond.push(block[2:4], n_samples=0) == (2, 0)  # n_in = 0 stays legal
    assert cond.push(block[2:4]) == (2, 2) and cond.info() == (16, 4)
    cond.close()
    ring.close()


def test_streams_and_engines_refuse_the_real_formats(gctx):
    import gnsscorr
    for fmt in (gnsscorr.GC_RAW_REAL_F32, gnsscorr.GC_RAW_REAL_2BIT, 7):
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024, iq_format=fmt)
        assert ei.value.status == gnsscorr.GC_ERR_INVALID and "unknown format %d" % fmt in str(ei.value)
    b = gnsscorr.TrackingBatch(gctx, 1, 3, 8)
    outcomes = []
    for fmt in (7, gnsscorr.GC_RAW_REAL_I8):  # an unknown value, then a real format: refused the same way
        with pytest.raises(gnsscorr.GnsscorrError) as ei:
            b.set_input_format(fmt)
        outcomes.append(ei.value.status)
    assert outcomes[0] == outcomes[1]
    b.close()


@pytest.mark.parametrize("name, D, T", [("F32", 8, 33), ("2BIT", 64, 16)])
def test_raw_ring_wrap(gctx, name, D, T):
    """6 MiB of raw bytes in blocks of about 1 MiB: the stream laps the raw ring (a 4 MiB chunk plus slack) whatever its slack.
    GC_RAW_REAL_F32 equals the complex run, GC_RAW_REAL_2BIT the GC_RAW_REAL_I8 run; the output ring holds every output."""
    import gnsscorr
    f = FS_IN / 4 if name == "F32" else -3.1e6
    taps = _taps(T, D)
    if name == "F32":
        n, block = (6 << 20) // 4, (1 << 20) // 4 + 12    # 1 572 864 samples, blocks of 262 156
        x = _real(n, "F32", 55)
        legs = [(x, gnsscorr.GC_RAW_REAL_F32, 1, block), (as_complex_layout(x), gnsscorr.GC_IQ_F32, 1, block)]
    else:
        n, block = (6 << 20) * 4, (1 << 20) * 4 + 40       # 25 165 824 samples, blocks of 4 194 344 (1 MiB + 10 bytes)
        x = _two_bit(n, 56)
        legs = [(gnsscorr.pack_2bit(x), gnsscorr.GC_RAW_REAL_2BIT, 4, block), (x, gnsscorr.GC_RAW_REAL_I8, 1, block)]
    n_out = (n + D - 1) // D
    got = []
    for raw, fmt, per, blk in legs:
        _, y = _run(gctx, raw, fmt, D, taps, f, sizes=[blk], capacity=max(8192, n_out), per=per)
        assert len(y) == n_out
        got.append(y)
    bad = np.flatnonzero(got[0] != got[1])
    print("raw ring wrap %s: %d samples, %d outputs, %d differ%s" % (name, n, n_out, bad.size, "" if bad.size == 0 else "; first at %d" % bad[0]))
    assert np.array_equal(got[0], got[1]) and np.abs(got[1]).max() > 0


def _blank_restatement(x, L, threshold, segments_est, segments_reset):
    """The header's state machine in float64 on real samples: E = sum x^2, floor from E / L."""
    x = np.asarray(x, np.float64)
    n_seg = len(x) // L
    E = (x[:n_seg * L] ** 2).reshape(n_seg, L).sum(axis=1)
    flags = np.zeros(n_seg, bool)
    ratio = np.full(n_seg, np.nan)
    n, last, noise = 0, False, 0.0
    for s, e in enumerate(E):
        if n < segments_est and not last:
            noise = (n * noise + e / float(L)) / (n + 1.0)
        else:
            r = e / noise
            ratio[s] = r / threshold
            if r > threshold:
                flags[s], last = True, True
            else:
                last = False
                if n > segments_reset:
                    n = 0
        n += 1
    return dict(flags=flags, ratio=ratio, n=n, noise=noise, decided=n_seg, blanked=int(flags.sum()))


def test_blanking_on_real_input(gctx):
    """GC_RAW_REAL_I16, L = 32: the blanked segments, blanking_info() and the ring equal the host restatement with dof = L.  As in
    tests/test_blanking_gpu.py the restatement first shows that no decided segment lies within 10 margins of the threshold, so
    that the float32 energy and running mean cannot legitimately decide differently; the pushes are ragged, so segments straddle
    push boundaries."""
    import blanking_ref
    import gnsscorr
    L, pfa, est, reset = 32, 0.04, 40, 300
    thr = float(np.float32(gnsscorr.chi2_upper_quantile(L, float(np.float32(pfa)))))
    band = 10.0 * blanking_ref.margin(L, est)
    n = 700 * L + L // 2
    for seed in range(8):
        rng = np.random.Generator(np.random.PCG64(900 + seed))
        x = rng.standard_normal(n)
        for start in np.sort(rng.integers((est + 2) * L, n - 2 * L, 25)):
            w = int(rng.integers(L // 4, 2 * L + 1))
            x[start:start + w] += 12.0 * np.cos(2 * np.pi * (0.11 * np.arange(w) + rng.uniform()))
        raw = np.clip(np.round(x * 1000.0), -32767, 32767).astype(np.int16)
        ref = _blank_restatement(raw, L, thr, est, reset)
        closest = float(np.nanmin(np.abs(ref["ratio"] - 1.0)))
        if closest >= band:
            break
    print("seed %d: closest |ratio - 1| = %.3e, band %.3e, %d of %d blanked, threshold %.4f" % (seed, closest, band, ref["blanked"], ref["decided"], thr))
    assert closest >= band and 0 < ref["blanked"] < ref["decided"]
    ring = gnsscorr.IqStream(gctx, capacity_samples=1 << 16, max_window_samples=4096)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, 1, np.ones(1, np.float32), gnsscorr.GC_RAW_REAL_I16)
    cond.set_pulse_blanking(pfa=pfa, length=L, segments_est=est, segments_reset=reset)
    pos, k = 0, 0
    while pos < n:
        m = min(RAGGED[k % len(RAGGED)], n - pos)
        k += 1
        first, n_out = cond.push(raw[pos:pos + m])
        assert (first, first + n_out) == (pos // L * L, (pos + m) // L * L)
        pos += m
    decided = n // L * L
    assert cond.info() == (n, decided)
    y = ring.read(0, decided).reshape(-1, L)
    want = raw[:decided].astype(np.float32).astype(np.complex64).reshape(-1, L)
    zero = ~y.any(axis=1)
    print("segments read back as zeros: %d, flagged by the restatement: %d" % (zero.sum(), ref["flags"].sum()))
    assert np.array_equal(y[ref["flags"]], np.zeros_like(y[ref["flags"]]))
    assert np.array_equal(y[~ref["flags"]], want[~ref["flags"]])
    binfo = cond.blanking_info()
    print("blanking_info", binfo, "restatement n %d noise %.9g" % (ref["n"], ref["noise"]))
    assert binfo["segments_decided"] == ref["decided"] and binfo["segments_blanked"] == ref["blanked"] and binfo["n_segments"] == ref["n"]
    assert abs(binfo["noise_power"] - ref["noise"]) <= blanking_ref.margin(L, est) * ref["noise"]
    assert binfo["threshold"] == thr
    cond.close()
    ring.close()


def test_blanking_is_refused_for_the_packed_format(gctx):
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, 1, np.ones(1, np.float32), gnsscorr.GC_RAW_REAL_2BIT)
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        cond.set_pulse_blanking(length=32, segments_est=4)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        cond.blanking_info()
    assert ei.value.status == gnsscorr.GC_ERR_STATE  # nothing was configured
    assert cond.push(np.arange(4, dtype=np.uint8)) == (0, 16)
    cond.close()
    ring.close()


def test_receiver_flow_from_real_samples_at_an_intermediate_frequency(gctx, oracle):
    """tests/test_conditioner_gpu.py::test_receiver_flow_at_an_intermediate_frequency's satellites (the same seed) from a front end
    that delivers REAL int8 samples at 16 Msps with the signals at a 4 MHz IF: conditioned with D = 4 and the same low-pass,
    acquired and tracked from the 4 Msps ring.  The search must find the PRNs, code-phase cells and Doppler bins that it finds
    for that test's complex cshort stream at 1.25 MHz.  A real signal has half its power at the image: detection and the cells
    are asserted, not the statistic's value."""
    import gnsscorr
    from test_closed_loop_gpu import GPS, _conf
    fs, n, D = 4_000_000, 4000, 4
    present, absent = [3, 8, 14, 22], [5, 11, 19, 30]
    codes = {p: oracle.gps_l1_ca_code(p).astype(np.float32) for p in present + absent}
    n_ms = 120
    x, truth = synth_stream([codes[p] for p in present], FS_IN, n_ms * n * D, seed=404, cn0_db_hz=(46.0, 50.0), doppler_max=4000.0)
    k = np.arange(x.size, dtype=np.float64)
    xc = x[:4 * n * D] * np.exp(2j * np.pi * (1.25e6 / FS_IN) * k[:4 * n * D])
    raw_c = np.clip(np.round(np.stack([xc.real, xc.imag], axis=1) * 64.0), -32767, 32767).astype(np.int16)
    # noise sigma of the real part is sqrt(1/2): 20 LSB of the int8 front end, clipping beyond 4.5 sigma
    raw_r = np.clip(np.round((x * np.exp(2j * np.pi * 0.25 * k)).real * 28.0), -127, 127).astype(np.int8)
    del x, k, xc
    taps = gnsscorr.fir_low_pass(1.0, FS_IN, 1.6e6, 612e3)
    prns = present + absent

    def search(ring):
        acq = gnsscorr.PcpsAcquisition(gctx, len(prns), fs, 4, 1, np.float32(fs) * np.float32(0.001), 4000.0, 4, 5000, 50)
        for s, p in enumerate(prns):
            acq.set_local_code(s, np.tile(oracle.gps_l1_ca_code_sampled(p, fs), 4))
        res = acq.dwell_stream(ring, 0)
        acq.close()
        stats = np.array([r.test_statistics for r in res])
        return res, stats, [s for s in range(len(prns)) if stats[s] > 2.0 * np.median(stats[len(present):])]

    ring_c = gnsscorr.IqStream(gctx, capacity_samples=40 * n, max_window_samples=4 * n)
    cond_c = gnsscorr.Conditioner(gctx, ring_c, FS_IN, 1.25e6, D, taps, gnsscorr.GC_IQ_I16)
    assert cond_c.push(raw_c) == (0, 4 * n)
    res_c, stats_c, det_c = search(ring_c)
    cond_c.close()
    ring_c.close()
    assert [prns[s] for s in det_c] == present, stats_c

    ring = gnsscorr.IqStream(gctx, capacity_samples=40 * n, max_window_samples=4 * n)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, FS_IN / 4, D, taps, gnsscorr.GC_RAW_REAL_I8)
    assert cond.push(raw_r[:4 * n * D]) == (0, 4 * n)
    res, stats, detected = search(ring)
    print("complex cshort statistics %s\nreal int8 statistics      %s" % (np.round(stats_c, 4), np.round(stats, 4)))
    assert [prns[s] for s in detected] == present, stats
    for s in detected:
        print("PRN %d: real (%d, %d Hz), complex (%d, %d Hz)" % (prns[s], res[s].indext, res[s].doppler_hz, res_c[s].indext, res_c[s].doppler_hz))
    for s in detected:
        assert (res[s].indext, res[s].doppler_hz) == (res_c[s].indext, res_c[s].doppler_hz)

    loop = gnsscorr.TrackingLoop(gctx, len(detected), 1023)
    for ch, s in enumerate(detected):
        r = res[s]
        conf = dict(GPS, acq_delay_samples=float(r.acq_delay_samples), acq_doppler_hz=float(r.acq_doppler_hz), acq_samplestamp_samples=0, sample_counter=0)
        loop.set_input_stream(ch, ring)
        loop.start(ch, _conf(gnsscorr, **conf), codes[prns[s]])
    recs = [[] for _ in detected]
    for ms in range(4, n_ms, 5):
        n_blk = min(5, n_ms - ms)
        first, n_out = cond.push(raw_r[ms * n * D:(ms + n_blk) * n * D])
        assert first == ms * n and n_out == n_blk * n
        out = loop.run(6)
        for ch in range(len(detected)):
            recs[ch].extend(r.copy() for r in out[ch] if r["valid"])
    loop.close()
    cond.close()
    ring.close()
    for ch in range(len(detected)):
        rr = np.array(recs[ch])
        t = truth[ch]
        print("PRN %d: %d periods, Doppler %.2f Hz (truth %.2f), lock test %.3f" % (present[ch], len(rr), rr["carrier_doppler_hz"][-50:].mean(), t["doppler"],
            rr["carrier_lock_test"][-1]))
        assert len(rr) >= n_ms - 3  # every complete code period was tracked
        stamps = rr["sample_counter"].astype(np.int64)
        assert np.all(np.diff(stamps) >= n - 1) and np.all(np.diff(stamps) <= n + 1) and stamps[-1] <= n_ms * n
        # the loop pulled in from the 50 Hz search bin and holds the carrier: a tenth of the bin, and a lock detector above one half
        assert abs(rr["carrier_doppler_hz"][-50:].mean() - t["doppler"]) < 5.0
        assert rr["carrier_lock_test"][-1] > 0.5


def test_cpp_real_if_selftest():
    """The C++ drop-in layer: hip_signal_conditioner with input_item_type "byte" and "2bit" (adapter/real_if_selftest.cpp)."""
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "real_if_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "real_if_selftest"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "real IF self-test passed" in p.stdout
