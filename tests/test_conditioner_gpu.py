"""GPU tests of the signal conditioner (gc_conditioner_*): the frequency-translating FIR decimator that writes an RF stream ring
from raw pushed samples.  Its definition is include/gnsscorr.h's; tests/conditioner_ref.py restates it in float64."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conditioner_ref
from helpers import synth_stream

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_IN = 16e6
CASES = [(1, 1, 0.0), (1, 33, 0.0), (4, 63, 1.25e6), (5, 64, -3.1e6), (7, 129, 10.0)]


def _taps(T, D, seed=5):
    """A low-pass for the decimated band with a little seeded asymmetry (a symmetric filter would hide a reversed tap order)."""
    if T == 1:
        return np.ones(1, np.float32)
    k = np.arange(T) - (T - 1) / 2.0
    h = np.sinc(k * 0.8 / D) * np.hamming(T)
    h = h / h.sum() + np.random.Generator(np.random.PCG64(seed)).standard_normal(T) * 1e-3
    return h.astype(np.float32)


def _raw(n, fmt, seed, tone_hz=1.3e6):
    """Seeded noise plus a tone, in the ring's input layout: complex64 [n] or int16 / int8 [n, 2]."""
    import gnsscorr
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5) + 2.0 * np.exp(2j * np.pi * tone_hz * np.arange(n) / FS_IN + 0.3j)
    if fmt == gnsscorr.GC_IQ_F32:
        return x.astype(np.complex64)
    scale, dt, lim = (1000.0, np.int16, 32767) if fmt == gnsscorr.GC_IQ_I16 else (20.0, np.int8, 127)
    return np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -lim, lim).astype(dt)


def _run(gctx, raw, fmt, D, taps, f, sizes=None, capacity=1 << 17, window=4096):
    """Pushes `raw` (in blocks of `sizes`, repeated; one block when None) and reads every resident output back."""
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=capacity, max_window_samples=window)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, f, D, taps, fmt)
    n = len(raw)
    pos, k, n_out_total = 0, 0, 0
    while pos < n:
        m = n - pos if sizes is None else min(sizes[k % len(sizes)], n - pos)
        k += 1
        first, n_out = cond.push(raw[pos:pos + m])
        assert first == n_out_total == (pos + D - 1) // D
        pos += m
        n_out_total += n_out
        assert cond.info() == (pos, (pos + D - 1) // D) and ring.info()[1] == n_out_total
    oldest, head, _ = ring.info()
    y = ring.read(oldest, head - oldest)
    cond.close()
    ring.close()
    return oldest, y


@pytest.mark.parametrize("D, T, f", CASES)
@pytest.mark.parametrize("fmt_name", ["F32", "I16", "I8"])
def test_parity_with_the_float64_restatement(gctx, fmt_name, D, T, f):
    """Each output component within (T + 16) 2^-23 sum|h| max|x| of the restatement: one rounding per product and per add, a few
    ulp for the mixer.  T = 1, h = {1}, D = 1, f = 0 is a bit-exact copy of the converted input."""
    import gnsscorr
    fmt = getattr(gnsscorr, "GC_IQ_" + fmt_name)
    raw = _raw(50021, fmt, seed=100 + D)
    taps = _taps(T, D)
    first, y = _run(gctx, raw, fmt, D, taps, f)
    assert first == 0 and len(y) == (len(raw) + D - 1) // D and y.dtype == np.complex64
    ref = conditioner_ref.condition(raw, taps, D, f, FS_IN)
    bound = conditioner_ref.error_bound(taps, raw)
    err = max(np.abs(y.real - ref.real).max(), np.abs(y.imag - ref.imag).max())
    print("conditioner parity %s D=%d T=%d f=%g: max component error %.3e, bound %.3e (%.4f of it)" % (fmt_name, D, T, f, err, bound, err / bound))
    assert err <= bound
    if (D, T, f) == (1, 1, 0.0):
        assert np.array_equal(y, conditioner_ref.to_complex(raw).astype(np.complex64))


@pytest.mark.parametrize("fmt_name, D, T, f", [("I16", 5, 64, -3.1e6), ("F32", 7, 129, 10.0), ("I8", 4, 63, 1.25e6)])
def test_outputs_do_not_depend_on_the_push_sizes(gctx, fmt_name, D, T, f):
    import gnsscorr
    fmt = getattr(gnsscorr, "GC_IQ_" + fmt_name)
    raw = _raw(120011, fmt, seed=7)
    taps = _taps(T, D)
    _, whole = _run(gctx, raw, fmt, D, taps, f)
    sizes = [1, 3, 70, 2, 5000, 6, 17, 64, 12345, 4, 1, 1, 128, 9973, 33, 5, 20000]  # some below D, some below T
    _, ragged = _run(gctx, raw, fmt, D, taps, f, sizes=sizes)
    assert len(whole) == len(ragged) == (len(raw) + D - 1) // D
    assert whole.tobytes() == ragged.tobytes()


def test_wrap_and_mirror(gctx):
    """More outputs than the ring holds: a window that straddles the wrap point and a window in the first max_window samples equal
    the restatement, read back (gc_stream_read splits at the wrap) and as a kernel sees them (a tracking window that crosses the
    wrap reads the mirror, which the conditioner's kernel writes itself)."""
    import gnsscorr
    D, T, f, fmt = 4, 63, 1.25e6, gnsscorr.GC_IQ_I16
    cap, win = 8192, 2048
    raw = _raw(4 * 20000 - 2, fmt, seed=21)
    taps = _taps(T, D)
    ring = gnsscorr.IqStream(gctx, capacity_samples=cap, max_window_samples=win)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, f, D, taps, fmt)
    for a, b in ((0, 30001), (30001, 52000), (52000, len(raw))):
        cond.push(raw[a:b])
    oldest, head, _ = ring.info()
    assert (oldest, head) == (20000 - cap, 20000)
    ref = conditioner_ref.condition(raw, taps, D, f, FS_IN)
    bound = conditioner_ref.error_bound(taps, raw)
    wrap = 2 * cap  # absolute sample 16384 sits at ring position 0
    for first, n in ((wrap - 700, 1500), (wrap + 100, 1200), (oldest, head - oldest)):
        y = ring.read(first, n)
        err = max(np.abs(y.real - ref[first:first + n].real).max(), np.abs(y.imag - ref[first:first + n].imag).max())
        print("window [%d, %d): max component error %.3e, bound %.3e" % (first, first + n, err, bound))
        assert err <= bound
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        ring.read(oldest - 1, 10)
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    with pytest.raises(gnsscorr.GnsscorrError):
        ring.read(head - 5, 10)
    # a correlator with an all-ones replica and no carrier sums its window: [wrap - 700, wrap + 800) is contiguous only through the
    # mirror; [wrap + 100, wrap + 1300) lies in the first max_window samples of the ring proper
    b = gnsscorr.TrackingBatch(gctx, 1, 3, 8)
    b.set_code(0, np.ones(8, np.float32), np.zeros(3, np.float32))
    b.set_input_stream(0, ring)
    for first, n in ((wrap - 700, 1500), (wrap + 100, 1200)):
        out = b.run(1, gnsscorr.epoch_params_array([gnsscorr.epoch_params(first, 0.0, 0.0, 0.0, 0.001, n)]))
        got = complex(out[0, 0, 1])
        want = ref[first:first + n].sum()
        # n samples each within `bound`, plus the correlator's own float32 sum: (n + 8) roundings of at most 2^-24 sum|y| each
        tol = n * bound + (n + 8) * 2.0 ** -24 * np.abs(ref[first:first + n]).sum() * np.sqrt(2.0)
        print("window sum at %d: |diff| %.3e, tolerance %.3e, |sum| %.3e" % (first, abs(got - want), tol, abs(want)))
        assert abs(got.real - want.real) <= tol and abs(got.imag - want.imag) <= tol
        assert np.abs(ref[first:first + n]).sum() > 100 * tol  # a stale or missing mirror would be far outside
    b.close()
    cond.close()
    ring.close()


def test_consumers_cannot_tell_a_conditioned_ring_from_a_pushed_one(gctx, oracle):
    """The same float32 samples in two rings -- written by the conditioner's kernel, and read back and pushed with gc_stream_push --
    give byte-identical tracking batch outputs and closed-loop records, block after block, across the wrap and the mirror."""
    import gnsscorr
    from test_closed_loop_gpu import GPS, _conf, _signal
    D, n_ep = 4, 40
    code, x = _signal(oracle, 9, FS_IN, 16000 * (n_ep + 3), 55, -2210.0, 4 * 777.0)
    k = np.arange(x.size)
    x = x * np.exp(2j * np.pi * 1.25e6 * k / FS_IN)
    raw = np.round(np.stack([x.real, x.imag], axis=1) * 64.0).astype(np.int16)
    taps = gnsscorr.fir_low_pass(1.0, FS_IN, 1.6e6, 612e3)
    assert len(taps) == 63
    rings = [gnsscorr.IqStream(gctx, capacity_samples=24000, max_window_samples=4000) for _ in range(2)]
    cond = gnsscorr.Conditioner(gctx, rings[0], FS_IN, 1.25e6, D, taps, gnsscorr.GC_IQ_I16)
    conf = dict(GPS, acq_delay_samples=777.0 + 8.0, acq_doppler_hz=-2200.0, acq_samplestamp_samples=0, sample_counter=0)
    shifts = np.array([-0.5, 0.0, 0.5], np.float32)
    loops, batches = [], []
    for r in rings:
        lp = gnsscorr.TrackingLoop(gctx, 1, 1023)
        lp.set_input_stream(0, r)
        lp.start(0, _conf(gnsscorr, **conf), code)
        loops.append(lp)
        b = gnsscorr.TrackingBatch(gctx, 1, 3, 1023)
        b.set_code(0, code, shifts)
        b.set_input_stream(0, r)
        batches.append(b)
    pushed, done, n_valid = 0, 0, 0
    while pushed < len(raw):
        m = min(26000, len(raw) - pushed)  # 6500 outputs per push: 1.6 code periods
        first, n_out = cond.push(raw[pushed:pushed + m])
        pushed += m
        y = rings[0].read(first, n_out)
        assert rings[1].push(y) == first
        assert rings[0].info() == rings[1].info()
        recs = [lp.run(3) for lp in loops]
        assert recs[0].tobytes() == recs[1].tobytes()
        n_valid += int(recs[0]["valid"].sum())
        head = rings[0].info()[1]
        while (done + 1) * 4000 + 1234 <= head:
            p = gnsscorr.epoch_params_array([gnsscorr.epoch_params(done * 4000 + 1234, 0.3, -0.0035, -100.25, 0.25575, 4000)])
            outs = [b.run(1, p) for b in batches]
            assert outs[0].tobytes() == outs[1].tobytes() and np.abs(outs[0]).max() > 0
            done += 1
    assert n_valid >= n_ep and done >= n_ep
    for h in loops + batches + [cond] + rings:
        h.close()


def test_receiver_flow_at_an_intermediate_frequency(gctx, oracle):
    """tests/test_receiver_flow_gpu.py's scenario with a front end that delivers cshort at 16 Msps and a 1.25 MHz IF: raw 5 ms blocks
    go through the conditioner (D = 4, 63-tap low-pass at 1.6 MHz); acquisition, hand-over and closed-loop tracking run on the 4 Msps
    conditioned ring, and every sample stamp is at that rate."""
    import gnsscorr
    from test_closed_loop_gpu import GPS, _conf
    fs, n, D = 4_000_000, 4000, 4
    present, absent = [3, 8, 14, 22], [5, 11, 19, 30]
    codes = {p: oracle.gps_l1_ca_code(p).astype(np.float32) for p in present + absent}
    n_ms = 260
    x, truth = synth_stream([codes[p] for p in present], FS_IN, n_ms * n * D, seed=404, cn0_db_hz=(46.0, 50.0), doppler_max=4000.0)
    k = np.arange(x.size, dtype=np.float64)
    x = x * np.exp(2j * np.pi * (1.25e6 / FS_IN) * k)  # the front end's IF
    raw = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * 64.0), -32767, 32767).astype(np.int16)  # cshort, noise sigma 45 LSB
    del x, k
    taps = gnsscorr.fir_low_pass(1.0, FS_IN, 1.6e6, 612e3)
    assert len(taps) == 63
    ring = gnsscorr.IqStream(gctx, capacity_samples=40 * n, max_window_samples=4 * n)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, 1.25e6, D, taps, gnsscorr.GC_IQ_I16)
    assert cond.push(raw[:4 * n * D]) == (0, 4 * n)

    prns = present + absent
    acq = gnsscorr.PcpsAcquisition(gctx, len(prns), fs, 4, 1, np.float32(fs) * np.float32(0.001), 4000.0, 4, 5000, 50)
    assert (acq.consumed_samples, acq.fft_size) == (4 * n, 8 * n)
    for s, p in enumerate(prns):
        acq.set_local_code(s, np.tile(oracle.gps_l1_ca_code_sampled(p, fs), 4))
    res = acq.dwell_stream(ring, 0)
    acq.close()
    stats = np.array([r.test_statistics for r in res])
    detected = [s for s in range(len(prns)) if stats[s] > 2.0 * np.median(stats[len(present):])]
    assert [prns[s] for s in detected] == present, stats

    loop = gnsscorr.TrackingLoop(gctx, len(detected), 1023)
    for ch, s in enumerate(detected):
        r = res[s]
        t = truth[ch]
        assert abs(r.acq_doppler_hz - t["doppler"]) <= 50.0
        conf = dict(GPS, acq_delay_samples=float(r.acq_delay_samples), acq_doppler_hz=float(r.acq_doppler_hz),
            acq_samplestamp_samples=0, sample_counter=0)
        loop.set_input_stream(ch, ring)
        loop.start(ch, _conf(gnsscorr, **conf), codes[prns[s]])
    recs = [[] for _ in detected]
    for ms in range(4, n_ms, 5):
        first, n_out = cond.push(raw[ms * n * D:(ms + 5) * n * D])  # 5 ms blocks of raw samples
        assert first == ms * n and n_out == min(5, n_ms - ms) * n
        out = loop.run(6)
        for ch in range(len(detected)):
            recs[ch].extend(r.copy() for r in out[ch] if r["valid"])
    loop.close()
    cond.close()
    ring.close()
    for ch in range(len(detected)):
        rr = np.array(recs[ch])
        t = truth[ch]
        assert len(rr) >= n_ms - 3                       # every complete code period was tracked
        stamps = rr["sample_counter"].astype(np.int64)
        assert np.all(np.diff(stamps) >= n - 1) and np.all(np.diff(stamps) <= n + 1)  # 4000 samples per period: the output rate
        assert stamps[-1] <= n_ms * n
        assert abs(rr["carrier_doppler_hz"][-50:].mean() - t["doppler"]) < 3.0   # PLL locked on the true Doppler
        assert rr["carrier_lock_test"][-1] > 0.8
        p = rr["corr"][-50:, 2] + 1j * rr["corr"][-50:, 3]
        e = rr["corr"][-50:, 0] + 1j * rr["corr"][-50:, 1]
        assert np.abs(p).mean() > 1.5 * np.abs(e).mean()  # prompt on the correlation peak, early half a chip off


def test_a_conditioned_ring_refuses_direct_pushes_and_outlives_its_handle(gctx):
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024)
    taps = _taps(33, 2)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, 2, taps, gnsscorr.GC_IQ_F32)
    block = _raw(1000, gnsscorr.GC_IQ_F32, seed=3)
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        ring.push(block)
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        ring.push_pinned(block.ctypes.data, block.size)  # refused before the pointer is used
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    assert ring.info()[:2] == (0, 0)
    # a second conditioner on the same ring, and one on a ring that already holds samples or has another format
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, 2, taps, gnsscorr.GC_IQ_F32)
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    used = gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024)
    used.push(block)
    with pytest.raises(gnsscorr.GnsscorrError):
        gnsscorr.Conditioner(gctx, used, FS_IN, 0.0, 2, taps, gnsscorr.GC_IQ_F32)
    used.close()
    i16 = gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024, iq_format=gnsscorr.GC_IQ_I16)
    with pytest.raises(gnsscorr.GnsscorrError):
        gnsscorr.Conditioner(gctx, i16, FS_IN, 0.0, 2, taps, gnsscorr.GC_IQ_F32)
    i16.close()
    # more outputs than the ring holds in one push
    with pytest.raises(gnsscorr.GnsscorrError):
        cond.push(np.zeros(2 * 8192 + 2, np.complex64))
    assert cond.push(block) == (0, 500)
    want = ring.read(0, 500)
    assert np.abs(want - conditioner_ref.condition(block, taps, 2, 0.0, FS_IN)).max() <= conditioner_ref.error_bound(taps, block)
    # the ring handle goes first: the conditioner keeps the ring alive and goes on writing it
    ring.close()
    assert cond.push(block) == (500, 500) and cond.info() == (2000, 1000)
    cond.close()


def test_cpp_signal_conditioner_selftest():
    """The C++ drop-in layer: hip_signal_conditioner (the reference adapter's configuration keys) owns ring + conditioner and hands
    the ring to hip_acquisition_bank and hip_tracking_group (adapter/conditioner_selftest.cpp)."""
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "conditioner_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "conditioner_selftest"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "signal conditioner self-test passed" in p.stdout
