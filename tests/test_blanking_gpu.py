"""GPU tests of the conditioner's pulse blanking (gc_conditioner_set_pulse_blanking): segment energies, the decision state machine
and the in-place zeroing of the raw ring, in front of the frequency-translating FIR decimator.  The definition is
include/gnsscorr.h's; tests/blanking_ref.py restates it in float64 (a restatement, not a pin of the reference block).

Every parity test first asserts ON THE RESTATEMENT that no decided segment lies within 10 * margin of the threshold, so that a
float32 energy and a float32 running mean cannot legitimately decide differently: no segment is excluded from any comparison."""
import functools
import os
import subprocess

import numpy as np
import pytest

import blanking_ref
import conditioner_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS_IN = 16e6
#        L    pfa    segments_est segments_reset
SHAPES = [(32, 0.04, 40, 300), (8, 0.01, 16, 100), (250, 0.04, 12, 60), (1024, 0.001, 4, 20)]
RAGGED = [1, 3, 70, 2, 5000, 6, 17, 64, 12345, 4, 1, 1, 128, 9973, 33, 5, 20000]  # tests/test_conditioner_gpu.py's


def _threshold(L, pfa):
    import gnsscorr
    return float(np.float32(gnsscorr.chi2_upper_quantile(2 * L, float(np.float32(pfa)))))


def _pulsed(n, L, first_pulse, n_bursts, fmt_name, seed):
    """Unit-variance complex noise plus bursts of amplitude 12 and width L/4 .. 2L from sample `first_pulse` on, scaled to the
    format as tests/test_conditioner_gpu.py::_raw does."""
    rng = np.random.Generator(np.random.PCG64(seed + 10 * L))
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    for start in np.sort(rng.integers(first_pulse, n - 2 * L, n_bursts)):
        w = int(rng.integers(max(1, L // 4), 2 * L + 1))
        x[start:start + w] += 12.0 * np.exp(2j * np.pi * (0.11 * np.arange(w) + rng.uniform()))
    if fmt_name == "F32":
        return x.astype(np.complex64)
    scale, dt, lim = (1000.0, np.int16, 32767) if fmt_name == "I16" else (20.0, np.int8, 127)
    return np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -lim, lim).astype(dt)


@functools.lru_cache(maxsize=None)
def _case(L, pfa, est, reset, fmt_name, n_seg=700, n_bursts=25):
    """(raw, restatement) for a shape and format: the first seed whose restatement keeps every decided segment at least 10 margins
    away from the threshold.  Computed once and shared; nobody changes it."""
    thr = _threshold(L, pfa)
    band = 10.0 * blanking_ref.margin(L, est)
    for seed in range(8):
        raw = _pulsed(n_seg * L + L // 2, L, (est + 2) * L, n_bursts, fmt_name, seed)
        ref = blanking_ref.blank(raw, L, thr, est, reset)
        closest = float(np.nanmin(np.abs(ref["ratio"] - 1.0)))
        if closest >= band:
            break
    print("L=%d %s: seed %d, closest |ratio - 1| = %.3e, band %.3e, %d of %d blanked, %d resets" % (L, fmt_name, seed, closest, band,
        ref["blanked"], ref["decided"], ref["resets"]))
    assert closest >= band, "no seed keeps every segment outside the band"
    raw.setflags(write=False)
    return raw, ref, thr


def _run(gctx, raw, fmt_name, D, taps, f, blanking, sizes=None, capacity=1 << 20):
    """Pushes `raw` through a conditioner (blanking: None or (L, pfa, est, reset)); returns (outputs, info, blanking_info)."""
    import gnsscorr
    fmt = getattr(gnsscorr, "GC_IQ_" + fmt_name)
    ring = gnsscorr.IqStream(gctx, capacity_samples=capacity, max_window_samples=4096)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, f, D, taps, fmt)
    L = 1
    if blanking is not None:
        L = blanking[0]
        cond.set_pulse_blanking(pfa=blanking[1], length=L, segments_est=blanking[2], segments_reset=blanking[3])
    pos, k, total = 0, 0, 0
    while pos < len(raw):
        m = len(raw) - pos if sizes is None else min(sizes[k % len(sizes)], len(raw) - pos)
        k += 1
        first, n_out = cond.push(raw[pos:pos + m])
        pos += m
        head = (pos // L * L + D - 1) // D
        assert first == total and first + n_out == head, (pos, first, n_out, head)
        total += n_out
        assert cond.info() == (pos, head) and ring.info()[1] == head
    oldest, head, _ = ring.info()
    y = ring.read(oldest, head - oldest)
    binfo = cond.blanking_info() if blanking is not None else None
    info = cond.info()
    cond.close()
    ring.close()
    return oldest, y, info, binfo


def _check_info(binfo, ref, thr, L, est):
    print("blanking_info", binfo, "restatement n %d noise %.9g" % (ref["n"], ref["noise"]))
    assert binfo["segments_decided"] == ref["decided"] and binfo["segments_blanked"] == ref["blanked"]
    assert binfo["n_segments"] == ref["n"]
    assert abs(binfo["noise_power"] - ref["noise"]) <= blanking_ref.margin(L, est) * ref["noise"]
    assert binfo["threshold"] == thr


@pytest.mark.parametrize("L, pfa, est, reset", SHAPES)
@pytest.mark.parametrize("fmt_name", ["F32", "I16", "I8"])
def test_flags_and_state_in_the_copy_configuration(gctx, fmt_name, L, pfa, est, reset):
    """T = 1, h = {1}, D = 1, f = 0: flagged segments read back as zeros, every other segment is the converted input bit for bit,
    the head is floor(N / L) L, and the state block equals the restatement's."""
    raw, ref, thr = _case(L, pfa, est, reset, fmt_name)
    assert ref["resets"] >= 2 and 0 < ref["blanked"] < ref["decided"]
    first, y, info, binfo = _run(gctx, raw, fmt_name, 1, np.ones(1, np.float32), 0.0, (L, pfa, est, reset))
    decided = len(raw) // L * L
    assert first == 0 and info == (len(raw), decided) and len(y) == decided
    x = conditioner_ref.to_complex(raw).astype(np.complex64)[:decided].reshape(-1, L)
    got = y.reshape(-1, L)
    zero = ~got.any(axis=1)
    print("segments read back as zeros: %d, flagged by the restatement: %d" % (zero.sum(), ref["flags"].sum()))
    assert np.array_equal(got[ref["flags"]], np.zeros_like(got[ref["flags"]]))
    assert np.array_equal(got[~ref["flags"]], x[~ref["flags"]])
    _check_info(binfo, ref, thr, L, est)


@pytest.mark.parametrize("fmt_name, D, T, f", [("I16", 5, 64, -3.1e6), ("I8", 4, 63, 1.25e6)])
def test_blanking_in_front_of_the_filter(gctx, fmt_name, D, T, f):
    """The outputs are the translating filter's outputs for the blanked raw stream, within the filter's own bound."""
    from test_conditioner_gpu import _taps
    L, pfa, est, reset = SHAPES[0]
    raw, ref, thr = _case(L, pfa, est, reset, fmt_name)
    taps = _taps(T, D)
    first, y, info, binfo = _run(gctx, raw, fmt_name, D, taps, f, (L, pfa, est, reset))
    decided = len(raw) // L * L
    n_out = (decided + D - 1) // D
    assert first == 0 and info == (len(raw), n_out) and len(y) == n_out
    blanked = blanking_ref.apply(raw, L, ref["flags"])
    want = conditioner_ref.condition(blanked, taps, D, f, FS_IN, 0, n_out)
    bound = conditioner_ref.error_bound(taps, raw)
    err = max(np.abs(y.real - want.real).max(), np.abs(y.imag - want.imag).max())
    unblanked = conditioner_ref.condition(raw, taps, D, f, FS_IN, 0, n_out)
    print("blanking + filter %s D=%d T=%d: max component error %.3e, bound %.3e; distance to the unblanked outputs %.3e" % (fmt_name, D, T, err, bound,
        np.abs(unblanked - want).max()))
    assert err <= bound
    assert np.abs(unblanked - want).max() > 100 * bound  # the comparison can tell blanked from unblanked
    _check_info(binfo, ref, thr, L, est)


@pytest.mark.parametrize("fmt_name, D, T, f, shape", [("I16", 5, 64, -3.1e6, 0), ("F32", 1, 1, 0.0, 2), ("I8", 4, 63, 1.25e6, 1)])
def test_results_do_not_depend_on_the_push_sizes(gctx, fmt_name, D, T, f, shape):
    from test_conditioner_gpu import _taps
    L, pfa, est, reset = SHAPES[shape]
    raw, ref, thr = _case(L, pfa, est, reset, fmt_name)
    taps = _taps(T, D)
    _, whole, info_w, b_w = _run(gctx, raw, fmt_name, D, taps, f, (L, pfa, est, reset))
    _, ragged, info_r, b_r = _run(gctx, raw, fmt_name, D, taps, f, (L, pfa, est, reset), sizes=RAGGED)
    assert min(RAGGED) < L and len(whole) == len(ragged) == (len(raw) // L * L + D - 1) // D
    assert whole.tobytes() == ragged.tobytes()
    assert info_w == info_r and b_w == b_r
    _check_info(b_r, ref, thr, L, est)


def test_raw_ring_wrap_and_chunk_boundary(gctx):
    """One cbyte stream longer than the raw ring (2 167 872 samples for cbyte) and pushed in blocks of which one is longer than a
    4 MiB chunk (2 097 152 samples): with L = 250 a segment straddles the ring's wrap and another the chunk boundary inside the
    second push (sample 2 197 155), its first part having arrived with the earlier copy."""
    L, pfa, est, reset = 250, 1e-4, 12, 60
    n_seg = 9200
    raw, ref, thr = _case(L, pfa, est, reset, "I8", n_seg=n_seg, n_bursts=80)
    assert len(raw) > 2167872 + L and (100003 + 2097152) % L != 0 and 2167872 % L != 0
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=1 << 22, max_window_samples=4096)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, 1, np.ones(1, np.float32), gnsscorr.GC_IQ_I8)
    cond.set_pulse_blanking(pfa=pfa, length=L, segments_est=est, segments_reset=reset)
    for a, b in ((0, 100003), (100003, 2250000), (2250000, len(raw))):
        first, n_out = cond.push(raw[a:b])
        assert (first, first + n_out) == (a // L * L, b // L * L)
    oldest, head, _ = ring.info()
    assert (oldest, head) == (0, n_seg * L)
    y = ring.read(0, head).reshape(-1, L)
    x = conditioner_ref.to_complex(raw).astype(np.complex64)[:head].reshape(-1, L)
    x[ref["flags"]] = 0
    bad = np.flatnonzero((y != x).any(axis=1))
    print("segments that differ from the restatement: %s" % bad[:20])
    assert bad.size == 0
    _check_info(cond.blanking_info(), ref, thr, L, est)
    cond.close()
    ring.close()


@pytest.mark.parametrize("fmt_name", ["F32", "I16", "I8"])
def test_blanking_off_is_untouched(gctx, fmt_name):
    """Without set_pulse_blanking the pulses stay: the copy configuration is a bit-exact copy of the converted input (the
    restatement without blanking) and the heads are (N, ceil(N / D))."""
    from test_conditioner_gpu import _taps
    import gnsscorr
    L, pfa, est, reset = SHAPES[0]
    raw, ref, thr = _case(L, pfa, est, reset, fmt_name)
    first, y, info, _ = _run(gctx, raw, fmt_name, 1, np.ones(1, np.float32), 0.0, None, sizes=RAGGED)
    assert first == 0 and info == (len(raw), len(raw))
    assert np.array_equal(y, conditioner_ref.to_complex(raw).astype(np.complex64))
    D, T, f = 5, 64, -3.1e6
    taps = _taps(T, D)
    first, y, info, _ = _run(gctx, raw, fmt_name, D, taps, f, None)
    assert info == (len(raw), (len(raw) + D - 1) // D) and len(y) == info[1]
    want = conditioner_ref.condition(raw, taps, D, f, FS_IN)
    assert max(np.abs(y.real - want.real).max(), np.abs(y.imag - want.imag).max()) <= conditioner_ref.error_bound(taps, raw)
    ring = gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, 1, np.ones(1, np.float32), getattr(gnsscorr, "GC_IQ_" + fmt_name))
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        cond.blanking_info()
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    cond.close()
    ring.close()


def test_set_pulse_blanking_after_a_push_is_refused(gctx):
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, 1, np.ones(1, np.float32), gnsscorr.GC_IQ_F32)
    cond.set_pulse_blanking(length=16, segments_est=4)
    cond.set_pulse_blanking(length=8, segments_est=2, segments_reset=10, threshold=30.0)  # still before the first push: replaces it
    assert cond.blanking_info() == dict(segments_decided=0, segments_blanked=0, noise_power=0.0, n_segments=0, threshold=30.0)
    assert cond.push(np.ones(20, np.complex64)) == (0, 16)
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        cond.set_pulse_blanking(length=8)
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        cond.set_pulse_blanking(length=0)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    assert cond.blanking_info()["segments_decided"] == 2 and cond.info() == (20, 16)
    plain = gnsscorr.Conditioner(gctx, gnsscorr.IqStream(gctx, capacity_samples=8192, max_window_samples=1024), FS_IN, 0.0, 1, np.ones(1, np.float32))
    plain.push(np.ones(4, np.complex64))
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        plain.set_pulse_blanking()
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    plain.close()
    cond.close()
    ring.close()


def test_acquisition_of_a_pulsed_stream_with_and_without_blanking(gctx, oracle):
    """User level: a 4 Msps GPS L1 C/A stream under pulses of about 10 % duty (DME-like: 64 samples every 640, amplitude 20 against
    unit noise) is acquired through a conditioned ring in the copy configuration.  On the CPU (oracle PCPS on the restated streams)
    the blanked statistic is at least twice the unblanked one; on the GPU the blanked run finds the oracle's delay and Doppler cell
    and a larger statistic than the unblanked run."""
    import gnsscorr
    from helpers import synth_stream
    fs, n, prn = 4_000_000, 4000, 7
    L, est, reset = 32, 60, 5000000
    code = oracle.gps_l1_ca_code(prn).astype(np.float32)
    x, truth = synth_stream([code], fs, 3 * n, seed=31, cn0_db_hz=(50.0, 50.0), doppler_max=4000.0)
    k = np.arange(3 * n)
    pulse = (k >= 2000) & ((k - 2000) % 640 < 64)
    raw = (x + pulse * 20.0 * np.exp(2j * np.pi * 0.07 * k)).astype(np.complex64)
    thr = _threshold(L, 0.04)
    ref = blanking_ref.blank(raw, L, thr, est, reset)
    assert float(np.nanmin(np.abs(ref["ratio"] - 1.0))) >= 10.0 * blanking_ref.margin(L, est)
    blanked = blanking_ref.apply(raw, L, ref["flags"])
    sampled = oracle.gps_l1_ca_code_sampled(prn, fs)
    p = oracle.pcps(fs_in=fs, sampled_ms=1, ms_per_code=1, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=4000.0,
        samples_per_chip=4, doppler_max=5000, doppler_step=250)
    p.set_local_code(sampled)
    q_b, q_u = p.core(blanked[n:2 * n]), p.core(raw[n:2 * n])
    print("CPU: blanked statistic %.4f at (%d, %d Hz), unblanked %.4f; %d of %d segments blanked; true Doppler %.1f Hz" % (q_b.test_statistics, q_b.indext,
        q_b.doppler, q_u.test_statistics, ref["blanked"], ref["decided"], truth[0]["doppler"]))
    assert q_b.test_statistics >= 2.0 * q_u.test_statistics
    assert abs(q_b.doppler - truth[0]["doppler"]) <= 250.0

    got = []
    for on in (True, False):
        ring = gnsscorr.IqStream(gctx, capacity_samples=4 * n, max_window_samples=2 * n)
        cond = gnsscorr.Conditioner(gctx, ring, fs, 0.0, 1, np.ones(1, np.float32), gnsscorr.GC_IQ_F32)
        if on:
            cond.set_pulse_blanking(length=L, segments_est=est, segments_reset=reset)
        assert cond.push(raw) == (0, 3 * n)
        acq = gnsscorr.PcpsAcquisition(gctx, 1, fs, 1, 1, np.float32(fs) * np.float32(0.001), 4000.0, 4, 5000, 250)
        acq.set_local_code(0, sampled)
        got.append(acq.dwell_stream(ring, n)[0])
        acq.close()
        cond.close()
        ring.close()
    r_b, r_u = got
    print("GPU: blanked statistic %.4f at (%d, %d Hz), unblanked %.4f" % (r_b.test_statistics, r_b.indext, r_b.doppler_hz, r_u.test_statistics))
    assert (r_b.indext, r_b.doppler_hz) == (q_b.indext, q_b.doppler)
    assert r_b.test_statistics > r_u.test_statistics


def test_cpp_blanking_selftest():
    """The C++ drop-in layer: hip_signal_conditioner with the pulse_blanking keys (adapter/blanking_selftest.cpp)."""
    exe = os.path.join(ROOT, "gnss-sdr-1_amd", "adapter", "blanking_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "blanking_selftest"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "pulse blanking self-test passed" in p.stdout
