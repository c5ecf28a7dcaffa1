"""Mixed closed-loop engines (gc_trk_loop_set_mixed): GPS L1 C/A, BeiDou B1I and Galileo E1 channels -- 3 or 5 taps, data or
pilot tracking, 1 or 4 ms periods -- in ONE engine, one launch.  Each channel's records must equal, byte for byte, those of a
single-signal engine of its kind on the same input: the mixed kernel runs the same per-period body."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FC = 1575.42e6


def _conf(gnsscorr, **kw):
    c = gnsscorr.LoopConf()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _base(fs):
    return dict(fs_in=fs, signal_carrier_freq_hz=FC, carrier_lock_th=0.85, pull_in_time_s=2, pll_filter_order=3, dll_filter_order=2,
        enable_fll_pull_in=0, enable_fll_steady_state=0, cn0_samples=20, cn0_min=25, max_lock_fail=50, acq_samplestamp_samples=0, sample_counter=0)


def _kinds(gnsscorr, fs, with_l5=False):
    """(name, conf dict, replica, sync or None, data replica or None, truth doppler, truth delay [samples]) per channel kind."""
    n1 = int(round(fs * 1e-3))
    b = _base(fs)
    e1b = gnsscorr.galileo_e1_code_gen_sinboc11_float("1B", 11)
    e1c = gnsscorr.galileo_e1_code_gen_sinboc11_float("1C", 11)
    gal = dict(b, code_chip_rate_hz=1.023e6, code_period_s=0.004, code_length_chips=4092, code_samples_per_chip=2, vector_length=4 * n1,
        pll_bw_hz=15.0, dll_bw_hz=0.75, fll_bw_hz=10.0, early_late_space_chips=0.15, very_early_late_space_chips=0.6)
    pilot = gnsscorr.LoopSyncConf.make(extend_correlation_symbols=1, track_pilot=True, symbols_per_bit=1)
    kinds = [
        ("gps", dict(b, code_chip_rate_hz=1.023e6, code_period_s=0.001, code_length_chips=1023, code_samples_per_chip=1, vector_length=n1, veml=0,
            pll_bw_hz=40.0, dll_bw_hz=2.0, fll_bw_hz=35.0, early_late_space_chips=0.5), gnsscorr.gps_l1_ca_code_gen_float(7), None, None, 1234.0, 1500.3),
        ("bds", dict(b, code_chip_rate_hz=2.046e6, code_period_s=0.001, code_length_chips=2046, code_samples_per_chip=1, vector_length=n1, veml=0,
            pll_bw_hz=40.0, dll_bw_hz=2.0, fll_bw_hz=35.0, early_late_space_chips=0.5), gnsscorr.beidou_b1i_code_gen_float(9), None, None, -2210.0, 702.6),
        ("gal_data", dict(gal, veml=1), e1b, None, None, -1234.0, 5000.2),
        ("gal_pilot", dict(gal, veml=1), e1c, pilot, e1b, 871.0, 9123.7),
        # a 3-tap pilot channel (Galileo E1 with the very-early / very-late taps off)
        ("gal_pilot_3tap", dict(gal, veml=0, very_early_late_space_chips=0.0), e1c, pilot, e1b, 2345.0, 11003.1),
    ]
    if with_l5:
        l5q = gnsscorr.gps_l5q_code_gen_float(3)
        l5i = gnsscorr.gps_l5i_code_gen_float(3)
        kinds.append(("l5_pilot", dict(b, signal_carrier_freq_hz=1176.45e6, code_chip_rate_hz=10.23e6, code_period_s=0.001, code_length_chips=10230,
            code_samples_per_chip=1, vector_length=n1, veml=0, pll_bw_hz=30.0, dll_bw_hz=2.0, fll_bw_hz=35.0, early_late_space_chips=0.5),
            l5q, pilot, l5i, 432.0, 2100.4))
    return kinds


def _stream(kinds, fs, n, seed=5, cn0=48.0):
    """One RF stream carrying every kind's signal (no data bits) plus unit-variance noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    i = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    amp = np.sqrt(10 ** (cn0 / 10) / fs)
    for name, c, code, _sync, _dc, dop, delay in kinds:
        L = code.size
        spc = c["code_samples_per_chip"]
        fc = c["signal_carrier_freq_hz"]
        rate = c["code_chip_rate_hz"] * spc * (1 + dop / fc) / fs
        tau0 = L - delay * c["code_chip_rate_hz"] * spc / fs
        chip = np.floor(tau0 + i * rate).astype(np.int64) % L
        x = x + amp * code[chip] * np.exp(1j * (2 * np.pi * dop * i / fs + 0.3))
    return x.astype(np.complex64)


def _start(gnsscorr, eng, ch, kind, acq_err_hz=3.0):
    name, c, code, sync, dc, dop, delay = kind
    eng.set_sync(ch, sync, dc)
    eng.start(ch, _conf(gnsscorr, **dict(c, acq_delay_samples=float(delay), acq_doppler_hz=dop + acq_err_hz)), code)


def _same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _singles(gnsscorr, gctx, kinds, dev_ptr, n, n_ep, threads, fmt=None):
    out = []
    for kind in kinds:
        eng = gnsscorr.TrackingLoop(gctx, 1, kind[2].size)
        if fmt is not None:
            eng.set_input_format(fmt)
        eng.set_geometry(threads_per_workgroup=threads, slices_per_channel=1)
        eng.set_input_dev(0, dev_ptr, n)
        _start(gnsscorr, eng, 0, kind)
        out.append(eng.run(n_ep)[0])
        eng.close()
    return out


@pytest.mark.parametrize("threads", [1024, 256])
def test_mixed_engine_bit_identical_to_single_signal_engines(gctx, threads):
    """Five kinds interleaved in slot order (GPS, BeiDou, Galileo data 5 taps, Galileo pilot 5 taps, a 3-tap pilot) for 44 periods
    on device input, resident LDS image; then a GPS L5 pilot channel (10230 samples: over the resident rule) pushes the whole mixed
    engine, and the single L5 engine, onto the per-period window."""
    import gnsscorr
    import torch
    fs, n_ep = 4e6, 44
    for with_l5 in (False, True):
        kinds = _kinds(gnsscorr, fs, with_l5)
        n = int(fs * 0.004) * (n_ep + 2)
        x = _stream(kinds, fs, n)
        d = torch.from_numpy(x.view(np.float32)).cuda()
        want = _singles(gnsscorr, gctx, kinds, d.data_ptr(), n, n_ep, threads)
        mixed = gnsscorr.TrackingLoop(gctx, len(kinds), max(k[2].size for k in kinds), mixed=True)
        mixed.set_geometry(threads_per_workgroup=threads, slices_per_channel=1)
        for ch, kind in enumerate(kinds):
            mixed.set_input_dev(ch, d.data_ptr(), n)
            _start(gnsscorr, mixed, ch, kind)
        got = mixed.run(n_ep)
        mixed.close()
        for ch, kind in enumerate(kinds):
            assert np.all(want[ch]["valid"] == 1), kind[0]
            assert _same_bytes(got[ch], want[ch]), (kind[0], with_l5)
        # corr[] holds each channel's own tap count: 3-tap channels leave taps 3 and 4 zero
        assert np.all(got[0]["corr"][:, 6:] == 0) and np.any(got[2]["corr"][:, 6:] != 0)


def test_mixed_engine_on_a_ring(gctx):
    """The same five kinds reading one gc_stream ring, fed 10 ms at a time: long-period channels produce fewer valid records per
    launch, every record equals the single-signal engines', and sample_counter advances exactly by the block lengths."""
    import gnsscorr
    fs, n_ep, blk, n_blk = 4e6, 12, 40000, 16
    kinds = _kinds(gnsscorr, fs)
    x = _stream(kinds, fs, blk * n_blk, seed=9)
    ring_m = gnsscorr.IqStream(gctx, 1 << 20, 20000)
    ring_s = gnsscorr.IqStream(gctx, 1 << 20, 20000)
    mixed = gnsscorr.TrackingLoop(gctx, len(kinds), 8184, mixed=True)
    singles = []
    for ch, kind in enumerate(kinds):
        mixed.set_input_stream(ch, ring_m)
        _start(gnsscorr, mixed, ch, kind)
        eng = gnsscorr.TrackingLoop(gctx, 1, kind[2].size)
        eng.set_input_stream(0, ring_s)
        _start(gnsscorr, eng, 0, kind)
        singles.append(eng)
    valid = [[] for _ in kinds]
    for k in range(n_blk):
        ring_m.push(x[k * blk:(k + 1) * blk])
        ring_s.push(x[k * blk:(k + 1) * blk])
        got = mixed.run(n_ep)
        for ch, eng in enumerate(singles):
            want = eng.run(n_ep)[0]
            assert _same_bytes(got[ch], want), (kinds[ch][0], k)
            v = got[ch][got[ch]["valid"] == 1]
            valid[ch].append(v)
            if k >= 2:
                per = kinds[ch][1]["vector_length"]
                assert len(v) <= -(-blk // per) + 1 and len(v) >= blk // per - 1, (kinds[ch][0], k, len(v))
    for eng in singles:
        eng.close()
    mixed.close()
    ring_m.close()
    ring_s.close()
    counts = [sum(len(v) for v in vv) for vv in valid]
    assert counts[2] < counts[0] / 3 and counts[3] < counts[1] / 3, counts  # 4 ms channels: a quarter of the records
    for ch, vv in enumerate(valid):
        r = np.concatenate(vv)
        sc = r["sample_counter"].astype(np.int64)
        # one record per code period: the counter advances by exactly the period's block length, and never past the pushed samples
        assert np.array_equal(np.diff(sc), r["current_prn_length_samples"][1:].astype(np.int64)), kinds[ch][0]
        assert sc[-1] <= blk * n_blk and sc[-1] > blk * n_blk - 2 * kinds[ch][1]["vector_length"]


def test_mixed_slot_reuse_and_refusals(gctx):
    import gnsscorr
    import torch
    fs, n_ep = 4e6, 24
    kinds = _kinds(gnsscorr, fs)
    gps, gal_pilot = kinds[0], kinds[3]
    n = int(fs * 0.004) * (2 * n_ep + 2)
    x = _stream(kinds, fs, n, seed=13)
    d = torch.from_numpy(x.view(np.float32)).cuda()
    want_gps, want_gal = _singles(gnsscorr, gctx, [gps, gal_pilot], d.data_ptr(), n, n_ep, 1024)
    loop = gnsscorr.TrackingLoop(gctx, 3, 8184, mixed=True)
    for ch in range(3):
        loop.set_input_dev(ch, d.data_ptr(), n)
    _start(gnsscorr, loop, 0, gps)
    _start(gnsscorr, loop, 1, gal_pilot)
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        loop.set_mixed(False)
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    rec = loop.run(n_ep)
    assert np.all(rec[2].view(np.uint8) == 0)  # a standby slot: all-zero records
    assert _same_bytes(rec[0], want_gps) and _same_bytes(rec[1], want_gal)
    # stop the GPS slot (standby records) and start a Galileo pilot channel in it; then the reverse in the Galileo slot (both restart
    # from the beginning of their blocks)
    loop.stop(0)
    rec = loop.run(2)
    assert np.all(rec[0].view(np.uint8) == 0) and np.all(rec[1]["valid"] == 1)
    _start(gnsscorr, loop, 0, gal_pilot)
    loop.stop(1)
    _start(gnsscorr, loop, 1, gps)
    rec = loop.run(n_ep)
    assert _same_bytes(rec[0], want_gal) and _same_bytes(rec[1], want_gps) and np.all(rec[2].view(np.uint8) == 0)
    # high_dyn stays engine-wide in a mixed engine
    with pytest.raises(gnsscorr.GnsscorrError, match="high_dyn mode"):
        hd = dict(kinds[1][1], high_dyn_smoother_length=4, acq_delay_samples=0.0, acq_doppler_hz=0.0)
        loop.start(2, _conf(gnsscorr, **hd), kinds[1][2])
    loop.close()
    # a default engine keeps both checks
    loop = gnsscorr.TrackingLoop(gctx, 2, 8184)
    for ch in range(2):
        loop.set_input_dev(ch, d.data_ptr(), n)
    _start(gnsscorr, loop, 0, gps)
    with pytest.raises(gnsscorr.GnsscorrError, match="tap count"):
        _start(gnsscorr, loop, 1, kinds[2])
    with pytest.raises(gnsscorr.GnsscorrError, match="pilot mode"):
        _start(gnsscorr, loop, 1, kinds[4])
    loop.close()


def test_mixed_high_dynamics_and_int16(gctx):
    """An all-high_dyn mixed engine (GPS + Galileo pilot) and a GC_IQ_I16 mixed engine (all five kinds), each bit-identical to
    the single-signal engines of the same mode and format."""
    import gnsscorr
    import torch
    fs, n_ep = 4e6, 40
    kinds = _kinds(gnsscorr, fs)
    n = int(fs * 0.004) * (n_ep + 2)
    x = _stream(kinds, fs, n, seed=21)
    d = torch.from_numpy(x.view(np.float32)).cuda()
    hd_kinds = [(k[0], dict(k[1], high_dyn_smoother_length=8, pull_in_time_s=0)) + k[2:] for k in (kinds[0], kinds[3])]
    want = _singles(gnsscorr, gctx, hd_kinds, d.data_ptr(), n, n_ep, 0)
    mixed = gnsscorr.TrackingLoop(gctx, 2, 8184, mixed=True)
    for ch, kind in enumerate(hd_kinds):
        mixed.set_input_dev(ch, d.data_ptr(), n)
        _start(gnsscorr, mixed, ch, kind)
    got = mixed.run(n_ep)
    mixed.close()
    for ch, kind in enumerate(hd_kinds):
        assert np.all(want[ch]["valid"] == 1) and _same_bytes(got[ch], want[ch]), kind[0]

    q = np.clip(np.round(x.view(np.float32) * 600.0), -32768, 32767).astype(np.int16)
    d16 = torch.from_numpy(q).cuda()
    want = _singles(gnsscorr, gctx, kinds, d16.data_ptr(), n, n_ep, 0, fmt=gnsscorr.GC_IQ_I16)
    mixed = gnsscorr.TrackingLoop(gctx, len(kinds), 8184, mixed=True)
    mixed.set_input_format(gnsscorr.GC_IQ_I16)
    for ch, kind in enumerate(kinds):
        mixed.set_input_dev(ch, d16.data_ptr(), n)
        _start(gnsscorr, mixed, ch, kind)
    got = mixed.run(n_ep)
    mixed.close()
    for ch, kind in enumerate(kinds):
        assert np.all(want[ch]["valid"] == 1) and _same_bytes(got[ch], want[ch]), kind[0]


def test_mixed_cfg5_share_locks(gctx):
    """One GPU's share of a GPS L1 C/A + Galileo E1 + BeiDou B1I receiver -- 16 + 8 + 8 channels at 25 Msps, 64 ms -- in ONE
    mixed engine: every channel locks; GPS and BeiDou fill 63-64 records, the 4 ms Galileo channels 15-16 (no timing here)."""
    import gnsscorr
    import torch
    fs, n_ep = 25e6, 64
    n1 = 25000
    b = _base(fs)
    gps_c = dict(b, code_chip_rate_hz=1.023e6, code_period_s=0.001, code_length_chips=1023, code_samples_per_chip=1, vector_length=n1, veml=0,
        pll_bw_hz=40.0, dll_bw_hz=2.0, fll_bw_hz=35.0, early_late_space_chips=0.5)
    bds_c = dict(gps_c, code_chip_rate_hz=2.046e6, code_length_chips=2046)
    gal_c = dict(b, code_chip_rate_hz=1.023e6, code_period_s=0.004, code_length_chips=4092, code_samples_per_chip=2, vector_length=4 * n1, veml=1,
        pll_bw_hz=15.0, dll_bw_hz=0.75, fll_bw_hz=10.0, early_late_space_chips=0.15, very_early_late_space_chips=0.6)
    rng = np.random.Generator(np.random.PCG64(2024))
    kinds = []
    for k in range(16):
        kinds.append(("gps", gps_c, gnsscorr.gps_l1_ca_code_gen_float(k + 1), None, None, float(rng.uniform(-4000, 4000)), float(rng.uniform(1000, n1 - 1000))))
    for k in range(8):
        kinds.append(("gal", gal_c, gnsscorr.galileo_e1_code_gen_sinboc11_float("1B", k + 1), None, None, float(rng.uniform(-4000, 4000)),
            float(rng.uniform(1000, 4 * n1 - 4000))))
    for k in range(8):
        kinds.append(("bds", bds_c, gnsscorr.beidou_b1i_code_gen_float(k + 6), None, None, float(rng.uniform(-4000, 4000)), float(rng.uniform(1000, n1 - 1000))))
    # 64 records of capacity; the stream runs 4 ms past them, since the pull-in skips up to a code period plus the code phase
    n = (n_ep + 4) * n1
    x = _stream(kinds, fs, n, seed=31, cn0=50.0)
    d = torch.from_numpy(x.view(np.float32)).cuda()
    loop = gnsscorr.TrackingLoop(gctx, len(kinds), 8184, mixed=True)
    for ch, kind in enumerate(kinds):
        loop.set_input_dev(ch, d.data_ptr(), n)
        _start(gnsscorr, loop, ch, kind, acq_err_hz=2.0)
    rec = loop.run(n_ep)
    loop.close()
    for ch, kind in enumerate(kinds):
        r = rec[ch][rec[ch]["valid"] == 1]
        lo, hi = (15, 16) if kind[0] == "gal" else (63, 64)
        assert lo <= len(r) <= hi, (ch, kind[0], len(r))
        tail = r[-4:] if kind[0] == "gal" else r[-10:]
        assert abs(float(tail["carrier_doppler_hz"].mean()) - kind[5]) < 3.0, (ch, kind[0], tail["carrier_doppler_hz"], kind[5])
        assert np.all(rec[ch]["valid"][len(r):] == 0)  # after the input ends: invalid records


def test_cpp_hybrid_tracking_group():
    """The C++ drop-in layer: ONE hip_tracking_group over GPS L1 C/A, Galileo E1 and BeiDou B1I slots on one ring (one mixed engine)
    hands out the same Gnss_Synchro items as three per-signal groups given the same hand-overs (adapter/hybrid_group_selftest.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "gnss-sdr-1_amd", "adapter", "hybrid_group_selftest")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe), "hybrid_group_selftest"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "hybrid group self-test passed" in p.stdout and " 0 differing" in p.stdout
