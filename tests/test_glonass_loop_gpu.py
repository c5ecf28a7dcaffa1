"""GPU tests of the GLONASS L1 / L2 C/A device loop (gc_trk_loop_start_glonass, csrc/trk_closed_loop_glonass.hip).

Scenarios, streams and the checker come from tests/glonass_loop_ref.py; tests/test_glonass_loop_ref.py has already held the
checker's filters to the reference's compiled ones and every scenario to "keeps lock, K_blk_samples >= 1e-3 sample away from a
half-integer in every period", so a last-bit difference in a correlator sum cannot move a block boundary here.  All cases run 60
periods; the samples are integers in -127..127, so the I16 and I8 engines read what the F32 engine reads as floats.
  B.1  the F32 / 1024-thread engine against the restatement, at the gates of tests/test_loop_sync_gpu.py::_compare;
  B.2  every other instantiation against that anchor, at the gates of tests/test_closed_loop_matrix_gpu.py;
  B.3  the loop maths on its own: pinned filters fed the device's recorded discriminator outputs, bit for bit; the discriminators
       on the device's own taps;
  B.4  ring input in uneven pushes, byte-identical to the bound block; a second channel on the ring unaffected by the first;
  B.5  loss of lock, restart, the refusals, and the veml path left alone."""
import numpy as np
import pytest

import glonass_loop_ref as R

pytestmark = pytest.mark.gpu
SUM_GATE, DOPPLER_GATE_HZ = 2e-5, 0.02  # tests/test_closed_loop_matrix_gpu.py
OTHERS = [(f, t) for f in ("f32", "i16", "i8") for t in (1024, 512, 256) if (f, t) != ("f32", 1024)]


def _conf(gnsscorr, d):
    c = gnsscorr.GlonassLoopConf()
    for k, v in d.items():
        setattr(c, k, v)
    return c


def _device_samples(x, fmt):
    import torch
    if fmt == "f32":
        host = x.view(np.float32)
    else:
        host = np.stack([x.real, x.imag], axis=1).astype(np.int16 if fmt == "i16" else np.int8)
        assert np.array_equal(host[:, 0], x.real) and np.array_equal(host[:, 1], x.imag)
    return torch.from_numpy(np.ascontiguousarray(host)).cuda()


@pytest.fixture(scope="module")
def glonass_code(oracle):
    return oracle.glonass_l1_ca_code().astype(np.float32)


@pytest.fixture(scope="module")
def bench(gctx, oracle, glonass_code):
    """What the tests share, computed once and never modified: streams, restatement runs, engine records."""
    import gnsscorr
    fmt_id = {"f32": gnsscorr.GC_IQ_F32, "i16": gnsscorr.GC_IQ_I16, "i8": gnsscorr.GC_IQ_I8}

    class Bench:
        def __init__(self):
            self.streams, self.refs, self.recs = {}, {}, {}

        def stream(self, name):
            if name not in self.streams:
                self.streams[name] = R.scenario_stream(glonass_code, R.NOISE_ONLY if name == "noise" else R.SCENARIOS[name])
            return self.streams[name]

        def ref(self, name):
            if name not in self.refs:
                self.refs[name] = R.run(oracle, self.stream(name), glonass_code, R.scenario_conf(R.SCENARIOS[name]), R.N_PERIODS)
            return self.refs[name]

        def engine(self, x, conf, fmt="f32", threads=1024, n_periods=R.N_PERIODS):
            d = _device_samples(x, fmt)
            loop = gnsscorr.TrackingLoop(gctx, 1, 511)
            try:
                loop.set_input_format(fmt_id[fmt])
                loop.set_geometry(threads_per_workgroup=threads, slices_per_channel=1)
                loop.set_input_dev(0, d.data_ptr(), x.size)
                loop.start_glonass(0, _conf(gnsscorr, conf))
                return loop.run(n_periods)[0]
            finally:
                loop.close()

        def rec(self, name, fmt="f32", threads=1024):
            k = (name, fmt, threads)
            if k not in self.recs:
                self.recs[k] = self.engine(self.stream(name), R.scenario_conf(R.SCENARIOS[name]), fmt, threads)
                self.recs[k].flags.writeable = False
            return self.recs[k]

    return Bench()


def _taps(g):
    return g["corr"][0:6:2] + 1j * g["corr"][1:6:2]


def _compare(rec, ref, tol=3e-3):
    """The gates of tests/test_loop_sync_gpu.py::_compare (fixed scenarios: its abs_tol is 0) on the GLONASS record layout."""
    assert len(ref) == len(rec)
    for k in range(len(ref)):
        r, g = ref[k], rec[k]
        assert int(g["state"]) == r["state"], (k, int(g["state"]), r["state"])
        assert int(g["sample_counter"]) == r["sample_counter"], (k, int(g["sample_counter"]), r["sample_counter"])
        assert int(g["current_prn_length_samples"]) == r["cur"], (k, int(g["current_prn_length_samples"]), r["cur"])
        assert int(g["valid"]) == 1 and int(g["integrating"]) == 0 and int(g["extend_count"]) == 0, k
        scale = abs(r["corr"][1]) + 1e-9
        gc = _taps(g)
        assert np.max(np.abs(gc - r["corr"])) <= tol * scale, (k, gc, r["corr"])
        assert np.array_equal(g["accu"][:6], g["corr"][:6]) and np.all(g["accu"][6:] == 0) and np.all(g["corr"][6:] == 0), k
        assert np.array_equal(g["prompt_data"], g["corr"][2:4]), k
        assert abs(float(g["carrier_doppler_hz"]) - r["doppler"]) < 0.05, (k, float(g["carrier_doppler_hz"]), r["doppler"])
        assert abs(float(g["code_freq_chips"]) - r["code_freq"]) < 0.05, k
        perr_own, cerr_own = R.discriminators(*gc)
        assert abs(float(g["code_error_chips"]) - cerr_own) < 2e-5, (k, float(g["code_error_chips"]), cerr_own)
        assert abs(float(g["carr_phase_error_hz"]) - perr_own) < 2e-6, (k, float(g["carr_phase_error_hz"]), perr_own)
        assert abs(float(g["code_error_chips"]) - r["cerr"]) < 3e-3, (k, float(g["code_error_chips"]), r["cerr"])
        assert abs(float(g["cn0_db_hz"]) - r["cn0"]) < 0.05 and abs(float(g["carrier_lock_test"]) - r["lock_test"]) < 2e-3, k
        assert abs(float(g["rem_code_phase_samples"]) - r["rem_code_samples"]) < 1e-3 and abs(float(g["acc_carrier_phase_rad"]) - r["acc_phase"]) < 0.05, k


@pytest.mark.parametrize("name", sorted(R.SCENARIOS))
def test_anchor_engine_against_the_restatement(bench, name):
    """B.1"""
    rec, ref = bench.rec(name), bench.ref(name)
    assert len(ref) == R.N_PERIODS
    _compare(rec, ref)
    sc = R.SCENARIOS[name]
    # the Doppler carries no FDMA offset; the pull-in emitted no record: the first one is a tracked period
    assert abs(float(rec["carrier_doppler_hz"][-1]) - sc["doppler"]) < 1.0
    assert int(rec["sample_counter"][0]) == ref[0]["pull_in"]["sample_counter"] + ref[0]["cur"]
    assert len(set(rec["cn0_db_hz"].tolist())) == 6  # the C/N0 branch ran five times


@pytest.mark.parametrize("fmt,threads", OTHERS, ids=["%s-%d" % ft for ft in OTHERS])
def test_every_instantiation_against_the_anchor(bench, fmt, threads):
    """B.2"""
    for name in sorted(R.SCENARIOS):
        a, g = bench.rec(name), bench.rec(name, fmt, threads)
        for f in ("state", "valid", "sample_counter", "current_prn_length_samples", "integrating", "extend_count"):
            assert np.array_equal(a[f], g[f]), (name, f)
        scale = float(np.max(np.hypot(a["corr"][:, 0:6:2], a["corr"][:, 1:6:2])))
        for f in ("corr", "accu", "prompt_data"):
            err = float(np.max(np.abs(a[f] - g[f]))) / scale
            assert err <= SUM_GATE, (name, f, err)
        dop = float(np.max(np.abs(a["carrier_doppler_hz"] - g["carrier_doppler_hz"])))
        assert dop <= DOPPLER_GATE_HZ, (name, dop)


@pytest.mark.parametrize("name", sorted(R.SCENARIOS))
def test_device_filters_against_the_pinned_filters(bench, name):
    """B.3: the pinned filters, fed the device's recorded discriminator outputs, reproduce the recorded filter outputs bit for bit;
    the discriminators on the device's own taps give the device's outputs."""
    rec = bench.rec(name)
    conf = R.scenario_conf(R.SCENARIOS[name])
    pll, dll = R.pll_filter(conf["pll_bw_hz"]), R.dll_filter(conf["dll_bw_hz"])
    want_p = np.array([pll.step(v) for v in rec["carr_phase_error_hz"]], np.float32)
    want_d = np.array([dll.step(v) for v in rec["code_error_chips"]], np.float32)
    assert np.array_equal(want_p.view(np.uint32), rec["carr_error_filt_hz"].view(np.uint32)), np.flatnonzero(want_p != rec["carr_error_filt_hz"])[:5]
    assert np.array_equal(want_d.view(np.uint32), rec["code_error_filt_chips"].view(np.uint32)), np.flatnonzero(want_d != rec["code_error_filt_chips"])[:5]
    assert np.any(rec["carr_error_filt_hz"] != 0) and np.any(rec["code_error_filt_chips"] != 0)
    for k, g in enumerate(rec):
        perr_own, cerr_own = R.discriminators(*_taps(g))
        assert abs(float(g["code_error_chips"]) - cerr_own) < 2e-5 and abs(float(g["carr_phase_error_hz"]) - perr_own) < 2e-6, k


def test_ring_input_in_uneven_pushes(gctx, bench, glonass_code):
    """B.4"""
    import gnsscorr
    x = R.ring_pair_stream(glonass_code)
    confs = [R.scenario_conf(R.RING_PAIR[w]) for w in ("A", "B")]
    alone = [bench.engine(x, c) for c in confs]
    for a in alone:
        assert np.all(a["valid"] == 1) and np.all(a["state"] == 2)
    vl = 6625
    ring = gnsscorr.IqStream(gctx, 16 * vl, 2 * vl)
    loop = gnsscorr.TrackingLoop(gctx, 3, 511)  # slot 2 stays in standby
    loop.set_geometry(threads_per_workgroup=1024, slices_per_channel=1)
    for ch in (0, 1):
        loop.set_input_stream(ch, ring)
    loop.start_glonass(0, _conf(gnsscorr, confs[0]))
    got = [[], []]
    sizes = [3000, 9000, 500, 13250, 6625, 100, 20000, 1, 6624, 7000]
    pos, i, runs = 0, 0, 0
    while pos < x.size:
        n = min(sizes[i % len(sizes)], x.size - pos)
        ring.push(x[pos:pos + n])
        pos, i = pos + n, i + 1
        if runs == 2:
            loop.start_glonass(1, _conf(gnsscorr, confs[1]))  # joins while channel 0 runs; it starts at stream sample 0, still resident
        rec = loop.run(5)
        runs += 1
        assert np.all(rec[2].view(np.uint8) == 0)
        for ch in (0, 1):
            valid = rec[ch][rec[ch]["valid"] == 1]
            # a launch stops at its first incomplete period: valid records first, then invalid ones that carry state and position only
            assert np.all(rec[ch]["valid"][:len(valid)] == 1)
            z = rec[ch][len(valid):].copy()
            z["state"], z["sample_counter"] = 0, 0
            assert np.all(z.view(np.uint8) == 0)
            got[ch].append(valid)
    loop.close()
    for ch in (0, 1):
        g = np.concatenate(got[ch])
        assert len(g) >= R.N_PERIODS, (ch, len(g))
        n = min(len(g), len(alone[ch]))
        assert g[:n].tobytes() == alone[ch][:n].tobytes(), (ch, np.flatnonzero(g[:n] != alone[ch][:n])[:5])


def test_rebinding_a_running_channel_continues_the_run(gctx, bench):
    """gc_trk_loop_set_input_dev on a running GLONASS channel keeps its state and restarts its position at 0: bound to the rest of
    the same buffer (from the sample the channel would read next) it reads the same addresses, so the records continue byte for byte
    those of an engine that ran the same two launches without the rebind."""
    import gnsscorr
    name, k = "2048k_L1_km1", 25
    x, conf = bench.stream(name), R.scenario_conf(R.SCENARIOS[name])
    d = _device_samples(x, "f32")

    def engine():
        loop = gnsscorr.TrackingLoop(gctx, 1, 511)
        loop.set_geometry(threads_per_workgroup=1024, slices_per_channel=1)
        loop.set_input_dev(0, d.data_ptr(), x.size)
        loop.start_glonass(0, _conf(gnsscorr, conf))
        return loop, loop.run(k)[0]

    a, a_first = engine()
    pos = int(a_first["sample_counter"][-1]) - conf["sample_counter"]
    assert 0 < pos < x.size
    a.set_input_dev(0, d.data_ptr() + pos * 8, x.size - pos)
    got = np.concatenate([a_first, a.run(R.N_PERIODS - k)[0]])
    a.close()
    b, b_first = engine()
    want = np.concatenate([b_first, b.run(R.N_PERIODS - k)[0]])
    b.close()
    assert np.all(want["valid"] == 1) and np.all(want["state"] == 2)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:5]


GPS = dict(fs_in=4e6, signal_carrier_freq_hz=1575.42e6, code_chip_rate_hz=1.023e6, code_period_s=0.001, carrier_lock_th=0.85, code_length_chips=1023,
    code_samples_per_chip=1, vector_length=4000, pull_in_time_s=0, veml=0, pll_filter_order=3, dll_filter_order=2, enable_fll_pull_in=0,
    enable_fll_steady_state=0, cn0_samples=20, cn0_min=25, max_lock_fail=50, pll_bw_hz=40.0, dll_bw_hz=2.0, fll_bw_hz=35.0, early_late_space_chips=0.5,
    very_early_late_space_chips=0.0, acq_samplestamp_samples=0, sample_counter=0, acq_delay_samples=1234.0, acq_doppler_hz=999.0)


def _gps_stream(code):
    rng = np.random.Generator(np.random.PCG64(31))
    n = 4000 * 23
    i = np.arange(n)
    chip = np.floor((1023 - 1234.0 * 1.023e6 / 4e6) + i * (1.023e6 * (1 + 1000.0 / 1575.42e6) / 4e6)).astype(np.int64) % 1023
    x = 0.2 * code[chip] * np.exp(1j * (2 * np.pi * 1000.0 * i / 4e6 + 0.3)) + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    return x.astype(np.complex64)


def test_loss_of_lock_restart_and_engine_kinds(gctx, oracle, bench, glonass_code):
    """B.5"""
    import gnsscorr
    import torch
    gps_code = oracle.gps_l1_ca_code(5).astype(np.float32)
    gx = _gps_stream(gps_code)
    gd = torch.from_numpy(gx.view(np.float32)).cuda()
    gps_conf = gnsscorr.LoopConf()
    for k, v in GPS.items():
        setattr(gps_conf, k, v)

    def veml_run():
        loop = gnsscorr.TrackingLoop(gctx, 1, 1023)
        loop.set_input_dev(0, gd.data_ptr(), gx.size)
        loop.start(0, gps_conf, gps_code)
        rec = loop.run(20)
        loop.close()
        return rec

    before = veml_run()
    assert np.all(before["valid"] == 1)

    # loss of lock on noise only, at the period the restatement names
    conf = R.scenario_conf(R.NOISE_ONLY, max_lock_fail=2, cn0_samples=4)
    x = bench.stream("noise")
    ref = R.run(oracle, x, glonass_code, conf, R.N_PERIODS)
    n = len(ref)
    assert 0 < n < R.N_PERIODS and ref[-1]["state"] == 0
    d = _device_samples(x, "f32")
    loop = gnsscorr.TrackingLoop(gctx, 2, 1023)
    loop.set_geometry(threads_per_workgroup=1024, slices_per_channel=1)
    loop.set_input_dev(0, d.data_ptr(), x.size)
    loop.start_glonass(0, _conf(gnsscorr, conf))
    rec = loop.run(R.N_PERIODS)[0]
    assert np.all(rec["valid"][:n] == 1) and np.all(rec["state"][:n - 1] == 2) and rec["state"][n - 1] == 0
    assert [int(v) for v in rec["sample_counter"][:n]] == [r["sample_counter"] for r in ref]
    assert [int(v) for v in rec["current_prn_length_samples"][:n]] == [r["cur"] for r in ref]
    tail = rec[n:].copy()
    assert np.all(tail["state"] == 0) and np.all(tail["sample_counter"] == ref[-1]["sample_counter"])
    tail["sample_counter"] = 0
    assert np.all(tail.view(np.uint8) == 0)
    assert np.all(loop.run(3)[0]["valid"] == 0)  # and it stays there, consuming nothing

    # a veml start while a GLONASS channel runs (a channel that lost lock still runs until it is stopped), and the refusal leaves it alone
    loop.set_input_dev(1, gd.data_ptr(), gx.size)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        loop.start(1, gps_conf, gps_code)
    assert e.value.status == gnsscorr.GC_ERR_STATE

    # stop, then start_glonass on the slot: it tracks again
    name = "2048k_L1_km1"
    sx = bench.stream(name)
    sd = _device_samples(sx, "f32")
    loop.stop(0)
    loop.set_input_dev(0, sd.data_ptr(), sx.size)
    loop.start_glonass(0, _conf(gnsscorr, R.scenario_conf(R.SCENARIOS[name])))
    again = loop.run(R.N_PERIODS)[0]
    assert again.tobytes() == bench.rec(name).tobytes()

    # every GLONASS channel stopped: the engine takes veml channels again, and then refuses a GLONASS start
    loop.stop(0)
    loop.start(1, gps_conf, gps_code)
    assert loop.run(20)[1].tobytes() == before[0].tobytes()
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        loop.start_glonass(0, _conf(gnsscorr, R.scenario_conf(R.SCENARIOS[name])))
    assert e.value.status == gnsscorr.GC_ERR_STATE
    loop.close()

    # a mixed engine has no GLONASS slots
    mixed = gnsscorr.TrackingLoop(gctx, 1, 1023, mixed=True)
    mixed.set_input_dev(0, sd.data_ptr(), sx.size)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        mixed.start_glonass(0, _conf(gnsscorr, R.scenario_conf(R.SCENARIOS[name])))
    assert e.value.status == gnsscorr.GC_ERR_STATE
    mixed.close()

    # ring input: two block lengths must fit the stream's window
    ring = gnsscorr.IqStream(gctx, 16 * 2048, 2 * 2048 - 1)
    small = gnsscorr.TrackingLoop(gctx, 1, 511)
    small.set_input_stream(0, ring)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        small.start_glonass(0, _conf(gnsscorr, R.scenario_conf(R.SCENARIOS[name])))
    assert e.value.status == gnsscorr.GC_ERR_INVALID
    small.close()

    # the veml path is left alone
    assert veml_run().tobytes() == before.tobytes()
