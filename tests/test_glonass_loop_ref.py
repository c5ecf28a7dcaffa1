"""CPU tests (no GPU) of the GLONASS device loop's checker and ABI.

  * tests/glonass_loop_ref.py's second-order filters are held BIT FOR BIT to the reference's compiled Tracking_2nd_DLL_filter /
    Tracking_2nd_PLL_filter (the s2_* / dll2_* / pll2_* scripts of tests/golden/ref_loop_filters.npz, the pin of
    tests/test_loop_filter_pin.py::test_adapter_second_order_filters_are_bit_exact), so the GPU parity of the loop rests on pinned filters;
  * every fixed-seed scenario the GPU tests use is checked here first: the restatement reaches and keeps lock, its Doppler ends
    within 1 Hz of the truth, and K_blk_samples stays at least 1e-3 sample away from a half-integer in EVERY period, so that a
    last-bit difference in a correlator sum cannot move a block boundary; the noise-only scenario loses lock inside the run;
  * gc_glonass_loop_conf has the size of its ctypes mirror, and the argument checks that need no device answer GC_ERR_INVALID."""
import ctypes as C
import os

import numpy as np
import pytest

import glonass_loop_ref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_second_order_filters_are_bit_exact():
    z = np.load(os.path.join(G, "ref_loop_filters.npz"))
    assert int(z["n_second_order"]) == 5
    for i in range(int(z["n_second_order"])):
        bw, pdi, bw2, pdi2 = (float(v) for v in z["s2_%d_conf" % i])
        e = z["s2_%d_in" % i]
        for name, make in (("dll2", R.dll_filter), ("pll2", R.pll_filter)):
            want = z["%s_%d_out" % (name, i)]
            f = make(bw, pdi)
            got = np.zeros(len(want), np.float32)
            for k in range(len(e)):
                if k == len(e) // 2:
                    f.set_pdi(pdi2)
                    f.set_bw(bw2)
                got[k] = f.step(e[k])
            assert np.array_equal(_bits(got), _bits(want)), ("%s script %d" % (name, i), np.flatnonzero(_bits(got) != _bits(want))[:5])


@pytest.fixture(scope="module")
def glonass_code(oracle):
    return oracle.glonass_l1_ca_code().astype(np.float32)


@pytest.mark.parametrize("name", sorted(R.SCENARIOS))
def test_scenario_keeps_lock_away_from_block_boundaries(oracle, glonass_code, name):
    sc = R.SCENARIOS[name]
    x = R.scenario_stream(glonass_code, sc)
    conf = R.scenario_conf(sc)
    assert abs(conf["channel_offset_hz"] + sc["doppler"]) < sc["fs"] / 2
    assert conf["acq_delay_samples"] != 0
    ref = R.run(oracle, x, glonass_code, conf, R.N_PERIODS)
    assert len(ref) == R.N_PERIODS and all(r["valid"] == 1 and r["state"] == 2 for r in ref)
    assert abs(ref[-1]["doppler"] - sc["doppler"]) < 1.0, ref[-1]["doppler"]
    margin = min(abs((r["K_blk"] % 1.0) - 0.5) for r in ref)
    assert margin >= 1e-3, margin
    # the C/N0 branch ran five times (cn0_samples = 10: periods 10, 21, 32, 43, 54) and saw the signal
    assert len({r["cn0"] for r in ref}) == 6 and ref[-1]["cn0"] > 45.0 and ref[-1]["lock_test"] > 0.85


@pytest.mark.parametrize("which", ["A", "B"])
def test_ring_pair_stream_keeps_both_channels_in_lock(oracle, glonass_code, which):
    sc = R.RING_PAIR[which]
    ref = R.run(oracle, R.ring_pair_stream(glonass_code), glonass_code, R.scenario_conf(sc), R.N_PERIODS)
    assert len(ref) == R.N_PERIODS and all(r["valid"] == 1 and r["state"] == 2 for r in ref)
    assert abs(ref[-1]["doppler"] - sc["doppler"]) < 1.0, ref[-1]["doppler"]
    assert min(abs((r["K_blk"] % 1.0) - 0.5) for r in ref) >= 1e-3


@pytest.mark.parametrize("name", sorted(R.SCENARIOS) + ["noise"])
def test_library_pull_in_against_the_restatement(name):
    """gc_glonass_loop_pull_in (the statements the kernel runs, on the host: what the adapters build the pull-in item from) against
    the restatement's start_tracking + pull-in, the scenario that starts a few periods and a bit after its acquisition stamp included."""
    import gnsscorr
    conf = R.scenario_conf(R.NOISE_ONLY if name == "noise" else R.SCENARIOS[name])
    c = gnsscorr.GlonassLoopConf()
    for k, v in conf.items():
        setattr(c, k, v)
    offset, counter, phase = gnsscorr.glonass_loop_pull_in(c)
    want = R.start(conf)["pull_in"]
    assert (offset, counter) == (want["samples_offset"], want["sample_counter"]) and offset > 0
    assert phase == want["acc_phase"]
    assert gnsscorr.load_library().gc_glonass_loop_pull_in(None, None, None, None) == gnsscorr.GC_ERR_INVALID


def test_scenario_ahead_starts_a_few_periods_and_a_bit_after_the_stamp():
    sc = R.SCENARIOS["6625k_L1_kp4_ahead"]
    ahead = sc["sample_counter"] - sc["acq_stamp"]
    assert ahead // 6625 == 3 and ahead % 6625 != 0


def test_noise_only_scenario_loses_lock(oracle, glonass_code):
    sc = R.NOISE_ONLY
    x = R.scenario_stream(glonass_code, sc)
    ref = R.run(oracle, x, glonass_code, R.scenario_conf(sc, max_lock_fail=2, cn0_samples=4), R.N_PERIODS)
    assert 0 < len(ref) < R.N_PERIODS and ref[-1]["state"] == 0 and all(r["state"] == 2 for r in ref[:-1])
    # an estimate every cn0_samples + 1 periods; max_lock_fail = 2 needs at least three failed ones
    assert len(ref) % 5 == 0 and len(ref) >= 15
    assert min(abs((r["K_blk"] % 1.0) - 0.5) for r in ref) >= 1e-3


def test_conf_size_and_argument_checks_without_a_device():
    import gnsscorr
    lib = gnsscorr.load_library()
    assert lib.gc_glonass_loop_conf_size() == C.sizeof(gnsscorr.GlonassLoopConf) == 96
    good = dict(R.scenario_conf(R.SCENARIOS["2048k_L1_km1"]))

    def status(**kw):
        c = gnsscorr.GlonassLoopConf()
        for k, v in dict(good, **kw).items():
            setattr(c, k, v)
        return lib.gc_trk_loop_start_glonass(None, 0, C.byref(c)), lib.gc_last_error().decode()

    assert lib.gc_trk_loop_start_glonass(None, 0, None) == gnsscorr.GC_ERR_INVALID
    # a good configuration gets as far as the handle
    st, msg = status()
    assert st == gnsscorr.GC_ERR_INVALID and "NULL handle" in msg
    for bad, word in ((dict(cn0_samples=0), "cn0_samples"), (dict(cn0_samples=65), "cn0_samples"), (dict(fs_in=0.0), "fs_in"), (dict(fs_in=2048000.5), "fs_in"),
            (dict(vector_length=0), "vector_length"), (dict(vector_length=1000), "2 * vector_length"), (dict(pll_bw_hz=0.0), "bandwidths"),
            (dict(dll_bw_hz=-1.0), "bandwidths"), (dict(early_late_space_chips=0.0), "early_late_space_chips"), (dict(band_carrier_freq_hz=0.0), "carrier"),
            (dict(acq_doppler_hz=float("nan")), "hand-over"), (dict(acq_samplestamp_samples=10, sample_counter=5), "sample_counter")):
        st, msg = status(**bad)
        assert st == gnsscorr.GC_ERR_INVALID and word in msg, (bad, st, msg)
    with pytest.raises(gnsscorr.GnsscorrError):
        gnsscorr.TrackingLoop.start_glonass(type("H", (), {"_h": None})(), 0, gnsscorr.GlonassLoopConf())
