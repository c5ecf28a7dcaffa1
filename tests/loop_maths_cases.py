"""The loop-maths matrix (test infrastructure): the case table and the replay shared by tests/test_loop_maths_inputs.py (CPU) and
tests/test_loop_maths_gpu.py.  Where the closed-loop matrix (closed_loop_matrix_cases.py) varies the kernel and holds the loop
configuration fixed, this one holds the kernel fixed and varies what trk_loop_device.hpp computes once per code period: every order of
the code and carrier loop filters, the FLL in each of its modes, the narrow-stage re-design, pilot tracking and an all-zero input.

Shape: the closed-loop matrix's (fs = 5.001 MHz, 5001 samples per 1 ms period, 50 dB-Hz); 3 taps on a random 1023-sample code, 5 taps
on 2046 samples at 2 per chip; 96 periods and cn0_samples = 10, so eight C/N0 estimates at one update per period.  Every channel of a
tap count reads one signal; the pilot channels read it with a data component added, group D reads zeros.

Channels per tap count:
  A  24  dll_filter_order {1, 2, 3} x pll_filter_order {2, 3} x FLL {off, pull-in only, steady only, both}; no sync: state 2 throughout
  B   8  narrow stage: symbols_per_bit = 1 and extend_correlation_symbols = 3, so the channel re-designs both filters after its first
         period (3 ms updates, narrow bandwidths and spacings, states 3 / 4); DLL {1, 2, 3} x PLL {2, 3}, plus DLL 3 / PLL 3 and
         DLL 1 / PLL 2 with the steady-state FLL
  C   2  track_pilot with the data replica, extend_correlation_symbols 1 (state 4) and 2 (states 3 / 4): four-quadrant PLL
  D   1  an all-zero input, DLL 3 / PLL 3 / FLL both, max_lock_fail = 0: P.x == 0 and pe + pl == 0, a NaN C/N0 and lock test, which
         must not count as a lock failure (one counted failure would end the channel)
A plain engine's channels share the pilot mode, so A, B and D are slots of one engine and C of a second one, per tap count.

The pull-in transitory (pull_in_time_s = 0) ends when sample_counter - acq_samplestamp_samples reaches one second of samples:
sample_counter starts 36.5 periods short of that, so pure-FLL, FLL-aided and PLL-only periods all occur in the FLL channels.
acq_delay_samples is what an acquisition at acq_samplestamp_samples would have measured for the code phase the signal has.

Doppler 2.5 kHz: the block length's fraction starts 8e-3 samples below a whole sample and moves away from it by as much every period
(see closed_loop_matrix_cases.py), 0.76 samples over the run, so no block length comes near a whole number."""
import copy

import numpy as np

import closed_loop_matrix_cases as M
import closed_loop_ref as R

FS, N, CN0, FC = M.FS, M.N, M.CN0, M.FC
N_EP = 96
f32 = np.float32

# taps -> (seed, Doppler [Hz], code delay in the buffer [samples])
SIGNALS = {3: (2101, 2500.0, 1234.0), 5: (2105, 2540.0, 2222.0)}
ACQ_STAMP = 1000
SAMPLE_COUNTER = ACQ_STAMP + int(FS) - 36 * N - N // 2  # the transitory ends at the 37th period or the one after
NARROW = {3: dict(pll_bw_narrow_hz=20.0, dll_bw_narrow_hz=1.0, early_late_space_narrow_chips=0.3, very_early_late_space_narrow_chips=0.0),
    5: dict(pll_bw_narrow_hz=20.0, dll_bw_narrow_hz=1.0, early_late_space_narrow_chips=0.1, very_early_late_space_narrow_chips=0.4)}
FLL_MODES = {"off": (0, 0), "pullin": (1, 0), "steady": (0, 1), "both": (1, 1)}


def _base_conf(taps):
    seed, doppler, delay = SIGNALS[taps]
    L, spc = (1023, 1) if taps == 3 else (2046, 2)
    diff = SAMPLE_COUNTER - ACQ_STAMP
    return dict(fs_in=FS, signal_carrier_freq_hz=FC, code_chip_rate_hz=L * 1000.0 / spc, code_period_s=0.001, carrier_lock_th=0.85,
        code_length_chips=L // spc, code_samples_per_chip=spc, vector_length=N, pull_in_time_s=0, veml=int(taps == 5), pll_filter_order=3,
        dll_filter_order=2, enable_fll_pull_in=0, enable_fll_steady_state=0, cn0_samples=10, cn0_min=25, max_lock_fail=50, pll_bw_hz=35.0,
        dll_bw_hz=2.0, fll_bw_hz=10.0, early_late_space_chips=(0.15 if taps == 5 else 0.5), very_early_late_space_chips=(0.6 if taps == 5 else 0.0),
        acq_samplestamp_samples=ACQ_STAMP, sample_counter=SAMPLE_COUNTER, acq_delay_samples=float((diff + int(delay)) % N), acq_doppler_hz=doppler + 3.0,
        high_dyn_smoother_length=0)


def channels(taps):
    """The case table of a tap count: dicts of name, group, engine ("plain" / "pilot"), buffer ("data" / "pilot" / "zero"), conf, sync."""
    out = []

    def add(name, group, engine, buffer, sync, **conf):
        out.append(dict(name=name, group=group, engine=engine, buffer=buffer, sync=sync, conf=dict(_base_conf(taps), **conf)))

    for dll in (1, 2, 3):
        for pll in (2, 3):
            for fll, (pull, steady) in FLL_MODES.items():
                add("A-dll%d-pll%d-fll_%s" % (dll, pll, fll), "A", "plain", "data", None, dll_filter_order=dll, pll_filter_order=pll,
                    enable_fll_pull_in=pull, enable_fll_steady_state=steady)
    narrow = dict(extend_correlation_symbols=3, track_pilot=False, symbols_per_bit=1, **NARROW[taps])
    for dll in (1, 2, 3):
        for pll in (2, 3):
            add("B-dll%d-pll%d" % (dll, pll), "B", "plain", "data", narrow, dll_filter_order=dll, pll_filter_order=pll)
    add("B-dll3-pll3-fll_steady", "B", "plain", "data", narrow, dll_filter_order=3, pll_filter_order=3, enable_fll_steady_state=1)
    add("B-dll1-pll2-fll_steady", "B", "plain", "data", narrow, dll_filter_order=1, pll_filter_order=2, enable_fll_steady_state=1)
    add("C-ext1", "C", "pilot", "pilot", dict(extend_correlation_symbols=1, track_pilot=True, symbols_per_bit=1), dll_filter_order=3, pll_filter_order=2)
    add("C-ext2", "C", "pilot", "pilot", dict(extend_correlation_symbols=2, track_pilot=True, symbols_per_bit=1, **NARROW[taps]), dll_filter_order=1,
        pll_filter_order=3)
    add("D-zero", "D", "plain", "zero", None, dll_filter_order=3, pll_filter_order=3, enable_fll_pull_in=1, enable_fll_steady_state=1, max_lock_fail=0)
    return out


ENGINES = [(taps, engine) for taps in (3, 5) for engine in ("plain", "pilot")]


def engine_channels(taps, engine):
    return [c for c in channels(taps) if c["engine"] == engine]


_built = {}


def signal(taps):
    """dict(code, data_code, data: the signal, pilot: the same with the data component, zero), complex64 streams of one length."""
    if taps not in _built:
        from test_loop_sync_gpu import _stream
        seed, doppler, delay = SIGNALS[taps]
        L = 1023 if taps == 3 else 2046
        rng = np.random.Generator(np.random.PCG64(seed))
        code = (rng.integers(0, 2, L) * 2 - 1).astype(np.float32)
        data_code = (rng.integers(0, 2, L) * 2 - 1).astype(np.float32)
        symbols = rng.integers(0, 2, 97) * 2.0 - 1.0
        n = N * (N_EP + 3)
        data = _stream([(code, [1.0], 1.0)], FS, n, doppler, delay, CN0, seed + 50, L * 1000.0)
        pilot = _stream([(code, [1.0], 1.0), (data_code, symbols, 1.0)], FS, n, doppler, delay, CN0, seed + 50, L * 1000.0)
        _built[taps] = dict(code=code, data_code=data_code, data=data, pilot=pilot, zero=np.zeros(n, np.complex64))
    return _built[taps]


_refs = {}


def reference(oracle, taps, name):
    """The CPU restatement's records of a channel; computed once, never modified."""
    if (taps, name) not in _refs:
        c = next(c for c in channels(taps) if c["name"] == name)
        s = signal(taps)
        _refs[taps, name] = R.run(oracle, s[c["buffer"]], s["code"], c["conf"], N_EP, sync=c["sync"], data_code=s["data_code"] if c["engine"] == "pilot" else None)
    return _refs[taps, name]


def records_of(ref, taps):
    """The restatement's records in the device's record layout (what the device would write were it the restatement)."""
    import gnsscorr
    rec = np.zeros(len(ref), gnsscorr.LOOP_RECORD_DTYPE)
    for k, r in enumerate(ref):
        g = rec[k]
        g["corr"][0:2 * taps:2], g["corr"][1:2 * taps:2] = r["corr"].real, r["corr"].imag
        g["accu"][0::2], g["accu"][1::2] = r["accu"].real, r["accu"].imag
        g["prompt_data"] = (r["prompt_data"].real, r["prompt_data"].imag)
        g["carrier_doppler_hz"] = g["carr_error_filt_hz"] = r["doppler"]
        g["code_freq_chips"], g["carr_phase_error_hz"], g["code_error_chips"], g["code_error_filt_chips"] = r["code_freq"], r["perr"], r["cerr"], r["cfilt"]
        g["cn0_db_hz"], g["carrier_lock_test"] = r["cn0"], r["lock_test"]
        g["sample_counter"], g["acc_carrier_phase_rad"], g["rem_code_phase_samples"] = r["sample_counter"], r["acc_phase"], r["rem_code_samples"]
        g["state"], g["valid"], g["current_prn_length_samples"], g["extend_count"], g["integrating"] = r["state"], r["valid"], r["cur"], r["ext_count"], r["integrating"]
    return rec


# ---- the replay: the pinned restatement fed with the device's own records, one period at a time ----
LIBM = ("atanf", "atan2f", "atan2", "hypotf", "log10")
BRANCHES = ("pure_fll", "fll_aided_pll", "pll_only", "state2", "state3", "state4", "integrating", "redesign", "cn0_1ms", "cn0_2ms", "cn0_3ms")


def _bits(v):
    return np.asarray(v).view(np.uint32 if np.asarray(v).dtype == np.float32 else np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype, (a.dtype, b.dtype)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _inside(lo, v, hi):
    lo, hi = min(lo, hi), max(lo, hi)
    return bool(lo <= v <= hi) or (np.isnan(v) and np.isnan(lo) and np.isnan(hi)) or _same(v, lo) or _same(v, hi)


def replay(rec, case, taps, gate):
    """Holds every record of one channel to the restatement evaluated on the device's own recorded inputs.  IEEE-only stages (+ - * /
    sqrt) bit for bit; a stage behind a libm call must be reproduced with that call's result moved by at most `gate` ulp.  Returns
    (largest shift needed per libm function, periods per branch).  Raises AssertionError naming the period and the field."""
    conf, y = case["conf"], dict(extend_correlation_symbols=1, track_pilot=False, symbols_per_bit=2)
    if case["sync"]:
        y.update(case["sync"])
    ext, pilot, veml = max(1, y["extend_correlation_symbols"]), bool(y["track_pilot"]), taps == 5
    fs, period = conf["fs_in"], conf["code_period_s"]
    dist = dict.fromkeys(LIBM, 0)
    seen = dict.fromkeys(BRANCHES, 0)

    def need(ok, k, what, *info):
        if not ok:
            raise AssertionError("%s, period %d: %s %r" % (case["name"], k, what, info))

    def smallest(k, what, fn, hit):
        """The smallest g <= gate for which hit(g) holds."""
        for g in range(gate + 1):
            if hit(g):
                dist[fn] = max(dist[fn], g)
                return
        need(False, k, "%s: not within %d ulp of %s" % (what, gate, fn))

    dll = R.LoopFilter(period, conf["dll_bw_hz"], conf["dll_filter_order"])
    pll0 = R.Pll(conf["fll_bw_hz"], conf["pll_bw_hz"], conf["pll_filter_order"])
    pll0.initialize(conf["acq_doppler_hz"])
    plls = [pll0]  # the carrier filter states the device may be in: more than one only where two FLL inputs gave one output
    offset, acc_phase = R.pull_in(conf)
    sample_counter = conf["sample_counter"] + offset
    state, cloop, pulling, corr_time, ext_count = 2, True, True, period, 0
    doppler, code_freq, rem_code, rem_carr = conf["acq_doppler_hz"], conf["code_chip_rate_hz"], 0.0, f32(0)
    accu = np.zeros(5, np.complex64)
    p_old = np.complex64(0)
    prompts, cn0, lock_test, fail = [], f32(0), f32(1), 0
    held = dict(carr_phase_error_hz=f32(0), carr_error_filt_hz=f32(0), code_error_chips=f32(0), code_error_filt_chips=f32(0), carrier_doppler_hz=f32(doppler),
        code_freq_chips=f32(code_freq))

    for k in range(len(rec)):
        g = rec[k]
        need(int(g["valid"]) == 1, k, "valid")
        if pulling and conf["pull_in_time_s"] < (sample_counter - conf["acq_samplestamp_samples"]) // int(fs):
            pulling = False
        corr = (g["corr"][0:2 * taps:2] + 1j * g["corr"][1:2 * taps:2]).astype(np.complex64)
        dev_accu = (g["accu"][0::2] + 1j * g["accu"][1::2]).astype(np.complex64)
        seen["state%d" % state] += 1
        update = state != 3
        if state == 2:
            accu[:] = 0
            accu[(0 if veml else 1):(0 if veml else 1) + taps] = corr
            coh = period
        else:
            for t in range(taps):  # no secondary code in this matrix: every period adds
                i = t if veml else t + 1
                accu[i] = np.complex64(complex(f32(accu[i].real + corr[t].real), f32(accu[i].imag + corr[t].imag)))
            cloop = not pilot
            coh = period * ext
        need(_same(dev_accu.view(np.float32), accu.view(np.float32)), k, "accu", dev_accu, accu)

        def nco():
            nonlocal acc_phase, rem_code, rem_carr, sample_counter
            u = R.nco_update(code_freq, doppler, rem_code, rem_carr, acc_phase, conf)
            need(int(g["current_prn_length_samples"]) == u["cur"], k, "current_prn_length_samples", int(g["current_prn_length_samples"]), u["cur"])
            need(_same(np.float64(g["rem_code_phase_samples"]), np.float64(u["rem_code_samples"])), k, "rem_code_phase_samples")
            need(_same(np.float64(g["acc_carrier_phase_rad"]), np.float64(u["acc_phase"])), k, "acc_carrier_phase_rad", float(g["acc_carrier_phase_rad"]), u["acc_phase"])
            acc_phase, rem_code, rem_carr = u["acc_phase"], u["rem_code_samples"], u["rem_carr"]
            sample_counter += u["cur"]
            need(int(g["sample_counter"]) == sample_counter, k, "sample_counter")

        if not update:
            nco()
            seen["integrating"] += 1
            need(int(g["integrating"]) == 1, k, "integrating")
            ext_count += 1
            if ext_count == ext - 1:
                ext_count, state = 0, 4
        else:
            need(int(g["integrating"]) == 0, k, "integrating")
            # cn0_and_tracking_lock_status
            locked = True
            if len(prompts) < conf["cn0_samples"]:
                prompts.append(np.complex64(accu[2]))
            else:
                pb, prompts = np.array(prompts, np.complex64), []
                lock_test = R.carrier_lock_detector(pb)
                need(_same(f32(g["carrier_lock_test"]), lock_test), k, "carrier_lock_test", float(g["carrier_lock_test"]), float(lock_test))
                dev = f32(g["cn0_db_hz"])
                smallest(k, "cn0_db_hz %r" % float(dev), "log10",
                    lambda m: _inside(R.cn0_svn_estimator(pb, coh, move=(-m, m)), dev, R.cn0_svn_estimator(pb, coh, move=(m, -m))))
                cn0 = dev
                seen["cn0_%dms" % int(round(coh * 1000))] += 1
                fail, locked = R.lock_fail_update(fail, float(lock_test), float(cn0), pulling, conf)
            need(_same(f32(g["cn0_db_hz"]), cn0) and _same(f32(g["carrier_lock_test"]), lock_test), k, "C/N0 and lock test between estimates")
            need(locked, k, "the lock-fail counter ends the channel here; the matrix has no such case")
            # run_dll_pll: the carrier side
            P = accu[2]
            dev_perr = f32(g["carr_phase_error_hz"])
            if cloop:
                smallest(k, "carr_phase_error_hz %r" % float(dev_perr), "atanf",
                    lambda m: any(_same(f32(R.pll_cloop_two_quadrant_atan(P, move=s) / R.PI_2), dev_perr) for s in (-m, m)))
            else:
                smallest(k, "carr_phase_error_hz %r" % float(dev_perr), "atan2f",
                    lambda m: any(_same(f32(R.pll_four_quadrant_atan(P, move=s) / R.PI_2), dev_perr) for s in (-m, m)))
            dev_filt = f32(g["carr_error_filt_hz"])
            need(_same(dev_filt, f32(g["carrier_doppler_hz"])), k, "carrier_doppler_hz is carr_error_filt_hz")
            use_fll = (pulling and conf["enable_fll_pull_in"]) or conf["enable_fll_steady_state"]
            pure = bool(pulling and conf["enable_fll_pull_in"])
            seen["pure_fll" if pure else "fll_aided_pll" if use_fll else "pll_only"] += 1
            pll_in = f32(0) if pure else dev_perr

            def carrier(fll_inputs):
                """The filter states that give the device's output for one of the inputs; the inputs' index of the first that does."""
                keep, first = [], None
                for f in plls:
                    for j, v in enumerate(fll_inputs):
                        c = copy.copy(f)
                        if _same(c.get_carrier_error(v, pll_in, f32(corr_time)), dev_filt) and not any((c.w, c.x) == (o.w, o.x) for o in keep):
                            keep.append(c)
                            first = j if first is None else min(first, j)
                return keep, first

            if use_fll:
                moves = sorted(range(-gate, gate + 1), key=abs)
                keep, first = carrier([f32(R.fll_four_quadrant_atan(p_old, P, 0.0, corr_time, move=m) / R.PI_2) for m in moves])
                need(keep, k, "carr_error_filt_hz %r: not within %d ulp of atan2 in the FLL discriminator" % (float(dev_filt), gate))
                dist["atan2"] = max(dist["atan2"], abs(moves[first]))
                p_old = np.complex64(P)
            else:
                keep, _ = carrier([f32(0)])
                need(keep, k, "carr_error_filt_hz", float(dev_filt), float(copy.copy(plls[0]).get_carrier_error(f32(0), pll_in, f32(corr_time))))
            plls = keep
            doppler = float(dev_filt)
            # the code side
            dev_cerr = f32(g["code_error_chips"])
            if veml:
                want = f32(R.dll_nc_vemlp_normalized(accu[0], accu[1], accu[3], accu[4]))
                need(_same(dev_cerr, want), k, "code_error_chips (VEMLP)", float(dev_cerr), float(want))
            else:
                smallest(k, "code_error_chips %r" % float(dev_cerr), "hypotf",
                    lambda m: _inside(f32(R.dll_nc_e_minus_l_normalized(accu[1], accu[3], move=(-m, m))), dev_cerr,
                        f32(R.dll_nc_e_minus_l_normalized(accu[1], accu[3], move=(m, -m)))))
            want = dll.apply(dev_cerr)
            dev_cfilt = f32(g["code_error_filt_chips"])
            need(_same(dev_cfilt, want), k, "code_error_filt_chips", float(dev_cfilt), float(want), state)
            dll.y[dll.i] = dev_cfilt  # (equal: the history is the device's own either way)
            code_freq = R.code_nco(doppler, float(dev_cfilt), conf)
            need(_same(f32(g["code_freq_chips"]), f32(code_freq)), k, "code_freq_chips")
            nco()
            for name in held:
                held[name] = f32(g[name])
            # general_work's transitions
            if state == 2:
                if case["sync"] and y["symbols_per_bit"] == 1:
                    accu[:] = 0
                    if ext > 1:
                        corr_time = float(f32(f32(ext) * f32(period)))
                        state = 3
                        dll.design(corr_time, y["dll_bw_narrow_hz"])
                        for f in plls:
                            f.set_params(conf["fll_bw_hz"], y["pll_bw_narrow_hz"], conf["pll_filter_order"])
                        seen["redesign"] += 1
                    else:
                        state = 4
            else:
                accu[:] = 0
                state = 3 if ext > 1 else 4
        for name, v in held.items():  # an integrating period leaves the loop's outputs as they were
            need(_same(f32(g[name]), v), k, name + " held", float(g[name]), float(v))
        need(int(g["state"]) == state and int(g["extend_count"]) == ext_count, k, "state, extend_count", int(g["state"]), state, int(g["extend_count"]), ext_count)
    return dist, seen
