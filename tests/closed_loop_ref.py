"""Python restatement of the dll_pll_veml_tracking loop (states 1-4) on top of the CPU oracle correlator:
the checker for the device closed-loop engine (test infrastructure).

Follows dll_pll_veml_tracking.cc: pull-in :1568-1600, do_correlation_step :886-911, cn0_and_tracking_lock_status
:839-878, run_dll_pll :914-973, update_tracking_vars :998-1070, acquire_secondary :800-836, save_correlation_results
:1072-1125 and the states 2 / 3 / 4 of general_work :1601-1896, with the loop filters of
tracking_loop_filter.cc:104-245 (no last integrator) and tracking_FLL_PLL_filter.cc:55-133, the discriminators of
tracking_discriminators.cc:49-128 and the lock detectors of lock_detectors.cc:68-111, float32 where the reference uses float.

The filters, the discriminators and the lock detectors are module-level so that run() and the replay of the device's own records
(tests/test_loop_maths_gpu.py) use the same code; tests/test_loop_filter_pin.py holds them to the reference's files compiled in
oracle/_ref.  `move` arguments shift a libm result by that many ulp of its own type (np.nextafter): the replay's gate on the
device's libm."""
import numpy as np

PI_2 = 6.283185307179586
f32 = np.float32


def moved(v, n):
    """The float32 / float64 scalar v, n ulp up (n > 0) or down."""
    to = type(v)(np.inf if n > 0 else -np.inf)
    for _ in range(abs(int(n))):
        v = np.nextafter(v, to)
    return v


# ---- discriminators (tracking_discriminators.cc): complex64 in, double out, radians / chips ----
def fll_four_quadrant_atan(p1, p2, t1, t2, move=0):
    """dot and cross are float expressions assigned to doubles; the atan2 is double (:49-55)."""
    a, b, c, d = f32(p1.real), f32(p1.imag), f32(p2.real), f32(p2.imag)
    with np.errstate(all="ignore"):
        dot = np.float64(f32(f32(a * c) + f32(b * d)))
        cross = np.float64(f32(f32(a * d) - f32(c * b)))
        return float(moved(np.arctan2(cross, dot), move)) / (t2 - t1)


def pll_four_quadrant_atan(p, move=0):
    """float atan2 (:65-68): the double atan2 rounded to float.  (numpy's own float32 arctan2 is 2 ulp from glibc's, which is
    correctly rounded, on about 1 input in 200.)"""
    return float(moved(f32(np.arctan2(np.float64(f32(p.imag)), np.float64(f32(p.real)))), move))


def pll_cloop_two_quadrant_atan(p, move=0):
    """float division and float atan (:78-85): the double atan rounded to float, as above."""
    if f32(p.real) != 0:
        with np.errstate(all="ignore"):
            return float(moved(f32(np.arctan(np.float64(f32(f32(p.imag) / f32(p.real))))), move))
    return 0.0


def dll_nc_e_minus_l_normalized(e, l, move=(0, 0)):
    """std::abs(gr_complex) is a float hypot (:96-106): np.hypot on float32, which is libm's (np.abs of a complex64 is numpy's own
    and 1 ulp away on half the inputs); move: ulp shifts of the two moduli."""
    with np.errstate(all="ignore"):
        pe = float(moved(np.hypot(f32(e.real), f32(e.imag)), move[0]))
        pl = float(moved(np.hypot(f32(l.real), f32(l.imag)), move[1]))
        if pe + pl == 0.0:
            return 0.0
        return float(np.float64(0.5 * (pe - pl)) / np.float64(pe + pl))


def _norm(v):
    re, im = f32(v.real), f32(v.imag)
    return f32(f32(re * re) + f32(im * im))


def dll_nc_vemlp_normalized(ve, e, l, vl):
    """std::sqrt(std::norm(VE) + std::norm(E)) on gr_complex: a float sum and a float root, widened afterwards (:118-128)."""
    with np.errstate(all="ignore"):
        pe = float(np.sqrt(f32(_norm(ve) + _norm(e))))
        pl = float(np.sqrt(f32(_norm(vl) + _norm(l))))
        if pe + pl == 0.0:
            return 0.0
        return float(np.float64(pe - pl) / np.float64(pe + pl))


# ---- lock detectors (lock_detectors.cc) ----
def cn0_svn_estimator(prompts, coh_integration_time_s, move=(0, 0)):
    """Sequential double sums (:68-85); move: ulp shifts of log10(SNR) and log10(T).  Returns a float32."""
    psig = ptot = 0.0
    for v in prompts:
        re, im = float(v.real), float(v.imag)
        psig += abs(re)
        ptot += im * im + re * re
    psig /= float(len(prompts))
    psig = psig * psig
    ptot /= float(len(prompts))
    with np.errstate(all="ignore"):
        snr = np.float64(psig) / np.float64(ptot - psig)
        return f32(10.0 * moved(np.log10(snr), move[0]) - 10.0 * moved(np.log10(np.float64(coh_integration_time_s)), move[1]))


def carrier_lock_detector(prompts):
    """Sequential float sums (:97-111).  Returns a float32."""
    si, sq = f32(0), f32(0)
    for v in prompts:
        si = f32(si + f32(v.real))
        sq = f32(sq + f32(v.imag))
    with np.errstate(all="ignore"):
        return f32(f32(f32(si * si) - f32(sq * sq)) / f32(f32(si * si) + f32(sq * sq)))


def lock_fail_update(fail, lock_test, cn0, pull_in, conf):
    """The loss-of-lock counter of cn0_and_tracking_lock_status (:855-877): (new counter, still locked).  NaN compares false on both
    sides of the `or`: an estimate that is not a number counts as a pass."""
    if not pull_in:
        if lock_test < conf["carrier_lock_th"] or cn0 < conf["cn0_min"]:
            fail += 1
        elif fail > 0:
            fail -= 1
    if fail > conf["max_lock_fail"]:
        return 0, False
    return fail, True


def code_nco(doppler, cfilt, conf):
    """d_code_freq_chips (:972)."""
    return (1.0 + doppler / conf["signal_carrier_freq_hz"]) * conf["code_chip_rate_hz"] - cfilt


def nco_update(code_freq, doppler, rem_code_samples, rem_carr, acc_phase, conf, carr_rate=None):
    """update_tracking_vars (:998-1070) without the rate smoothers' histories: carr_rate(step, block length) gives the carrier
    phase rate of the high-dynamics mode (None: 0).  Returns a dict of the new values."""
    fs = conf["fs_in"]
    T_prn = (1.0 / code_freq) * conf["code_length_chips"] * fs
    K = T_prn + rem_code_samples
    cur = int(np.floor(K))
    step = PI_2 * doppler / fs
    rate = carr_rate(step, float(cur)) if carr_rate else 0.0
    adv = step * cur + 0.5 * rate * float(cur) * float(cur)
    rem_carr = f32(f32(rem_carr) + f32(adv))
    rem_carr = f32(np.fmod(rem_carr, f32(PI_2)))
    rem = K - cur
    return dict(cur=cur, step=step, carr_rate=rate, rem_carr=rem_carr, acc_phase=acc_phase - adv, code_step=code_freq / fs, rem_code_samples=rem,
        rem_code_chips=code_freq * rem / fs)


def pull_in(conf):
    """The sample skip of state 1 (:1568-1600): (samples skipped, accumulated carrier phase after it)."""
    fs = conf["fs_in"]
    delta = float(conf["sample_counter"] - conf["acq_samplestamp_samples"]) - conf["acq_delay_samples"]
    T_prn = (1.0 / conf["code_chip_rate_hz"]) * conf["code_length_chips"] * fs
    offset = int(np.round(T_prn - np.fmod(delta, T_prn)))
    return offset, 0.0 - (PI_2 * conf["acq_doppler_hz"] / fs) * offset


class LoopFilter:
    def __init__(self, T, bw, order=2):
        self.order = order
        self.design(T, bw)
        self.x = [f32(0)] * 4
        self.y = [f32(0)] * 4
        self.i = 3

    def design(self, T, bw):
        """update_coefficients: new coefficients, history untouched (set_noise_bandwidth / set_update_interval)."""
        order = self.order
        T, bw = f32(T), float(f32(bw))  # both are floats in the reference; the arithmetic below widens where C widens
        zeta = f32(1.0 / np.sqrt(2.0))
        if order == 1:
            self.b, self.a = [f32(f32(bw * 4.0))], []
        elif order == 3:
            wn = f32(bw / 0.7845)
            a3, b3 = f32(1.1), f32(2.4)
            g1, g2, g3 = f32(wn * wn * wn), f32(a3 * wn * wn), f32(b3 * wn)
            self.b = [f32(float(g3) + float(T) / 2.0 * (float(g2) + float(T) / 2.0 * float(g1))), f32(float(f32(f32(g1 * T) * T)) / 2.0 - 2.0 * float(g3)),
                f32(float(g3) + float(T) / 2.0 * (-float(g2) + float(T) / 2.0 * float(g1)))]
            self.a = [f32(2.0), f32(-1.0)]
        else:
            wn = f32(float(f32(bw)) * (8.0 * float(zeta)) / (4.0 * float(zeta) * float(zeta) + 1.0))
            g1 = f32(wn * wn)
            g2 = f32(float(wn) * 2.0 * float(zeta))
            self.b = [f32(float(f32(g1 * T)) / 2.0 + float(g2)), f32(float(f32(g1 * T)) / 2.0 - float(g2))]
            self.a = [f32(1.0)]

    def apply(self, v):
        r = f32(0)
        for k, a in enumerate(self.a):
            r = f32(r + f32(a * self.y[(self.i + k) % 4]))
        self.i = (self.i - 1) % 4
        self.x[self.i] = f32(v)
        for k, b in enumerate(self.b):
            r = f32(r + f32(b * self.x[(self.i + k) % 4]))
        self.y[self.i] = r
        return r


class Pll:
    def __init__(self, fll_bw, pll_bw, order=3):
        self.set_params(fll_bw, pll_bw, order)
        self.w = f32(0)
        self.x = f32(0)

    def set_params(self, fll_bw, pll_bw, order):
        self.order = order
        self.a2 = f32(1.414)
        if order == 3:
            self.b3, self.a3 = f32(2.4), f32(1.1)
            self.w0p = f32(pll_bw / 0.7845)
            self.w0p2 = f32(self.w0p * self.w0p)
            self.w0p3 = f32(self.w0p2 * self.w0p)
            self.w0f = f32(fll_bw / 0.53)
            self.w0f2 = f32(self.w0f * self.w0f)
        else:
            self.w0p = f32(pll_bw / 0.53)
            self.w0p2 = f32(self.w0p * self.w0p)
            self.w0f = f32(fll_bw / 0.25)

    def initialize(self, doppler):
        if self.order == 3:
            self.x, self.w = f32(2.0 * float(f32(doppler))), f32(0)
        else:
            self.w, self.x = f32(doppler), f32(0)

    def get_carrier_error(self, fll, pll, T):
        fll, pll, T = f32(fll), f32(pll), f32(T)
        if self.order == 3:
            self.w = f32(self.w + f32(T * f32(f32(self.w0p3 * pll) + f32(self.w0f2 * fll))))
            self.x = f32(float(self.x) + float(T) * (0.5 * float(self.w) + float(f32(f32(self.a2 * self.w0f) * fll)) + float(f32(f32(self.a3 * self.w0p2) * pll))))
            return f32(0.5 * float(self.x) + float(f32(f32(self.b3 * self.w0p) * pll)))
        w_new = f32(f32(self.w + f32(f32(pll * self.w0p2) * T)) + f32(f32(fll * self.w0f) * T))
        err = f32(0.5 * float(f32(w_new + self.w)) + float(f32(f32(self.a2 * self.w0p) * pll)))
        self.w = w_new
        return err


def run(oracle, x, code, conf, n_epochs, sync=None, data_code=None):
    """conf: dict with the gc_loop_conf fields; sync: dict with the gc_loop_sync_conf fields (secondary_code a '0'/'1'
    string, preamble_symbols a list of +1/-1) or None (never leaves state 2).  Returns a list of per-epoch dicts."""
    fs = conf["fs_in"]
    spc = conf["code_samples_per_chip"]
    veml = bool(conf["veml"])
    y = dict(extend_correlation_symbols=1, track_pilot=False, symbols_per_bit=2, secondary_code="", preamble_symbols=[],
        bit_sync_min_time_s=10.0, pll_bw_narrow_hz=0.0, dll_bw_narrow_hz=0.0, early_late_space_narrow_chips=0.0, very_early_late_space_narrow_chips=0.0)
    if sync:
        y.update(sync)
    ext = max(1, y["extend_correlation_symbols"])
    sec, pre = y["secondary_code"], list(y["preamble_symbols"])
    pilot = bool(y["track_pilot"])

    def taps_for(el, vel):
        if veml:
            return np.array([-vel * spc, -el * spc, 0.0, el * spc, vel * spc], np.float32)
        return np.array([-el * spc, 0.0, el * spc], np.float32)

    shifts = taps_for(f32(conf["early_late_space_chips"]), f32(conf["very_early_late_space_chips"]))
    N = conf["vector_length"]
    dll = LoopFilter(conf["code_period_s"], conf["dll_bw_hz"], conf["dll_filter_order"])
    pll = Pll(conf["fll_bw_hz"], conf["pll_bw_hz"], conf["pll_filter_order"])
    pll.initialize(conf["acq_doppler_hz"])
    doppler = conf["acq_doppler_hz"]
    step = PI_2 * doppler / fs
    rem_carr = f32(0.0)
    rem_code_samples = 0.0
    rem_code_chips = 0.0
    sample_counter = conf["sample_counter"]
    acq_stamp = conf["acq_samplestamp_samples"]
    # pull-in
    code_freq = conf["code_chip_rate_hz"]
    code_step = code_freq / fs
    offset, acc_phase = pull_in(conf)
    sample_counter += offset
    pos = offset
    st = dict(state=2, cloop=True, corr_time=conf["code_period_s"], cur=N, prompt_buffer=[], cn0=0.0, lock_test=1.0, fail=0,
        perr=0.0, cerr=0.0, cfilt=0.0, hist=[], current_symbol=0, ext_count=0, pull_in=True, P_old=np.complex64(0))
    accu = np.zeros(5, np.complex64)  # VE E P L VL
    out = []
    # high dynamics (:1016-1033, :1047-1064)
    sl = int(conf.get("high_dyn_smoother_length", 0))
    hd = dict(carr=[], code=[], carr_rate=0.0, code_rate=0.0)

    def smoothed(hist, value, samples, current):
        hist.append((value, samples))
        del hist[:-2 * sl]
        if len(hist) < 2 * sl:
            return current
        cp1 = sum(h[0] for h in hist[:sl]) / sl
        newer = [hist[2 * sl - k - 1] for k in range(sl)]
        cp2 = sum(h[0] for h in newer) / sl
        return (cp2 - cp1) / sum(h[1] for h in newer)

    def lock_status(coh_time):
        if len(st["prompt_buffer"]) < conf["cn0_samples"]:
            st["prompt_buffer"].append(np.complex64(accu[2]))
            return True
        pb = np.array(st["prompt_buffer"], np.complex64)
        st["prompt_buffer"] = []
        st["cn0"] = float(cn0_svn_estimator(pb, coh_time))
        st["lock_test"] = float(carrier_lock_detector(pb))
        st["fail"], locked = lock_fail_update(st["fail"], st["lock_test"], st["cn0"], st["pull_in"], conf)
        return locked

    def run_dll_pll():
        nonlocal doppler, code_freq
        P = accu[2]
        if st["cloop"]:
            st["perr"] = pll_cloop_two_quadrant_atan(P) / PI_2
        else:
            st["perr"] = pll_four_quadrant_atan(P) / PI_2
        if (st["pull_in"] and conf["enable_fll_pull_in"]) or conf["enable_fll_steady_state"]:
            ferr = fll_four_quadrant_atan(st["P_old"], P, 0.0, st["corr_time"]) / PI_2
            st["P_old"] = np.complex64(P)
            if st["pull_in"] and conf["enable_fll_pull_in"]:
                doppler = float(pll.get_carrier_error(ferr, 0.0, st["corr_time"]))
            else:
                doppler = float(pll.get_carrier_error(ferr, st["perr"], st["corr_time"]))
        else:
            doppler = float(pll.get_carrier_error(0.0, st["perr"], st["corr_time"]))
        if veml:
            st["cerr"] = dll_nc_vemlp_normalized(accu[0], accu[1], accu[3], accu[4])
        else:
            st["cerr"] = dll_nc_e_minus_l_normalized(accu[1], accu[3])
        st["cfilt"] = float(dll.apply(st["cerr"]))
        code_freq = code_nco(doppler, st["cfilt"], conf)

    def update_tracking_vars():
        nonlocal step, rem_carr, acc_phase, code_step, rem_code_samples, rem_code_chips
        u = nco_update(code_freq, doppler, rem_code_samples, rem_carr, acc_phase, conf,
            carr_rate=(lambda s_, n_: smoothed(hd["carr"], s_, n_, hd["carr_rate"])) if sl else None)
        cur = st["cur"] = u["cur"]
        step, rem_carr, acc_phase, code_step = u["step"], u["rem_carr"], u["acc_phase"], u["code_step"]
        if sl:
            hd["carr_rate"] = u["carr_rate"]
            hd["code_rate"] = smoothed(hd["code"], code_step, float(cur), hd["code_rate"])
        rem_code_samples, rem_code_chips = u["rem_code_samples"], u["rem_code_chips"]

    def save_correlation_results(taps):
        sign = 1.0
        if sec:
            if sec[st["current_symbol"]] != "0":
                sign = -1.0
            st["current_symbol"] = (st["current_symbol"] + 1) % len(sec)
        else:
            st["current_symbol"] = (st["current_symbol"] + 1) % y["symbols_per_bit"] if y["symbols_per_bit"] > 0 else 0
        for t in range(5):
            if not veml and t in (0, 4):
                continue
            v = taps[t if veml else t - 1]
            accu[t] = np.complex64(accu[t] + v) if sign > 0 else np.complex64(accu[t] - v)
        st["cloop"] = not pilot

    for _ in range(n_epochs):
        if st["state"] == 0 or pos + N > len(x):
            break
        if st["pull_in"] and conf["pull_in_time_s"] < (sample_counter - acq_stamp) // int(fs):
            st["pull_in"] = False
        args = (f32(rem_carr), f32(step), f32(f32(rem_code_chips) * f32(spc)), f32(f32(code_step) * f32(spc)), N)
        if sl:
            args = args + (f32(hd["carr_rate"]), f32(f32(hd["code_rate"]) * f32(spc)), True)
        pos_in, shifts_in = pos, shifts.copy()
        corr = oracle.multicorrelator(x[pos:], code, shifts, *args)
        pdata = oracle.multicorrelator(x[pos:], data_code, shifts[len(shifts) // 2:len(shifts) // 2 + 1], *args)[0] if pilot else corr[len(shifts) // 2]
        P = corr[len(shifts) // 2]
        valid, integrating, log_accu, log_count = 0, 0, None, 0
        state_in = st["state"]
        if st["state"] == 2:
            accu[:] = 0
            for t in range(len(corr)):
                accu[t if veml else t + 1] = corr[t]
            if not lock_status(conf["code_period_s"]):
                st["state"] = 0
                log_accu = accu.copy()
                hd.update(carr=[], code=[], carr_rate=0.0, code_rate=0.0)
            else:
                run_dll_pll()
                update_tracking_vars()
                valid, log_accu, log_count = 1, accu.copy(), st["ext_count"]
                nxt = False
                if sec:
                    st["hist"].append(P.real < 0)
                    st["hist"] = st["hist"][-len(sec):]
                    if len(st["hist"]) == len(sec):
                        cv = sum((1 if (neg == (c == "0")) else -1) for neg, c in zip(st["hist"], sec))
                        nxt = abs(cv) == len(sec)
                elif y["symbols_per_bit"] > 1:
                    t_trk = f32(float(f32(sample_counter - acq_stamp)) / fs)
                    if t_trk > y["bit_sync_min_time_s"] and pre:
                        st["hist"].append(P.real < 0)
                        st["hist"] = st["hist"][-len(pre):]
                        if len(st["hist"]) == len(pre):
                            cv = sum((-p if neg else p) for neg, p in zip(st["hist"], pre))
                            nxt = cv == len(pre)
                else:
                    nxt = True
                if nxt:
                    accu[:] = 0
                    st["hist"] = []
                    st["current_symbol"] = 0
                    if ext > 1:
                        st["ext_count"] = 0
                        st["corr_time"] = float(f32(f32(ext) * f32(conf["code_period_s"])))
                        st["state"] = 3
                        dll.design(st["corr_time"], y["dll_bw_narrow_hz"])
                        pll.set_params(conf["fll_bw_hz"], y["pll_bw_narrow_hz"], conf["pll_filter_order"])
                        shifts = taps_for(f32(y["early_late_space_narrow_chips"]), f32(y["very_early_late_space_narrow_chips"]))
                    else:
                        st["state"] = 4
        elif st["state"] == 3:
            update_tracking_vars()
            save_correlation_results(corr)
            st["ext_count"] += 1
            if st["ext_count"] == ext - 1:
                st["ext_count"] = 0
                st["state"] = 4
            valid, integrating, log_accu, log_count = 1, 1, accu.copy(), st["ext_count"]
        else:
            save_correlation_results(corr)
            if not lock_status(conf["code_period_s"] * ext):
                st["state"] = 0
                log_accu = accu.copy()
            else:
                run_dll_pll()
                update_tracking_vars()
                valid, log_accu, log_count = 1, accu.copy(), st["ext_count"]
                accu[:] = 0
                if ext > 1:
                    st["state"] = 3
        cur = st["cur"]
        sample_counter += cur
        pos += cur
        out.append(dict(corr=corr, doppler=doppler, code_freq=code_freq, cur=cur, sample_counter=sample_counter, cn0=st["cn0"], lock_test=st["lock_test"],
            perr=st["perr"], cerr=st["cerr"], cfilt=st["cfilt"], pull_in=st["pull_in"], rem_code_samples=rem_code_samples, acc_phase=acc_phase, state=st["state"], state_in=state_in, valid=valid,
            integrating=integrating, accu=log_accu, ext_count=log_count, prompt_data=pdata, args=args, pos=pos_in, shifts=shifts_in))
    return out
