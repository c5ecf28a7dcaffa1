"""Python restatement of the reference's GLONASS L1 / L2 C/A tracking block on top of the CPU oracle correlator: the checker
for the device GLONASS loop (test infrastructure), plus the fixed-seed scenarios its CPU and GPU tests share.

Follows glonass_l1_ca_dll_pll_tracking_cc.cc (the L2 block differs in the carrier constants only): start_tracking :160-243,
the pull-in alignment :570-590 and the per-period loop of general_work :592-777, with Tracking_2nd_DLL_filter
(tracking_2nd_DLL_filter.cc:40-76) and Tracking_2nd_PLL_filter (tracking_2nd_PLL_filter.cc:40-88), float32 where the reference
uses float and float64 where it uses double.  (np.float32 op python-float stays float32 in NumPy 2, so every double-precision
sub-expression converts its operands with float() first.)"""
import numpy as np

PI_2 = 6.283185307179586
CODE_RATE_HZ = 0.511e6
CODE_LENGTH_CHIPS = 511.0
BANDS = {1: (1.602e9, 0.5625e6), 2: (1.246e9, 0.4375e6)}  # GLONASS_L1_L2_CA.h:84-97: carrier, channel spacing
f32 = np.float32


class SecondOrderFilter:
    """Tracking_2nd_DLL_filter (k = 1) / Tracking_2nd_PLL_filter (k = 0.25): float state, the integrator term in double."""

    def __init__(self, k, pdi=0.001):
        self.k, self.pdi, self.zeta = f32(k), f32(pdi), f32(0.7)
        self.tau1 = self.tau2 = f32(0)
        self.initialize()

    def set_bw(self, bw):
        z = float(self.zeta)
        wn = f32(float(f32(bw)) * 8.0 * z / (4.0 * z * z + 1.0))
        self.tau1 = f32(self.k / f32(wn * wn))
        self.tau2 = f32(2.0 * z / float(wn))

    def set_pdi(self, pdi):
        self.pdi = f32(pdi)

    def initialize(self):
        self.old_nco, self.old_error = f32(0), f32(0)

    def step(self, discriminator):
        d = f32(discriminator)
        proportional = f32(self.old_nco + f32(f32(self.tau2 / self.tau1) * f32(d - self.old_error)))
        integral = float(f32(d + self.old_error)) * (float(self.pdi) / (2.0 * float(self.tau1)))
        nco = f32(float(proportional) + integral)
        self.old_nco, self.old_error = nco, d
        return nco


def dll_filter(bw, pdi=0.001):
    f = SecondOrderFilter(1.0, pdi)
    f.set_bw(bw)
    return f


def pll_filter(bw, pdi=0.001):
    f = SecondOrderFilter(0.25, pdi)
    f.set_bw(bw)
    return f


def discriminators(E, P, L):
    """pll_cloop_two_quadrant_atan / 2 pi and dll_nc_e_minus_l_normalized in double on complex taps."""
    E, P, L = complex(E), complex(P), complex(L)
    perr = (np.arctan(P.imag / P.real) if P.real != 0 else 0.0) / PI_2
    e, l = abs(E), abs(L)
    return float(perr), (0.0 if e + l == 0 else 0.5 * (e - l) / (e + l))


def start(conf):
    """start_tracking and the pull-in alignment (which emits no record): the loop's state before its first period, as a dict."""
    fs = float(int(conf["fs_in"]))
    el = f32(conf["early_late_space_chips"])
    shifts = np.array([-el, 0.0, el], np.float32)
    # ---- start_tracking ----
    acq_phase, acq_doppler = float(conf["acq_delay_samples"]), float(conf["acq_doppler_hz"])
    acq_stamp, sample_counter = int(conf["acq_samplestamp_samples"]), int(conf["sample_counter"])
    diff_seconds = float(f32(f32(sample_counter - acq_stamp) / f32(int(conf["fs_in"]))))
    offset_hz = float(conf["channel_offset_hz"])
    freq_ch = float(conf["band_carrier_freq_hz"]) + offset_hz
    code_freq = ((freq_ch + acq_doppler) / freq_ch) * CODE_RATE_HZ
    code_step = code_freq / fs
    T_mod_s = (1 / code_freq) * CODE_LENGTH_CHIPS
    T_mod = T_mod_s * fs
    cur = int(np.round(T_mod))
    T_true_s = CODE_LENGTH_CHIPS / CODE_RATE_HZ
    T_true = T_true_s * fs
    n_diff = diff_seconds / T_true_s
    corrected = float(np.fmod(acq_phase + (T_true_s - T_mod_s) * n_diff * fs, T_true))
    if corrected < 0:
        corrected = T_mod + corrected
    acq_phase = corrected
    carrier_freq = acq_doppler + offset_hz
    doppler = acq_doppler
    step = PI_2 * carrier_freq / fs
    doppler_step = PI_2 * doppler / fs
    dll, pll = dll_filter(conf["dll_bw_hz"]), pll_filter(conf["pll_bw_hz"])
    rem_code_samples = rem_code_chips = rem_carr = acc_phase = 0.0
    # ---- pull-in: no record ----
    delay = (sample_counter - acq_stamp) & 0xffffffff  # int32_t acq_to_trk_delay_samples
    delay = delay - 2 ** 32 if delay >= 2 ** 31 else delay
    shift_correction = float(f32(f32(cur) - np.fmod(f32(delay), f32(cur))))
    samples_offset = int(np.round(acq_phase + shift_correction))
    sample_counter += samples_offset
    pos = samples_offset
    acc_phase -= doppler_step * samples_offset
    pull_in = dict(samples_offset=samples_offset, sample_counter=sample_counter, acc_phase=acc_phase, doppler=doppler)
    return dict(locals())


def run(oracle, x, code, conf, n_epochs):
    """conf: dict with the gc_glonass_loop_conf fields.  Returns one dict per period that ran; the run stops where the device
    loop stops writing valid records (input exhausted, loss of lock, a block length outside 1..2 * vector_length)."""
    v = start(conf)
    fs, shifts, freq_ch, dll, pll, pull_in = (v[k] for k in ("fs", "shifts", "freq_ch", "dll", "pll", "pull_in"))
    code_freq, code_step, cur, carrier_freq, doppler, step, doppler_step = (v[k] for k in ("code_freq", "code_step", "cur", "carrier_freq", "doppler", "step", "doppler_step"))
    rem_code_samples, rem_code_chips, rem_carr, acc_phase, sample_counter, pos = (v[k] for k in ("rem_code_samples", "rem_code_chips", "rem_carr", "acc_phase", "sample_counter", "pos"))
    prompt_buffer, cn0, lock_test, fail = [], 0.0, 1.0, 0
    out = []
    state = 2
    for _ in range(n_epochs):
        if state != 2 or pos + cur > len(x):
            break
        args = (f32(rem_carr), f32(step), f32(rem_code_chips), f32(code_step), cur)
        corr = oracle.multicorrelator(x[pos:], code, shifts, *args)
        E, P, L = corr
        pos_in, n_in = pos, cur
        perr = (float(np.arctan(f32(P.imag / P.real))) if P.real != 0 else 0.0) / PI_2
        pfilt = float(pll.step(perr))
        carrier_freq += pfilt
        doppler += pfilt
        code_freq = CODE_RATE_HZ + ((doppler * CODE_RATE_HZ) / freq_ch)
        pe, pl = float(f32(abs(E))), float(f32(abs(L)))
        cerr = 0.0 if pe + pl == 0 else 0.5 * (pe - pl) / (pe + pl)
        cfilt = float(dll.step(cerr))
        T_chip = 1.0 / code_freq
        T_prn_s = T_chip * CODE_LENGTH_CHIPS
        cfilt_secs = T_prn_s * cfilt * T_chip
        T_prn = T_prn_s * fs
        K = T_prn + rem_code_samples + cfilt_secs * fs
        cur = int(np.round(K))
        doppler_step = PI_2 * doppler / fs
        step = PI_2 * carrier_freq / fs
        rem_carr = float(np.fmod(rem_carr + step * cur, PI_2))
        acc_phase -= doppler_step * cur
        code_step = code_freq / fs
        rem_code_samples = K - cur
        rem_code_chips = code_freq * (rem_code_samples / fs)
        if len(prompt_buffer) < conf["cn0_samples"]:
            prompt_buffer.append(np.complex64(P))
        else:
            pb = np.array(prompt_buffer, np.complex64)
            prompt_buffer = []
            psig = np.mean(np.abs(pb.real.astype(np.float64))) ** 2
            ptot = np.mean(pb.imag.astype(np.float64) ** 2 + pb.real.astype(np.float64) ** 2)
            with np.errstate(all="ignore"):
                cn0 = float(f32(10 * np.log10(psig / (ptot - psig)) - 10 * np.log10(0.001)))
            si, sq = f32(0), f32(0)
            for v in pb:
                si = f32(si + v.real)
                sq = f32(sq + v.imag)
            lock_test = float(f32(f32(f32(si * si) - f32(sq * sq)) / f32(f32(si * si) + f32(sq * sq))))
            if lock_test < conf["carrier_lock_th"] or cn0 < conf["cn0_min"]:
                fail += 1
            elif fail > 0:
                fail -= 1
            if fail > conf["max_lock_fail"]:
                fail = 0
                state = 0
        consumed = cur
        if cur < 1 or cur > 2 * conf["vector_length"]:
            state, consumed = 0, 0
        sample_counter += consumed
        pos += consumed
        out.append(dict(corr=corr, doppler=doppler, carrier_freq=carrier_freq, code_freq=code_freq, cur=cur, sample_counter=sample_counter, cn0=cn0,
            lock_test=lock_test, perr=perr, pfilt=pfilt, cerr=cerr, cfilt=cfilt, rem_code_samples=rem_code_samples, acc_phase=acc_phase, state=state,
            valid=1, K_blk=K, args=args, pos=pos_in, n=n_in, pull_in=pull_in))
    return out


# ---- scenarios shared by tests/test_glonass_loop_ref.py (CPU) and tests/test_glonass_loop_gpu.py ----
N_PERIODS = 60
QUANT = 12.0  # samples are integers in -127..127 (unit-variance noise times QUANT): the I16 / I8 engines see what the F32 engine sees


def make_stream(code, fs, n, band, k, doppler, delay, cn0, seed, signal=True, phase_at=(0, 0.7)):
    """One GLONASS satellite on frequency channel k at complex baseband around the band's centre, in unit-variance noise: the
    carrier sits at k * spacing + doppler, the code runs at 511 kchip/s scaled by the Doppler against the slot's own carrier and
    its period starts `delay` samples into the stream; phase_at = (sample, radians) fixes the carrier phase.  Integer-valued complex64."""
    carrier, spacing = BANDS[band]
    rng = np.random.Generator(np.random.PCG64(seed))
    i = np.arange(n)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)
    if signal:
        rate = CODE_RATE_HZ * (1 + doppler / (carrier + spacing * k)) / fs
        chip = np.floor((511 - delay * CODE_RATE_HZ / fs) + i * rate).astype(np.int64) % 511
        amp = np.sqrt(10 ** (cn0 / 10) / fs)
        x = x + amp * code[chip] * np.exp(1j * (PI_2 * (((spacing * k + doppler) * (i - phase_at[0]) / fs) % 1.0) + phase_at[1]))
    q = np.clip(np.round(x * QUANT), -127, 127)
    return (q.real + 1j * q.imag).astype(np.complex64)


def scenario_conf(sc, max_lock_fail=50, cn0_samples=10):
    carrier, spacing = BANDS[sc["band"]]
    return dict(fs_in=sc["fs"], band_carrier_freq_hz=carrier, channel_offset_hz=spacing * sc["k"], carrier_lock_th=0.85,
        acq_delay_samples=sc["delay"] + sc.get("delay_error", 0.0), acq_doppler_hz=sc["doppler"] + sc["doppler_error"],
        acq_samplestamp_samples=sc.get("acq_stamp", 0), sample_counter=sc.get("sample_counter", 0), vector_length=int(round(sc["fs"] / 1000)),
        cn0_samples=cn0_samples, cn0_min=25, max_lock_fail=max_lock_fail, pll_bw_hz=sc["pll_bw"], dll_bw_hz=sc["dll_bw"], early_late_space_chips=0.5)


def scenario_stream(code, sc):
    """The stream the channel's buffer holds: its sample 0 is stream sample `sample_counter` of the scenario."""
    fs = sc["fs"]
    n = int(round(fs / 1000)) * (N_PERIODS + 3)
    ahead = sc.get("sample_counter", 0) - sc.get("acq_stamp", 0)
    # the code phase `delay` was measured at the acquisition stamp: `ahead` samples later the period starts here
    period = fs / 1000.0 / (1 + sc["doppler"] / (BANDS[sc["band"]][0] + BANDS[sc["band"]][1] * sc["k"]))
    delay_now = (sc["delay"] - ahead) % period
    # The second-order loop of this block is lightly damped: a carrier phase error at the hand-over rings for tens of periods.
    # The scenarios hand over with a small one (0.05 rad at the first tracked sample), so that 60 periods end in steady state.
    first = start(scenario_conf(sc))["pos"]
    return make_stream(code, fs, n, sc["band"], sc["k"], sc["doppler"], delay_now, sc["cn0"], sc["seed"], sc.get("signal", True), (first, 0.05))


SCENARIOS = {
    "2048k_L1_km1": dict(fs=2048000, band=1, k=-1, doppler=1530.0, doppler_error=-0.6, delay=733.4, cn0=76.0, seed=11, pll_bw=35.0, dll_bw=2.0),
    "2048k_L1_kp1": dict(fs=2048000, band=1, k=1, doppler=-2210.0, doppler_error=0.5, delay=1501.7, cn0=76.0, seed=12, pll_bw=35.0, dll_bw=2.0),
    "6625k_L1_km5": dict(fs=6625000, band=1, k=-5, doppler=3120.0, doppler_error=0.4, delay=4410.3, cn0=70.0, seed=13, pll_bw=15.0, dll_bw=2.0),
    "6625k_L1_kp4_ahead": dict(fs=6625000, band=1, k=4, doppler=-975.0, doppler_error=-0.5, delay=2222.6, cn0=70.0, seed=14, pll_bw=15.0, dll_bw=2.0,
        acq_stamp=6625 * 2, sample_counter=6625 * 2 + 3 * 6625 + 1234),
    "6625k_L2_kp3": dict(fs=6625000, band=2, k=3, doppler=450.0, doppler_error=0.7, delay=127.9, cn0=70.0, seed=15, pll_bw=15.0, dll_bw=2.0),
}
NOISE_ONLY = dict(fs=2048000, band=1, k=1, doppler=0.0, doppler_error=0.0, delay=300.0, cn0=0.0, seed=21, pll_bw=20.0, dll_bw=2.0, signal=False)

# Two satellites of one band in one stream (the ring test): both start at stream sample 0; the stream is the sum of their
# integer-valued streams (within +-254: the F32 engine only).
RING_PAIR = {
    "A": dict(SCENARIOS["6625k_L1_km5"]),
    "B": dict(SCENARIOS["6625k_L1_kp4_ahead"], acq_stamp=0, sample_counter=0, seed=16),
}


def ring_pair_stream(code):
    return (scenario_stream(code, RING_PAIR["A"]) + scenario_stream(code, RING_PAIR["B"])).astype(np.complex64)
