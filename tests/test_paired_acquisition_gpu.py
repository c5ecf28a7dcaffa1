"""GPU tests of the paired acquisition engine (gc_acq_create_paired): every satellite slot holds two replicas A and B, and a grid
cell gets c = max(a, b) or c = a + b of a = |IFFT(X conj FFT(A))|^2 and b = |IFFT(X conj FFT(B))|^2 where a one-replica dwell puts
its |.|^2.  Bars are those of tests/test_acquisition_gpu.py: index and Doppler exact, magnitudes within TOL = 1e-4 of the peak; where
the combined value must equal a one-replica engine's (max(a, a), a + 0, 0 + a) not a bit may differ.  Sizes: DWELL_SIZES of
tests/acq_plan_ref.py, one code period with 4 Doppler bins at every instantiated column size."""
import numpy as np
import pytest

from acq_plan_ref import DWELL_SIZES, plan
from test_acquisition_gpu import TOL, _conf
from test_acquisition_matrix_gpu import _size_conf

pytestmark = pytest.mark.gpu
SIZE_IDS = ["%d-n1_%d" % (n, plan(n)[0]) for n in DWELL_SIZES]
FIELDS = ("indext", "doppler_index", "doppler_hz", "mag", "test_statistics", "second_peak", "second_peak_full_row")


def _fields(r):
    return tuple(getattr(r, f) for f in FIELDS)


def _comb(combine, a, b):
    return np.maximum(a, b) if combine == "max" else a + b


def _sampled(oracle, prn, fs):
    return oracle.gps_l1_ca_code_sampled(prn, fs)


def two_component_signal(oracle, fs, n_samples, seed, s=1, noise=True, prns=(9, 21), doppler=None, whole_samples=False):
    """x = A_s (c_a(tau) + j s c_b(tau)) exp(j(2 pi f n / fs + phi)) + w, w ~ CN(0, 1): both components at 47 dB-Hz with one common
    delay and Doppler (drawn from the seed unless given; whole_samples: the delay is a whole number of samples of the sampled
    replicas, so that both components correlate with their replicas without a sampling loss).  Returns (x, tau0 in chips, Doppler)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ca, cb = (oracle.gps_l1_ca_code(p).astype(np.float64) for p in prns)
    n = np.arange(n_samples, dtype=np.float64)
    amp = np.sqrt(10.0 ** 4.7 / fs)
    fd, tau0, phi = rng.uniform(-900.0, 900.0), rng.uniform(0, 1023), rng.uniform(0, 2 * np.pi)
    if doppler is not None:
        fd = doppler
    if whole_samples:
        period = int(round(fs * 0.001))
        shift = int(round(-tau0 * fs / 1.023e6)) % period
        tau0 = (-shift * 1.023e6 / fs) % 1023
        sa, sb = (np.roll(np.resize(_sampled(oracle, p, fs).real.astype(np.float64), period), shift) for p in prns)
        comp = np.resize(sa, n_samples) + 1j * s * np.resize(sb, n_samples)
    else:
        chip = np.floor(tau0 + n * (1.023e6 / fs)).astype(np.int64) % 1023
        comp = ca[chip] + 1j * s * cb[chip]
    x = amp * comp * np.exp(1j * (2 * np.pi * fd * n / fs + phi))
    if noise:
        x = x + (rng.standard_normal(n_samples) + 1j * rng.standard_normal(n_samples)) * np.sqrt(0.5)
    return x.astype(np.complex64), tau0, fd


# ---- 1. degenerate pairs equal the plain engine bit for bit ----------------------------------------------------------------------

@pytest.mark.parametrize("n", DWELL_SIZES, ids=SIZE_IDS)
def test_degenerate_pairs_equal_the_plain_engine(gctx, oracle, n):
    """max(a, a) = a, a + 0 = a and 0 + a = a exactly (|IFFT(0)|^2 is +0), and the grid accumulates prev + c as the plain engine
    accumulates prev + |.|^2: MAX with (A, A), SUM with (A, 0) and SUM with (0, A) give the plain engine's grids and every result
    field, with dwell() per block (PMAX / PSUM, then the accumulating epilogues twice) and with three dwell_enqueue + one fetch."""
    import gnsscorr
    import torch
    from helpers import synth_stream
    fs, n_dwells = n * 1000, 3
    prns = (9, 21)
    x, _ = synth_stream([oracle.gps_l1_ca_code(prns[0]).astype(np.float32)], fs, n_dwells * n, seed=8000 + n, cn0_db_hz=(47.0, 47.0), doppler_max=900.0)
    c = _size_conf(n, max_dwells=n_dwells)
    codes = [_sampled(oracle, p, fs) for p in prns]
    zero = np.zeros(n, np.complex64)
    engines = [("plain", None, None), ("max (A, A)", "max", lambda a: (a, a)), ("sum (A, 0)", "sum", lambda a: (a, zero)), ("sum (0, A)", "sum", lambda a: (zero, a))]
    d_x = torch.from_numpy(x.view(np.float32)).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    want = None
    for name, combine, pair in engines:
        acq = gnsscorr.PcpsAcquisition(gctx, len(prns), combine=combine, **c)
        assert (acq.fft_size, acq.num_doppler_bins) == (n, 4)
        for s_, code in enumerate(codes):
            if combine is None:
                acq.set_local_code(s_, code)
            else:
                acq.set_local_code_pair(s_, *pair(code))
        got = []
        for d in range(n_dwells):
            got.append([_fields(r) for r in acq.dwell(x[d * n:])])
        got.append([acq.grid(s_) for s_ in range(len(prns))])
        got.append([acq.peek(acq.PEEK_ROW_MAX, s_) for s_ in range(len(prns))])
        acq.reset()
        for d in range(n_dwells):
            acq.dwell_enqueue(d_x.data_ptr() + 8 * n * d, st.cuda_stream)
        got.append([_fields(r) for r in acq.fetch_results(st.cuda_stream)])
        got.append([acq.grid(s_) for s_ in range(len(prns))])
        acq.close()
        # enqueue + fetch equals per-block processing on the same engine
        assert got[n_dwells + 2] == got[n_dwells - 1], name
        for s_ in range(len(prns)):
            assert np.array_equal(got[n_dwells + 3][s_], got[n_dwells][s_]), (name, s_)
        if want is None:
            want = got
            assert want[n_dwells - 1][0][4] > 2.0 * want[n_dwells - 1][1][4]  # PRN 9 present, PRN 21 absent
            continue
        for d in range(n_dwells):
            assert got[d] == want[d], (name, "dwell %d" % d)
        for s_ in range(len(prns)):
            assert np.array_equal(got[n_dwells][s_], want[n_dwells][s_]), (name, s_, "grid")
            assert np.array_equal(got[n_dwells + 1][s_], want[n_dwells + 1][s_]), (name, s_, "row maxima")


# ---- 2. two different replicas against the oracle --------------------------------------------------------------------------------

_REF2 = {}


def _two_replica_reference(oracle, n):
    """Per size, once: the two-dwell signal, and per dwell the one-replica grids gA_d, gB_d and the input power from oracle.pcps."""
    if n not in _REF2:
        fs = n * 1000
        x, tau0, fd = two_component_signal(oracle, fs, 2 * n, seed=9000 + n)
        grids, power = [], []
        for prn in (9, 21):
            p = oracle.pcps(**_size_conf(n))
            p.set_local_code(_sampled(oracle, prn, fs))
            g = []
            for d in range(2):
                p.reset_grid()
                q = p.core(x[d * n:])
                g.append(p.grid())
                if prn == 9:
                    power.append(q.input_power)
            grids.append(g)
        for g in grids:
            for a in g:
                a.setflags(write=False)
        _REF2[n] = (x, tau0, fd, grids[0], grids[1], power)
    return _REF2[n]


@pytest.mark.parametrize("combine", ["max", "sum"])
@pytest.mark.parametrize("n", DWELL_SIZES, ids=SIZE_IDS)
def test_two_replicas_against_the_oracle(gctx, oracle, n, combine):
    import gnsscorr
    fs = n * 1000
    x, tau0, fd, gA, gB, power = _two_replica_reference(oracle, n)
    codes = (_sampled(oracle, 9, fs), _sampled(oracle, 21, fs))
    # two dwells: the grid is comb(gA_0, gB_0) + comb(gA_1, gB_1)
    acq = gnsscorr.PcpsAcquisition(gctx, 1, combine=combine, **_size_conf(n, max_dwells=2))
    acq.set_local_code_pair(0, *codes)
    for d in range(2):
        r = acq.dwell(x[d * n:])[0]
    want = _comb(combine, gA[0], gB[0]) + _comb(combine, gA[1], gB[1])
    grid = acq.grid(0)
    peak = float(want.max())
    print("n %d %s: grid error %.3e of the peak, mag %.9g against %.9g" % (n, combine, np.max(np.abs(grid - want)) / peak, r.mag, peak))
    assert np.max(np.abs(grid - want)) <= TOL * peak
    row, col = np.unravel_index(int(np.argmax(want)), want.shape)  # first maximum, rows in increasing Doppler
    assert (r.doppler_index, r.indext) == (row, col)
    assert r.doppler_hz == -1000 + 500 * row
    assert r.mag == pytest.approx(peak, rel=TOL)
    # the peak is the signal's: both components share one delay and one Doppler
    expect = (-tau0 * fs / 1.023e6) % n
    assert min(abs(col - expect), n - abs(col - expect)) <= n / 1023.0 + 1 and abs(r.doppler_hz - fd) <= 500
    rm = acq.peek(acq.PEEK_ROW_MAX, 0)
    assert np.array_equal(rm[:, 1].astype(np.int64), grid.argmax(axis=1)) and np.array_equal(rm[:, 0], grid.max(axis=1))
    acq.close()
    # one dwell with the CFAR statistic: max / N^4 / input_power
    acq = gnsscorr.PcpsAcquisition(gctx, 1, combine=combine, **_size_conf(n, max_dwells=1))
    acq.set_local_code_pair(0, *codes)
    r = acq.dwell(x)[0]
    one = _comb(combine, gA[0], gB[0])
    stat = float(one.max()) / float(n) ** 4 / power[0]
    print("n %d %s: statistic %.9g against %.9g" % (n, combine, r.test_statistics, stat))
    assert r.test_statistics == pytest.approx(stat, rel=2 * TOL)
    assert (r.doppler_index, r.indext) == np.unravel_index(int(np.argmax(one)), one.shape)
    acq.close()


# ---- 3. sign recovery, noise free ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [1, -1])
def test_sign_recovery_noise_free(gctx, oracle, s):
    """CCCWSR on x = A (c9 + j s c21): the engine's MAX grid on cccwsr_replicas(c9, c21) against the block's own formula
    (pcps_cccwsr_acquisition_cc.cc:316-370) evaluated with the oracle's FFT and its wipe-off rows (the float32 running phase of
    the engine), and the doubled amplitude of the winning hypothesis: its cross terms of two real codes at one delay cancel, so the
    peak is 4 x that of c9 alone but for the plain peak's own cross-correlation, at most (65 / 1023)^2 of it.  The Doppler sits on
    a bin of the grid (-500 Hz): with no residual rotation inside the block that cross-correlation is real, in quadrature to the
    plain peak's main term, and the delay is a whole number of samples: a fractional delay costs each code its own sampling loss
    (it depends on the code's chip transitions), and the bound assumes equal main terms of the two components.  (With the
    fractional delay of the seed the ratio was 4.0145: c21 lost less than c9.)"""
    import gnsscorr
    fs, n = 4_000_000, 4000
    x, tau0, fd = two_component_signal(oracle, fs, n, seed=300 + s, s=s, noise=False, doppler=-500.0, whole_samples=True)
    c = _size_conf(n)
    cd, cp = _sampled(oracle, 9, fs), _sampled(oracle, 21, fs)
    pd = oracle.pcps(**c)
    pd.set_local_code(cd)
    pd.core(x)
    pp = oracle.pcps(**c)
    pp.set_local_code(cp)
    pp.core(x)
    W = pd.wipeoffs()
    Fd = np.conj(oracle.fft(cd.astype(np.complex128)))
    Fp = np.conj(oracle.fft(cp.astype(np.complex128)))
    want = np.zeros((4, n))
    winner = []
    for b in range(4):
        X = oracle.fft(x.astype(np.complex128) * W[b].astype(np.complex128))
        d, p = oracle.fft(X * Fd, inverse=True), oracle.fft(X * Fp, inverse=True)
        plus = (d.real - p.imag) + 1j * (d.imag + p.real)    # :344-346
        minus = (d.real + p.imag) + 1j * (d.imag - p.real)   # :348-350
        want[b] = np.maximum(np.abs(plus) ** 2, np.abs(minus) ** 2)
        winner.append((float(np.max(np.abs(plus) ** 2)), float(np.max(np.abs(minus) ** 2))))
    acq = gnsscorr.PcpsAcquisition(gctx, 1, combine="max", **c)
    acq.set_local_code_pair(0, *gnsscorr.cccwsr_replicas(cd, cp))
    r = acq.dwell(x)[0]
    grid = acq.grid(0)
    peak = float(want.max())
    print("s %+d: grid error %.3e of the peak" % (s, np.max(np.abs(grid - want)) / peak))
    assert np.max(np.abs(grid - want)) <= TOL * peak
    row, col = np.unravel_index(int(np.argmax(want)), want.shape)
    assert (r.doppler_index, r.indext) == (row, col) and r.mag == pytest.approx(peak, rel=TOL)
    # x = c9 + j s c21 correlates with conj(cd - j s' cp): s = +1 is the block's minus hypothesis (replica B), s = -1 its plus
    assert (winner[row][1] > winner[row][0]) == (s == 1)
    acq.close()
    plain = gnsscorr.PcpsAcquisition(gctx, 1, **c)
    plain.set_local_code(0, cd)
    r1 = plain.dwell(x)[0]
    plain.close()
    print("s %+d: paired peak %.9g, plain peak %.9g, ratio %.6f" % (s, r.mag, r1.mag, r.mag / r1.mag))
    assert (r1.doppler_index, r1.indext) == (r.doppler_index, r.indext)
    assert 3.9 <= r.mag / r1.mag <= 4.001
    # SUM on (c9, c21): gA + gB of the one-replica searches
    acq = gnsscorr.PcpsAcquisition(gctx, 1, combine="sum", **c)
    acq.set_local_code_pair(0, cd, cp)
    acq.dwell(x)
    ref = pd.grid() + pp.grid()
    assert np.max(np.abs(acq.grid(0) - ref)) <= TOL * ref.max()
    acq.close()


# ---- 4. ragged batches on the product shape --------------------------------------------------------------------------------------

def test_ragged_satellite_batches_25msps(gctx, oracle, monkeypatch):
    """N = 25000, 20 bins, five satellites, MAX, two dwells: a satellite's pair is 8 MB of the inter-pass buffer, so
    GNSSCORR_ACQ_Q_MB = 1 (read when the engine is created) leaves the one pair the engine always keeps room for -- five batches --
    and 20 MB gives 2 + 2 + 1; the default runs all five at once.  Same additions per cell whatever the batches: not a bit may differ."""
    import gnsscorr
    from helpers import synth_stream
    fs, n = 25_000_000, 25000
    present = (3, 11)
    pairs = ((3, 17), (25, 11), (5, 6), (3, 11), (7, 8))
    x, truth = synth_stream([oracle.gps_l1_ca_code(p).astype(np.float32) for p in present], fs, 2 * n, seed=1404, cn0_db_hz=(46.0, 48.0))
    c = _conf(fs, 1, 1, 25000.0, 5000, 500, max_dwells=2)
    out = []
    for q_mb in (None, "1", "20"):
        if q_mb is None:
            monkeypatch.delenv("GNSSCORR_ACQ_Q_MB", raising=False)
        else:
            monkeypatch.setenv("GNSSCORR_ACQ_Q_MB", q_mb)
        acq = gnsscorr.PcpsAcquisition(gctx, len(pairs), combine="max", **c)
        assert (acq.fft_size, acq.num_doppler_bins) == (n, 20)
        for s_, (pa, pb) in enumerate(pairs):
            acq.set_local_code_pair(s_, _sampled(oracle, pa, fs), _sampled(oracle, pb, fs))
        for d in range(2):
            res = acq.dwell(x[d * n:])
        out.append(([_fields(r) for r in res], [acq.grid(s_) for s_ in range(len(pairs))]))
        acq.close()
    for k in (1, 2):
        assert out[k][0] == out[0][0]
        for s_ in range(len(pairs)):
            assert np.array_equal(out[k][1][s_], out[0][1][s_]), (k, s_)
    # satellite 1, (25 absent, 11 present), against the oracle
    grids = []
    for prn in pairs[1]:
        p = oracle.pcps(**_conf(fs, 1, 1, 25000.0, 5000, 500))
        p.set_local_code(_sampled(oracle, prn, fs))
        g = []
        for d in range(2):
            p.reset_grid()
            p.core(x[d * n:])
            g.append(p.grid())
        grids.append(g)
    want = np.maximum(grids[0][0], grids[1][0]) + np.maximum(grids[0][1], grids[1][1])
    got = out[0][1][1]
    assert np.max(np.abs(got - want)) <= TOL * want.max()
    row, col = np.unravel_index(int(np.argmax(want)), want.shape)
    assert (out[0][0][1][1], out[0][0][1][0]) == (row, col)
    t = truth[1]
    expect = (-t["tau0"] * fs / 1.023e6) % n
    assert min(abs(col - expect), n - abs(col - expect)) <= 25 and abs(-5000 + 500 * row - t["doppler"]) <= 500
    # the slots that hold one present PRN stand out over the absent pairs
    # (slot 3 holds both present PRNs: its second peak may be the other component's, so it is left out of this comparison)
    stats = [f[4] for f in out[0][0]]
    assert min(stats[0], stats[1]) > max(stats[2], stats[4])


# ---- 5. bit transition and step two ----------------------------------------------------------------------------------------------

def test_bit_transition_degenerate_pair_equals_plain(gctx, oracle):
    import gnsscorr
    from helpers import synth_stream
    fs, n = 4_000_000, 4000
    x, _ = synth_stream([oracle.gps_l1_ca_code(9).astype(np.float32)], fs, 2 * n, seed=51, cn0_db_hz=(47.0, 47.0), doppler_max=2000.0)
    c = _conf(fs, 1, 1, 4000.0, 5000, 500, bit_transition_flag=True)
    code = _sampled(oracle, 9, fs)
    code2 = np.concatenate([code, code])
    plain = gnsscorr.PcpsAcquisition(gctx, 1, **c)
    plain.set_local_code(0, code2)
    pair = gnsscorr.PcpsAcquisition(gctx, 1, combine="max", **c)
    assert (pair.fft_size, pair.consumed_samples) == (plain.fft_size, plain.consumed_samples) == (16000, 8000)
    pair.set_local_code_pair(0, code2, code2)
    r0, r1 = plain.dwell(x)[0], pair.dwell(x)[0]
    assert _fields(r1) == _fields(r0) and r1.input_power == r0.input_power
    assert np.array_equal(pair.grid(0), plain.grid(0))
    plain.close()
    pair.close()


def test_step_two_degenerate_pair_equals_plain(gctx, oracle):
    import gnsscorr
    from helpers import synth_stream
    fs, n = 4_000_000, 4000
    x, truth = synth_stream([oracle.gps_l1_ca_code(9).astype(np.float32)], fs, n, seed=52, cn0_db_hz=(48.0, 48.0), doppler_max=2000.0)
    c = _conf(fs, 1, 1, 4000.0, 5000, 250, make_2_steps=True, num_doppler_bins_step2=4, doppler_step2=125.0)
    code = _sampled(oracle, 9, fs)
    plain = gnsscorr.PcpsAcquisition(gctx, 1, **c)
    plain.set_local_code(0, code)
    pair = gnsscorr.PcpsAcquisition(gctx, 1, combine="max", **c)
    pair.set_local_code_pair(0, code, code)
    r0, r1 = plain.dwell(x)[0], pair.dwell(x)[0]
    assert _fields(r1) == _fields(r0) and abs(r0.doppler_hz - truth[0]["doppler"]) <= 250
    for a in (plain, pair):
        a.set_step_two(True, float(r0.acq_doppler_hz))
        assert a.num_doppler_bins == 4
    s0, s1 = plain.dwell(x)[0], pair.dwell(x)[0]
    assert _fields(s1) == _fields(s0) and s1.acq_doppler_hz == s0.acq_doppler_hz
    assert np.array_equal(pair.grid(0), plain.grid(0))
    for a in (plain, pair):
        a.set_step_two(False)
        assert a.num_doppler_bins == 40
        a.reset()
    assert _fields(pair.dwell(x)[0]) == _fields(plain.dwell(x)[0])
    plain.close()
    pair.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_usable(gctx, oracle):
    import ctypes as C
    import gnsscorr
    fs, n = 4_000_000, 4000
    c = _conf(fs, 1, 1, 4000.0, 5000, 500)
    lib = gnsscorr.load_library()
    code = _sampled(oracle, 9, fs)
    x, _, _ = two_component_signal(oracle, fs, n, seed=61)
    # an unknown combiner
    conf = gnsscorr.AcqConf(fs, 1, 1, np.float32(fs) * np.float32(0.001), 4000.0, 4, 5000, 500, 1, 0, 1, 0, 0, 4, 125.0)
    for combine in (0, 3, -1):
        h = C.c_void_p()
        assert lib.gc_acq_create_paired(gctx._h, C.byref(conf), 1, combine, C.byref(h)) == gnsscorr.GC_ERR_INVALID
        assert not h.value
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        gnsscorr.PcpsAcquisition(gctx, 1, combine="product", **c)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    pair = gnsscorr.PcpsAcquisition(gctx, 2, combine="max", **c)
    plain = gnsscorr.PcpsAcquisition(gctx, 1, **c)
    # the one-replica call on a paired engine, the pair call on a plain engine, a slot out of range
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        pair.set_local_code(0, code)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        plain.set_local_code_pair(0, code, code)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        pair.set_local_code_pair(2, code, code)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    # a dwell with a slot unset (the refused set_local_code above has set nothing)
    pair.set_local_code_pair(0, code, np.zeros(n, np.complex64))
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        pair.dwell(x)
    assert ei.value.status == gnsscorr.GC_ERR_STATE
    # PEEK_CODE takes 2 * sat + replica: 0 .. 3 here
    with pytest.raises(gnsscorr.GnsscorrError) as ei:
        pair.peek(pair.PEEK_CODE, 4)
    assert ei.value.status == gnsscorr.GC_ERR_INVALID
    # both engines still work, and agree: slot 0 holds (A, 0) under MAX = A, slot 1 (0, A)
    pair.set_local_code_pair(1, np.zeros(n, np.complex64), code)
    plain.set_local_code(0, code)
    pair.reset()
    r, r0 = pair.dwell(x), plain.dwell(x)[0]
    assert _fields(r[0]) == _fields(r0) and _fields(r[1]) == _fields(r0)
    fc = plain.peek(plain.PEEK_CODE, 0)
    assert np.array_equal(pair.peek(pair.PEEK_CODE, 0), fc) and np.array_equal(pair.peek(pair.PEEK_CODE, 3), fc)
    assert not np.any(pair.peek(pair.PEEK_CODE, 1)) and not np.any(pair.peek(pair.PEEK_CODE, 2))
    pair.close()
    plain.close()
