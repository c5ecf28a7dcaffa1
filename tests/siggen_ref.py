"""The signal generator's model (include/gnsscorr.h, "Signal generator") restated in numpy: Python integers / uint64 for every phase
and for Philox, float64 for everything after.

    x[t] = sum_s amplitude_s b_s(t) w_s(t) + sigma (g_re(t) + j g_im(t))

A satellite is a dict: code_step_q, code_phase0_q, carr_step_q, carr_phase0_q (Python integers, Q0.64), amplitude, table_len and comps,
a list of dicts with table (float [table_len]), gain, axis, secondary (+-1 array or None), periods_per_symbol, period_offset."""
import math

import numpy as np

M64 = (1 << 64) - 1
_U32 = np.uint64(0xFFFFFFFF)


def q64(x):
    """floor(x 2^64) of a float x in [0, 1): exact."""
    assert 0.0 <= x < 1.0
    return int(math.ldexp(x, 64))


def frac(q):
    f = q - math.floor(q)
    return 0.0 if f >= 1.0 else f


def plan_words(doppler_hz, carrier_phase0_turns, code_phase0_periods, code_periods_per_sample, fs_hz):
    """(code_step_q, code_phase0_q, carr_step_q, carr_phase0_q): the C ABI's one rule, floor(x 2^64)."""
    return (q64(code_periods_per_sample), q64(code_phase0_periods), q64(frac(doppler_hz / fs_hz)), q64(frac(carrier_phase0_turns)))


def from_satellite(sat, fs_hz):
    """The dict of a gnsscorr.SiggenSatellite, its words computed here."""
    c = sat.c
    w = plan_words(c.doppler_hz, c.carrier_phase0_turns, c.code_phase0_periods, c.code_periods_per_sample, fs_hz)
    comps = []
    for i in range(int(c.n_components)):
        k = c.comp[i]
        comps.append(dict(table=np.asarray(sat.tables[i], np.float32), gain=float(k.gain), axis=int(k.axis),
            secondary=None if sat.secondaries[i] is None else np.asarray(sat.secondaries[i], np.int8),
            periods_per_symbol=int(k.periods_per_symbol), period_offset=int(k.period_offset)))
    return dict(code_step_q=w[0], code_phase0_q=w[1], carr_step_q=w[2], carr_phase0_q=w[3], amplitude=float(np.float32(c.amplitude)),
        table_len=int(c.table_len), comps=comps)


def amplitude_bound(sats):
    """A = sum_s |amplitude_s| sum_c |gain_c| max |table_c|: what a noise-free sample cannot exceed."""
    return float(sum(abs(s["amplitude"]) * sum(abs(c["gain"]) * float(np.max(np.abs(c["table"]))) for c in s["comps"]) for s in sats))


def mulhi(a, b):
    """Upper 64 bits of the 128-bit products of uint64 arrays (or scalars), from 32-bit halves."""
    a = np.asarray(a, np.uint64)
    b = np.asarray(b, np.uint64)
    s32 = np.uint64(32)
    a0, a1, b0, b1 = a & _U32, a >> s32, b & _U32, b >> s32
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> s32) + (p01 & _U32) + (p10 & _U32)
    return p11 + (p01 >> s32) + (p10 >> s32) + (mid >> s32)


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter: uint32 [..., 4]; key: (k0, k1).  Returns uint32 [..., 4]."""
    c = np.asarray(counter, np.uint64)
    c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    m0, m1, s32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & _U32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & _U32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _key(seed):
    return (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def _times(t_first, n):
    """Scenario samples t_first .. t_first + n - 1 mod 2^64 as uint64."""
    return np.uint64(t_first & M64) + np.arange(n, dtype=np.uint64)


def code_phase(sat, t):
    """(k, f, e) of the samples t (uint64 array): U = phase0 + t step = k 2^64 + f, e = (f table_len) >> 64."""
    step, phase0 = np.uint64(sat["code_step_q"]), np.uint64(sat["code_phase0_q"])
    with np.errstate(over="ignore"):
        lo = t * step
        f = lo + phase0
        k = mulhi(t, step) + (f < lo).astype(np.uint64)
    e = mulhi(f, np.uint64(sat["table_len"])).astype(np.int64)
    return k, f, e


def symbols(seed, j, s, c):
    """Data symbols j (uint64 array) of component c of satellite s (index from 0): +-1 float64."""
    uj, inv = np.unique(j, return_inverse=True)
    ctr = np.stack([uj & _U32, uj >> np.uint64(32), np.full(uj.shape, 2 * s + c, np.uint64), np.ones(uj.shape, np.uint64)], axis=-1)
    x0 = philox4x32_10(ctr, _key(seed))[..., 0]
    return np.where(x0 & 1, -1.0, 1.0)[inv]


def noise(seed, t_first, n):
    """g_re + j g_im of samples t_first .. t_first + n - 1, complex128: Box-Muller on the two 24-bit uniforms."""
    t = _times(t_first, n)
    z = np.zeros(n, np.uint64)
    x = philox4x32_10(np.stack([t & _U32, t >> np.uint64(32), z, z], axis=-1), _key(seed))
    u1 = ((x[:, 0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (x[:, 1] >> 8).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.exp(2j * np.pi * u2)


def satellite(sat, s, seed, t_first, n):
    """amplitude_s b_s w_s of samples t_first .. t_first + n - 1, complex128."""
    t = _times(t_first, n)
    k, _, e = code_phase(sat, t)
    b = np.zeros(n, np.complex128)
    for c, comp in enumerate(sat["comps"]):
        v = np.asarray(comp["table"], np.float64)[e] * comp["gain"]
        with np.errstate(over="ignore"):
            kk = k + np.uint64(comp["period_offset"])
        if comp["periods_per_symbol"]:
            v = v * symbols(seed, kk // np.uint64(comp["periods_per_symbol"]), s, c)
        if comp["secondary"] is not None and len(comp["secondary"]):
            v = v * np.asarray(comp["secondary"], np.float64)[(kk % np.uint64(len(comp["secondary"]))).astype(np.int64)]
        b += 1j * v if comp["axis"] else v
    with np.errstate(over="ignore"):
        theta = np.uint64(sat["carr_phase0_q"]) + t * np.uint64(sat["carr_step_q"])
    # all 64 bits of theta: split so that float64 loses nothing that matters (2^-53 turns)
    turns = (theta >> np.uint64(32)).astype(np.float64) * 2.0 ** -32 + (theta & _U32).astype(np.float64) * 2.0 ** -64
    return sat["amplitude"] * b * np.exp(2j * np.pi * turns)


def generate(sats, sigma, seed, t_first, n):
    """Samples t_first .. t_first + n - 1 of the scene, complex128."""
    x = np.zeros(n, np.complex128)
    for s, sat in enumerate(sats):
        x += satellite(sat, s, seed, t_first, n)
    if sigma != 0.0:
        x += float(np.float32(sigma)) * noise(seed, t_first, n)
    return x
