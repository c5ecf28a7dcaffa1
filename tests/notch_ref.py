"""CPU restatement of the notch filter ring stage (include/gnsscorr.h, gc_ring_notch_*): the reference's Notch_Filter and
Notch_Filter_Lite blocks (notch_cc.cc, notch_lite_cc.cc; behaviour restated, no code taken).  Test infrastructure only.  A
restatement, not a pin: the blocks need GNU Radio and VOLK and are not compiled here.

The decisions -- energies, the DFT noise floor, the running mean, the tests, the lite coefficient -- run in float32, one rounding
per operation in the order the definition states.  The filter runs in float64 given those decisions, sample after sample.

    for every whole segment s:
      if n < segments_est and not active:  noise = (n * noise + F[s]) / (n + 1);  pass
      elif E[s] / noise > threshold:       if not active: active = true; last = 0; (lite: cn = 0);   filter
      else:                                if n > segments_reset: n = 0;   active = false;   pass
      n = n + 1

The module also reports how far the input keeps from a tie: the smallest |E / noise / threshold - 1| over the decided segments and
the smallest |P[k] - cut| over the bins of the estimated ones.  With those margins kept, a flag that differs is a defect and not
a rounding effect.
"""
import numpy as np

F32 = np.float32


def twiddles(L):
    a = -2.0 * np.pi * np.arange(L, dtype=np.float64) / float(L)
    return np.cos(a).astype(F32), np.sin(a).astype(F32)


def bin_powers(seg, L, tw):
    """|X[k]|^2 of one segment, float32: X[k] = sum over i ascending of x[i] tw[(k i) mod L], all bins at once."""
    wr, wi = tw
    xr, xi = seg.real.astype(F32), seg.imag.astype(F32)
    k = np.arange(L)
    ar, ai = np.zeros(L, F32), np.zeros(L, F32)
    for i in range(L):
        j = (k * i) % L
        ar = ar + (xr[i] * wr[j] - xi[i] * wi[j])
        ai = ai + (xr[i] * wi[j] + xi[i] * wr[j])
    return ar * ar + ai * ai


def floor_of(seg, L, tw, noise_floor):
    """(F[s] as float32, smallest |P[k] - cut| in dB)."""
    pw = bin_powers(seg, L, tw)
    db = F32(10.0) * np.log10(pw + F32(1e-20)).astype(F32)
    cut = np.cumsum(db, dtype=F32)[-1] / F32(L) + F32(15.0)
    keep = db <= cut
    kept = F32(np.count_nonzero(keep))
    if noise_floor == "linear":
        f = np.cumsum(pw[keep], dtype=F32)[-1] / kept / F32(2 * L)
    else:
        fl = np.cumsum(db[keep], dtype=F32)[-1] / kept
        f = F32(np.float64(10.0) ** (np.float64(fl) / 10.0) / np.float64(F32(2 * L)))
    return F32(f), float(np.min(np.abs(db.astype(np.float64) - np.float64(cut))))


def _unit(c):
    m = abs(c)
    return c / m if m > 0.0 else 1.0 + 0.0j


def notch(x, L, threshold, p_c_factor=0.9, segments_est=12500, segments_reset=5000000, mode="full", segments_coeff=1, noise_floor="reference"):
    """x: complex64 [n].  Returns a dict: out (complex128 [n_seg * L], the filtered samples in float64; unflagged segments are x),
    flags / starts / estimated (bool [n_seg]), noise (float32), n, active, cn, decided, filtered, last (complex128, the last
    output of the newest filtered segment), ratio [n_seg] (E / noise / threshold, nan where estimated), decision_margin and
    exclusion_margin_db."""
    x = np.ascontiguousarray(x, np.complex64)
    n_seg = len(x) // L
    tw = twiddles(L)
    thr = F32(threshold)
    p = float(F32(p_c_factor))
    out = x[:n_seg * L].astype(np.complex128)
    flags, starts, estimated = np.zeros(n_seg, bool), np.zeros(n_seg, bool), np.zeros(n_seg, bool)
    ratio = np.full(n_seg, np.nan)
    n, active, noise, cn = 0, False, F32(0.0), 0
    last, z0 = 0.0 + 0.0j, 0.0 + 0.0j
    excl = np.inf
    for s in range(n_seg):
        seg = x[s * L:(s + 1) * L]
        if n < segments_est and not active:
            f, m = floor_of(seg, L, tw, noise_floor)
            excl = min(excl, m)
            noise = (F32(n) * noise + f) / F32(n + 1)
            estimated[s] = True
        else:
            re, im = seg.real.astype(F32), seg.imag.astype(F32)
            e = np.cumsum(re * re + im * im, dtype=F32)[-1]
            with np.errstate(divide="ignore", invalid="ignore"):
                r = e / noise
            ratio[s] = float(r) / float(thr)
            if r > thr:
                flags[s] = True
                if not active:
                    active, last, cn = True, 0.0 + 0.0j, 0
                    starts[s] = True
                if mode == "lite":
                    if cn == 0:
                        c1 = np.complex64(seg[1]) * np.conj(seg[0])
                        c2 = np.complex64(seg[L - 1]) * np.conj(seg[L - 2])
                        th = (np.arctan2(F32(c1.imag), F32(c1.real)) + np.arctan2(F32(c2.imag), F32(c2.real))) / F32(2.0)
                        z0 = complex(float(np.cos(F32(th))), float(np.sin(F32(th))))
                    cn = (cn + 1) % segments_coeff
                xm1 = complex(x[s * L - 1]) if s > 0 else 0.0 + 0.0j
                for k in range(L):
                    xk = complex(seg[k])
                    z = _unit(xk * np.conj(xm1)) if mode == "full" else z0
                    last = xk - z * xm1 + p * z * last
                    out[s * L + k] = last
                    xm1 = xk
            else:
                if n > segments_reset:
                    n = 0
                active = False
        n += 1
    decided = ~estimated
    margin = float(np.min(np.abs(ratio[decided] - 1.0))) if decided.any() else np.inf
    return dict(out=out, flags=flags, starts=starts, estimated=estimated, noise=F32(noise), n=n, active=active, cn=cn, decided=n_seg,
        filtered=int(flags.sum()), last=last, ratio=ratio, decision_margin=margin, exclusion_margin_db=float(excl))


def error_bound(p_c_factor, x):
    """8 eps_f32 / (1 - p) max|x|: the recursion amplifies a rounding by 1 / (1 - p)."""
    return 8.0 * 2.0 ** -23 / (1.0 - float(p_c_factor)) * float(np.max(np.abs(x)))


def noise(n, seed, power=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    return ((rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(power / 2.0)).astype(np.complex64)


def tone(n, cycles_per_sample, amplitude, spans, phase=0.3):
    """A tone present in the sample spans [(first, end), ...], zero elsewhere (complex128)."""
    t = np.zeros(n, np.complex128)
    for a, b in spans:
        k = np.arange(a, min(b, n))
        t[k] = amplitude * np.exp(2j * np.pi * cycles_per_sample * k + 1j * phase)
    return t
