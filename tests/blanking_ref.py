"""CPU restatement of the conditioner's pulse blanking (include/gnsscorr.h, gc_conditioner_set_pulse_blanking) in float64: the
state machine of the reference's pulse_blanking_cc.cc, statement for statement, on segment energies from the plain cast.  Test
infrastructure only.  A restatement, not a pin: the reference block needs GNU Radio and is not compiled here.

    state: n = 0, last_filtered = false, noise = 0
    for every whole segment s (raw samples [sL, (s + 1)L)):
      if n < segments_est and not last_filtered:  noise = (n * noise + E[s] / (2L)) / (n + 1);  pass
      elif E[s] / noise > threshold:              blank;  last_filtered = true
      else:                                       pass;   last_filtered = false;  if n > segments_reset: n = 0
      n = n + 1
"""
import numpy as np

import conditioner_ref


def margin(L, segments_est):
    """Relative room between a float32 energy + float32 running mean and float64: one rounding per product and per add of the
    sum (L of them, and a few), one per estimation step."""
    return (L + segments_est + 16) * 2.0 ** -23


def energies(raw, L):
    x = conditioner_ref.to_complex(raw)
    n_seg = len(x) // L
    p = x.real ** 2 + x.imag ** 2
    return p[:n_seg * L].reshape(n_seg, L).sum(axis=1)


def blank(raw, L, threshold, segments_est, segments_reset):
    """Returns dict(flags [n_seg] bool, ratio [n_seg] = E / noise / threshold (nan where the segment was used for the estimate),
    n, last_filtered, noise, decided, blanked, resets)."""
    E = energies(raw, L)
    flags = np.zeros(len(E), bool)
    ratio = np.full(len(E), np.nan)
    n, last, noise, resets = 0, False, 0.0, 0
    thr = float(threshold)
    for s, e in enumerate(E):
        if n < segments_est and not last:
            noise = (n * noise + e / (2.0 * L)) / (n + 1.0)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                r = np.float64(e) / np.float64(noise)
            ratio[s] = r / thr
            if r > thr:
                flags[s] = True
                last = True
            else:
                last = False
                if n > segments_reset:
                    n = 0
                    resets += 1
        n += 1
    return dict(flags=flags, ratio=ratio, n=n, last_filtered=last, noise=noise, decided=len(E), blanked=int(flags.sum()), resets=resets)


def apply(raw, L, flags):
    """The raw stream with the flagged segments zeroed (same dtype and layout); the undecided tail stays."""
    out = np.array(raw, copy=True)
    for s in np.flatnonzero(flags):
        out[s * L:(s + 1) * L] = 0
    return out
