"""The open-loop multicorrelator restated in float64 (test infrastructure): what trk_multicorrelator_kernel computes for one record,
as plain maths.

  chips     the reference's float32 index walk, from the compiled oracle (oracle.resampler_indices; with rate= the high-dynamics
            resampler, whose taps >= 1 are tap 0 delayed by whole samples and wrapped at N).  That walk IS the specification: a
            float64 walk would put samples next to a chip edge on the other chip.
  carrier   sample n is multiplied by exp(-j theta(n)), theta(n) = theta0 + n dtheta in float64, where theta0 and dtheta are the
            angles of the record's float32 phasors (phase0 = exp(-j rem_carr), phase_inc = exp(-j phase_step): what the reference's
            rotator multiplies with).  High-dynamics rotator: + drate * float32((n - 1)^2 in uint32) for n >= 1 -- the rule of
            carrier_at (trk_device.hpp) and of oracle/gnss_oracle.c.
  sums      float64 products and sums; complex chips likewise.

No float32 rotator, no modulus drift of the reference's never-renormalised phasor, no summation order.  The 16-bit mode is defined by
its integer rounding and has no restatement: its reference is the compiled oracle.multicorrelator_16sc."""
import numpy as np

MODES = ("plain", "hd_resampler", "hd_full", "complex")


def angles(rec):
    """(theta0, dtheta, drate) in float64 from the float32 phasors of a gc_epoch_params record."""
    return (float(np.arctan2(-np.float64(rec.phase0_im), np.float64(rec.phase0_re))),
        float(np.arctan2(-np.float64(rec.phase_inc_im), np.float64(rec.phase_inc_re))),
        float(np.arctan2(-np.float64(rec.phase_rate_im), np.float64(rec.phase_rate_re))))


def carrier(rec, n_samples, mode):
    """theta(n), n < n_samples."""
    theta0, dtheta, drate = angles(rec)
    n = np.arange(n_samples, dtype=np.float64)
    theta = theta0 + n * dtheta
    if mode == "hd_full" and n_samples > 1:
        m = np.arange(n_samples - 1, dtype=np.uint32)  # (n - 1) for n >= 1
        theta[1:] += drate * (m * m).astype(np.float32).astype(np.float64)
    return theta


def correlate(oracle, window, code, shifts, rec, mode):
    """The n_taps sums of one record.  window: the record's samples (complex, at least rec.n_samples of them, as the device reads
    them: integers cast to float); code: real chips, or complex ones for mode "complex"; rec: gnsscorr.EpochParams."""
    assert mode in MODES, mode
    n_samples = int(rec.n_samples)
    shifts = np.ascontiguousarray(shifts, np.float32)
    if n_samples == 0:
        return np.zeros(len(shifts), np.complex128)
    rate = float(rec.code_phase_rate_step_chips) if mode in ("hd_resampler", "hd_full") else None
    idx = oracle.resampler_indices(float(rec.rem_code_phase_chips), float(rec.code_phase_step_chips), shifts, len(code), n_samples, rate=rate)
    y = np.asarray(window[:n_samples], np.complex128) * np.exp(-1j * carrier(rec, n_samples, mode))
    chips = np.asarray(code, np.complex128 if mode == "complex" else np.float64)
    return np.array([np.sum(y * chips[idx[t]]) for t in range(len(shifts))])
