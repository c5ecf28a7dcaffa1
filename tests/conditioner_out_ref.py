"""Host quantiser of the integer output rings (include/gnsscorr.h, "Integer output rings"): for each component c of a float32 output

    v = c * scale                      one float32 product
    v = MAX if v > MAX;  MIN if v < MIN;  unchanged otherwise
    q = (intN) rintf(v)                round to nearest, ties to even
    a NaN component stores 0

and a component counts as clipped when v > MAX or v < MIN (strict, before the rounding; a NaN is not clipped).  numpy in float32:
np.rint(np.clip(np.float32(y) * np.float32(scale), MIN, MAX))."""
import numpy as np

GC_IQ_I16, GC_IQ_I8 = 1, 2
RANGES = {GC_IQ_I16: (-32768.0, 32767.0, np.int16), GC_IQ_I8: (-128.0, 127.0, np.int8)}


def components(y):
    """complex64 [n] -> float32 [n, 2] (re, im), the same bits."""
    return np.ascontiguousarray(y, np.complex64).view(np.float32).reshape(-1, 2)


def quantise(y, out_format, scale=1.0):
    """(int16 / int8 [n, 2], clipped components) of the complex64 outputs y."""
    lo, hi, dt = RANGES[out_format]
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(over="ignore", invalid="ignore"):
        v = components(y) * np.float32(scale)
    assert v.dtype == np.float32
    clipped = int(np.count_nonzero(v > hi)) + int(np.count_nonzero(v < lo))
    q = np.rint(np.clip(v, lo, hi))
    q = np.where(np.isnan(q), np.float32(0.0), q)
    return q.astype(dt), clipped
