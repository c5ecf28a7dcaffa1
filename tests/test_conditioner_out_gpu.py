"""GPU tests of the integer output rings of the conditioner and the ring decimator (GC_IQ_I16 / GC_IQ_I8 output rings,
gc_stream_accept_quantised_output, gc_*_set_output_scale, gc_*_output_info).  The yardstick is the float32 ring of the same library: a float32 twin runs on the same raw
samples, the host quantises its outputs exactly as include/gnsscorr.h states (tests/conditioner_out_ref.py), and every stored
component and the clipped count must be EQUAL -- no tolerance anywhere."""
import numpy as np
import pytest

import conditioner_out_ref

pytestmark = pytest.mark.gpu
FS_IN = 16e6
# Output ring of the value cases: 1001 samples (odd: the mirror lies an odd number of samples behind the ring, so the dword
# boundaries of a cbyte piece and of its mirror copy differ) with a mirror of 96.  Raw pushes of odd sizes: pieces start at odd
# output numbers, the ring wraps at least twice for D = 3 and 6 times for D = 1, and pieces end inside the mirror part
# (ring positions < 96) after odd counts.
RING_CAP, RING_WIN = 1001, 96
PUSHES = [37, 1, 250, 999, 3, 700, 64, 1, 999, 333, 5, 999, 128, 999, 517]
_twins = {}


def _fmt(name):
    import gnsscorr
    return getattr(gnsscorr, name)


def _out_ring(gctx, cap, win, out_fmt):
    """An output ring; an integer one is opened for a device producer (without that the producers refuse it, as they always did)."""
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=cap, max_window_samples=win, iq_format=out_fmt)
    return ring if out_fmt == gnsscorr.GC_IQ_F32 else ring.accept_quantised_output()


def _taps(T):
    if T == 1:
        return np.ones(1, np.float32)
    k = np.arange(T) - (T - 1) / 2.0
    h = np.sinc(k * 0.25) * np.hamming(T)
    return (h / h.sum() + np.random.Generator(np.random.PCG64(5)).standard_normal(T) * 1e-3).astype(np.float32)


def _raw(n, in_name, seed):
    """Seeded noise plus a tone in the layout of the format: complex64 [n], int16 [n, 2], or int16 [n] (real)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5) + 2.0 * np.exp(2j * np.pi * 1.3e6 * np.arange(n) / FS_IN + 0.3j)
    if in_name == "GC_IQ_F32":
        return (x * 40.0).astype(np.complex64)
    if in_name == "GC_IQ_I16":
        return np.round(np.stack([x.real, x.imag], axis=1) * 40.0).astype(np.int16)
    return np.round(x.real * 40.0).astype(np.int16)  # GC_RAW_REAL_I16


def _run_conditioner(gctx, raw, in_name, out_fmt, D, taps, translate, scale, cap, win, sizes, check=None, blanking=None):
    """Pushes raw in pieces of `sizes`; check(ring, head) after each push.  Returns (outputs resident at the end, first of them,
    output_info, blanking_info or None)."""
    import gnsscorr
    ring = _out_ring(gctx, cap, win, out_fmt)
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, translate, D, taps, _fmt(in_name))
    if scale is not None:
        cond.set_output_scale(scale)
    if blanking:
        cond.set_pulse_blanking(**blanking)
    pos, k = 0, 0
    while pos < len(raw):
        m = min(sizes[k % len(sizes)], len(raw) - pos)
        k += 1
        first, n_out = cond.push(raw[pos:pos + m])
        pos += m
        assert first + n_out == ring.info()[1]
        if check:
            check(ring, cond)
    oldest, head, _ = ring.info()
    y = ring.read(oldest, head - oldest)
    info = cond.output_info()
    binfo = cond.blanking_info() if blanking else None
    cond.close()
    ring.close()
    return y, oldest, info, binfo


def _run_decimator(gctx, raw, in_name, out_fmt, D, taps, scale, cap, win, sizes, check=None):
    import gnsscorr
    src = gnsscorr.IqStream(gctx, capacity_samples=4099, max_window_samples=64, iq_format=_fmt(in_name))
    ring = _out_ring(gctx, cap, win, out_fmt)
    dec = gnsscorr.RingDecimator(gctx, src, D, taps, ring)
    if scale is not None:
        dec.set_output_scale(scale)
    pos, k = 0, 0
    while pos < len(raw):
        m = min(sizes[k % len(sizes)], len(raw) - pos)
        k += 1
        src.push(raw[pos:pos + m])
        pos += m
        first, n_out = dec.update()
        assert first + n_out == ring.info()[1] == (pos + D - 1) // D
        if check:
            check(ring, dec)
    oldest, head, _ = ring.info()
    y = ring.read(oldest, head - oldest)
    info = dec.output_info()
    dec.close()
    ring.close()
    src.close()
    return y, oldest, info, None


def _twin(gctx, producer, in_name, D, T, mix, n):
    """The float32 outputs of one configuration, all of them (a ring that holds the whole run), computed once and shared."""
    import gnsscorr
    key = (producer, in_name, D, T, mix, n)
    if key not in _twins:
        raw = _raw(n, in_name, seed=100 + D)
        taps = _taps(T)
        if producer == "conditioner":
            y, oldest, info, _ = _run_conditioner(gctx, raw, in_name, gnsscorr.GC_IQ_F32, D, taps, 1.25e6 if mix else 0.0, None, 1 << 14, RING_WIN, [n])
        else:
            y, oldest, info, _ = _run_decimator(gctx, raw, in_name, gnsscorr.GC_IQ_F32, D, taps, None, 1 << 14, RING_WIN, [2000])
        assert oldest == 0 and len(y) == (n + D - 1) // D and y.dtype == np.complex64
        assert info == (gnsscorr.GC_IQ_F32, 1.0, 0)  # a float ring reports scale 1 and nothing clipped
        y.setflags(write=False)
        _twins[key] = (raw, taps, y)
    return _twins[key]


def _checker(y_twin, out_fmt, scale, seen):
    """After each push: every resident sample of the ring and the clipped count so far equal the host's."""
    want, _ = conditioner_out_ref.quantise(y_twin, out_fmt, scale)

    def check(ring, producer):
        oldest, head, cap = ring.info()
        assert oldest == max(0, head - cap)
        got = ring.read(oldest, head - oldest)
        assert got.dtype == want.dtype and got.shape == (head - oldest, 2)
        bad = np.nonzero(np.any(got != want[oldest:head], axis=1))[0]
        assert bad.size == 0, "outputs %s ... of [%d, %d) differ: got %s, want %s" % (oldest + bad[:4], oldest, head, got[bad[:4]].tolist(),
            want[oldest + bad[:4]].tolist())
        fmt, s, clipped = producer.output_info()
        assert (fmt, s) == (out_fmt, np.float32(scale))
        assert clipped == conditioner_out_ref.quantise(y_twin[:head], out_fmt, scale)[1]
        seen.append((oldest, head, clipped))
    return check


@pytest.mark.parametrize("producer", ["conditioner", "decimator"])
@pytest.mark.parametrize("out_name", ["GC_IQ_I16", "GC_IQ_I8"])
def test_creation_on_integer_rings(gctx, producer, out_name):
    """The feature exists: before it, both creations returned GC_ERR_INVALID for any ring that is not GC_IQ_F32, and no call opened
    an integer ring for a device producer."""
    import gnsscorr
    out_fmt = _fmt(out_name)
    ring = _out_ring(gctx, 1024, 64, out_fmt)
    if producer == "conditioner":
        p = gnsscorr.Conditioner(gctx, ring, FS_IN, 0.0, 2, _taps(7), gnsscorr.GC_IQ_I16)
        src = None
    else:
        src = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=gnsscorr.GC_IQ_I16)
        p = gnsscorr.RingDecimator(gctx, src, 2, _taps(7), ring)
    assert p.output_info() == (out_fmt, 1.0, 0)
    p.set_output_scale(127.0)
    assert p.output_info() == (out_fmt, 127.0, 0)
    # the ring is kernel-fed now: a plain push is refused
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        ring.push(np.zeros((8, 2), np.int16 if out_name == "GC_IQ_I16" else np.int8))
    assert e.value.status == gnsscorr.GC_ERR_STATE
    p.close()
    ring.close()
    if src:
        src.close()


def test_an_integer_ring_must_be_opened_first(gctx):
    """Quantising is opt-in per ring: without gc_stream_accept_quantised_output both producers refuse an integer ring with
    GC_ERR_INVALID, as they always did, and leave it a plain ring; the call itself is refused on a float ring (GC_ERR_INVALID) and
    once the ring has samples or a producer (GC_ERR_STATE)."""
    import gnsscorr
    i16 = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=gnsscorr.GC_IQ_I16)
    src = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64, iq_format=gnsscorr.GC_IQ_I16)
    for make in (lambda: gnsscorr.Conditioner(gctx, i16, FS_IN, 0.0, 2, _taps(7), gnsscorr.GC_IQ_I16), lambda: gnsscorr.RingDecimator(gctx, src, 2, _taps(7), i16)):
        with pytest.raises(gnsscorr.GnsscorrError) as e:
            make()
        assert e.value.status == gnsscorr.GC_ERR_INVALID and "gc_stream_accept_quantised_output" in str(e.value)
    f32 = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        f32.accept_quantised_output()
    assert e.value.status == gnsscorr.GC_ERR_INVALID
    # opened: still a plain ring until a producer exists; then the producer is created, and a second opening is refused
    assert i16.accept_quantised_output() is i16 and i16.accept_quantised_output() is i16
    cond = gnsscorr.Conditioner(gctx, i16, FS_IN, 0.0, 2, _taps(7), gnsscorr.GC_IQ_I16)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        i16.accept_quantised_output()
    assert e.value.status == gnsscorr.GC_ERR_STATE
    src.push(np.zeros((8, 2), np.int16))
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        src.accept_quantised_output()
    assert e.value.status == gnsscorr.GC_ERR_STATE
    for h in (cond, f32, src, i16):
        h.close()


def test_setter_rules(gctx):
    import gnsscorr
    raw = _raw(64, "GC_IQ_I16", 1)
    # a float ring has no scale; its info says scale 1, nothing clipped
    f32 = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    cond = gnsscorr.Conditioner(gctx, f32, FS_IN, 0.0, 1, _taps(1), gnsscorr.GC_IQ_I16)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        cond.set_output_scale(2.0)
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "GC_IQ_F32" in str(e.value)
    dec_out = gnsscorr.IqStream(gctx, capacity_samples=1024, max_window_samples=64)
    dec = gnsscorr.RingDecimator(gctx, f32, 1, _taps(1), dec_out)
    with pytest.raises(gnsscorr.GnsscorrError) as e:
        dec.set_output_scale(2.0)
    assert e.value.status == gnsscorr.GC_ERR_INVALID and "GC_IQ_F32" in str(e.value)
    assert cond.output_info() == (gnsscorr.GC_IQ_F32, 1.0, 0) and dec.output_info() == (gnsscorr.GC_IQ_F32, 1.0, 0)
    for h in (dec, cond, dec_out, f32):
        h.close()
    # an integer ring: any number of times before the first push / update, GC_ERR_STATE afterwards, GC_ERR_INVALID for a bad scale
    i16 = _out_ring(gctx, 1024, 64, gnsscorr.GC_IQ_I16)
    cond = gnsscorr.Conditioner(gctx, i16, FS_IN, 0.0, 1, _taps(1), gnsscorr.GC_IQ_I16)
    i8 = _out_ring(gctx, 1024, 64, gnsscorr.GC_IQ_I8)
    dec = gnsscorr.RingDecimator(gctx, i16, 1, _taps(1), i8)
    for p in (cond, dec):
        p.set_output_scale(3.0)
        p.set_output_scale(0.5)
        for bad in (0.0, -2.0, float("nan"), float("inf")):
            with pytest.raises(gnsscorr.GnsscorrError) as e:
                p.set_output_scale(bad)
            assert e.value.status == gnsscorr.GC_ERR_INVALID
        assert p.output_info()[1] == 0.5
    cond.push(raw)
    dec.update()
    for p in (cond, dec):
        with pytest.raises(gnsscorr.GnsscorrError) as e:
            p.set_output_scale(2.0)
        assert e.value.status == gnsscorr.GC_ERR_STATE
        assert p.output_info()[:2] == (p._ring.iq_format, 0.5)
    # scale 0.5 on integers: the cshort ring holds rint(x / 2), the cbyte ring rint(rint(x / 2) / 2)
    want16, _ = conditioner_out_ref.quantise(raw.astype(np.float32).reshape(-1).view(np.complex64), gnsscorr.GC_IQ_I16, 0.5)
    assert np.array_equal(i16.read(0, 64), want16)
    want8, _ = conditioner_out_ref.quantise(want16.astype(np.float32).reshape(-1).view(np.complex64), gnsscorr.GC_IQ_I8, 0.5)
    assert np.array_equal(i8.read(0, 64), want8)
    for h in (dec, cond, i8, i16):
        h.close()


@pytest.mark.parametrize("in_name", ["GC_IQ_F32", "GC_IQ_I16", "GC_RAW_REAL_I16"])
@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("D, T", [(1, 1), (3, 7)])
@pytest.mark.parametrize("out_name, scale", [("GC_IQ_I16", 300.0), ("GC_IQ_I8", 1.0)])
def test_conditioner_values(gctx, out_name, scale, D, T, mix, in_name):
    """Raw samples of about 40 LSB rms with a tone of 80: scale 300 makes the cshort ring clip at the tone's peaks, scale 1 the cbyte
    ring at the larger noise peaks (for D, T = 1, 1; the filter of T = 7 passes less)."""
    out_fmt = _fmt(out_name)
    n = 6035
    raw, taps, y = _twin(gctx, "conditioner", in_name, D, T, mix, n)
    seen = []
    got, oldest, info, _ = _run_conditioner(gctx, raw, in_name, out_fmt, D, taps, 1.25e6 if mix else 0.0, scale, RING_CAP, RING_WIN, PUSHES,
        _checker(y, out_fmt, scale, seen))
    assert len(seen) >= len(PUSHES) and seen[-1][1] == len(y)
    assert len(y) >= 2 * RING_CAP and oldest == len(y) - RING_CAP
    if (D, T) == (1, 1):
        assert seen[-1][2] > 0  # the clamp acted, and the count was exact after every push


@pytest.mark.parametrize("in_name", ["GC_IQ_F32", "GC_IQ_I16"])
@pytest.mark.parametrize("D, T", [(1, 1), (3, 7)])
@pytest.mark.parametrize("out_name, scale", [("GC_IQ_I16", 300.0), ("GC_IQ_I8", 1.0)])
def test_decimator_values(gctx, out_name, scale, D, T, in_name):
    """The decimator has neither a mixer nor real input: every source format it has a distinct load path for, both (D, T)."""
    out_fmt = _fmt(out_name)
    n = 6035
    raw, taps, y = _twin(gctx, "decimator", in_name, D, T, False, n)
    seen = []
    got, oldest, info, _ = _run_decimator(gctx, raw, in_name, out_fmt, D, taps, scale, RING_CAP, RING_WIN, PUSHES, _checker(y, out_fmt, scale, seen))
    assert seen[-1][1] == len(y) and oldest == len(y) - RING_CAP
    # bit identity between the two producers in every output format: the conditioner without translation stored the same
    _, _, y_cond = _twin(gctx, "conditioner", in_name, D, T, False, n)
    assert y_cond.tobytes() == y.tobytes()


@pytest.mark.parametrize("out_name", ["GC_IQ_I16", "GC_IQ_I8"])
def test_tile_instantiations(gctx, out_name):
    """cond_tile_outputs: tile = 1024, halved while a launch would not reach want = 2 x CUs workgroups, never below 256 (D = 1,
    T = 3 fits in LDS at 1024).  With int8 input a chunk is 2 Mi raw samples, so each push below is one launch:
      100 outputs                 -> tile 256  (R = 1), one short workgroup
      (want - 1) * 512 + 37       -> tile 512  (R = 2): ceil(n / 1024) < want <= ceil(n / 512)
      (want - 1) * 1024 + 37      -> tile 1024 (R = 4): ceil(n / 1024) = want
    (262 281 and 523 301 outputs on 256 CUs).  Each launch's last tile is ragged (n_out % 64 = 36, 37, 37), and the second and third
    pieces start at odd outputs."""
    import gnsscorr
    import torch
    out_fmt = _fmt(out_name)
    want_groups = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    sizes = [100, (want_groups - 1) * 512 + 37, (want_groups - 1) * 1024 + 37]
    assert all(s % 64 != 0 for s in sizes) and sizes[2] < (1 << 21)
    n = sum(sizes)
    rng = np.random.Generator(np.random.PCG64(8))
    raw = rng.integers(-100, 101, size=(n, 2)).astype(np.int8)
    taps = np.array([0.5, 1.0, -0.25], np.float32)
    y, oldest, info, _ = _run_conditioner(gctx, raw, "GC_IQ_I8", gnsscorr.GC_IQ_F32, 1, taps, 0.0, None, n + 256, 128, sizes)
    assert oldest == 0 and len(y) == n
    scale = 250.0 if out_name == "GC_IQ_I16" else 1.0  # |y| <= 175, clipped beyond 131 and 127: a few per cent of the components
    got, oldest, info, _ = _run_conditioner(gctx, raw, "GC_IQ_I8", out_fmt, 1, taps, 0.0, scale, n + 256, 128, sizes)
    want, clipped = conditioner_out_ref.quantise(y, out_fmt, scale)
    assert oldest == 0 and np.array_equal(got, want)
    assert info == (out_fmt, scale, clipped) and 0 < clipped < n


def _edge_values(out_fmt, scale):
    """float32 inputs x whose products x * scale hit the ties, the limits and the specials."""
    lo, hi, _ = conditioner_out_ref.RANGES[out_fmt]
    f = np.float32
    targets = [k + 0.5 for k in range(-6, 6)]  # exact ties, even and odd k, both signs
    targets += [hi - 1.5, hi - 0.5, hi - 0.25, hi, hi + 0.25, hi + 0.5, hi + 1.0, hi + 1000.0, lo + 1.5, lo + 0.5, lo + 0.25, lo, lo - 0.25, lo - 0.5, lo - 1.0,
        lo - 1000.0, 0.0, -0.0, 0.49999997, -0.49999997, 1e-30, 3e38, -3e38]
    x = [f(t) / f(scale) for t in targets]
    # the float32 neighbours of each quotient: with a scale that is no power of two the product may land on either side
    x += [np.nextafter(v, f(np.inf)) for v in x] + [np.nextafter(v, f(-np.inf)) for v in x]
    # ties that survive any scale with an exact product: half-integers times an odd integer scale stay half-integers
    x += [f(k + 0.5) for k in range(-4, 4)]
    x += [f(np.inf), f(-np.inf), f(np.nan)]
    return np.array(x, np.float32)


@pytest.mark.parametrize("producer", ["conditioner", "decimator"])
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("out_name", ["GC_IQ_I16", "GC_IQ_I8"])
def test_rounding_and_saturation(gctx, out_name, scale, producer):
    """T = 1, h = {1}, D = 1 on float input is a copy, so the ring holds the quantised INPUT: exact ties k + 0.5 (even and odd k, both
    signs), values just inside and outside MIN and MAX including (MAX, MAX + 0.5), +-inf and one NaN, with scale 1 and with scale 3
    (no power of two; half-integers times 3 stay exact ties)."""
    import gnsscorr
    out_fmt = _fmt(out_name)
    v = _edge_values(out_fmt, scale)
    x = np.zeros(len(v), np.complex64)  # every value passes through both components; one NaN in each
    x.real, x.imag = v, v[::-1]
    assert np.array_equal(conditioner_out_ref.components(x)[:, 0], v, equal_nan=True)
    want, clipped = conditioner_out_ref.quantise(x, out_fmt, scale)
    lo, hi, _ = conditioner_out_ref.RANGES[out_fmt]
    prod = conditioner_out_ref.components(x) * np.float32(scale)
    # the inputs do hit what the case is about: ties with even and odd k of both signs, and the interval (MAX, MAX + 0.5)
    assert all(np.any(prod == np.float32(t)) for t in (1.5, 4.5, -1.5, -4.5)) and np.any((prod > hi) & (prod < hi + 0.5)) and np.any((prod < lo) & (prod > lo - 0.5))
    if scale == 1.0:
        assert np.any(prod == hi) and np.any(prod == lo) and np.any(prod == hi + 0.5)
    assert clipped > 0 and np.count_nonzero(np.isnan(prod)) == 2
    run = _run_conditioner if producer == "conditioner" else _run_decimator
    args = (gctx, x, "GC_IQ_F32", out_fmt, 1, np.ones(1, np.float32))
    if producer == "conditioner":
        got, oldest, info, _ = run(*args, 0.0, scale, 1024, 64, [len(x)])
    else:
        got, oldest, info, _ = run(*args, scale, 1024, 64, [len(x)])
    assert oldest == 0
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, "inputs %s: got %s, want %s" % (x[bad[:6]], got[bad[:6]].tolist(), want[bad[:6]].tolist())
    assert info == (out_fmt, scale, clipped)


def test_blanking_with_a_cshort_ring(gctx):
    """Pulse blanking acts on the raw ring in front of the FIR: the cshort ring equals the quantised float twin, and the blanking
    state equals the twin's."""
    import gnsscorr
    n, D, T = 12000, 3, 7
    raw = _raw(n, "GC_IQ_I16", seed=77)
    raw[5000:5100] *= 30  # a pulse: three whole segments and two partial ones
    taps = _taps(T)
    blanking = dict(pfa=0.01, length=32, segments_est=50, segments_reset=1000)
    y, oldest, info, b_twin = _run_conditioner(gctx, raw, "GC_IQ_I16", gnsscorr.GC_IQ_F32, D, taps, 1.25e6, None, 1 << 13, RING_WIN, [n], blanking=blanking)
    assert oldest == 0 and b_twin["segments_blanked"] >= 3
    scale = 300.0
    got, oldest, info, b_got = _run_conditioner(gctx, raw, "GC_IQ_I16", gnsscorr.GC_IQ_I16, D, taps, 1.25e6, scale, 1 << 13, RING_WIN, PUSHES, blanking=blanking)
    want, clipped = conditioner_out_ref.quantise(y, gnsscorr.GC_IQ_I16, scale)
    assert oldest == 0 and len(got) == len(want) == (n // 32 * 32 + D - 1) // D
    assert np.array_equal(got, want) and info == (gnsscorr.GC_IQ_I16, scale, clipped) and clipped > 0
    assert b_got == b_twin


def _integer_signal(oracle, n, amp, lim, seed):
    """GPS L1 C/A PRN 12 at 4 Msps in noise, rounded to integers within +-lim: (code, int array [n, 2])."""
    from test_closed_loop_gpu import _signal
    code, x = _signal(oracle, 12, 4e6, n, seed, 905.0, 2100.0)
    q = np.clip(np.round(x.view(np.float32).reshape(-1, 2) * amp), -lim, lim)
    return code, q


def test_downstream_closed_loop_and_acquisition_on_a_conditioned_cshort_ring(gctx, oracle):
    """Integer-valued float input through T = 1, h = {1}, D = 1, scale = 1 leaves exactly those integers in the conditioned cshort
    ring; a plain cshort ring gets the same integers by push.  One closed-loop channel (4000 samples per code, 3 code periods) and one
    dwell_stream must return the same bits from both: the kernel-written mirror (windows cross the ring's end at 9001), the reader
    table and the eviction guard serve a kernel-fed integer ring as they serve a pushed one."""
    import gnsscorr
    from test_closed_loop_gpu import GPS, _conf
    n_ep, cap = 3, 9001  # odd capacity; 9001 < 4 * 4000: the third window wraps
    code, q = _integer_signal(oracle, 4000 * (n_ep + 2), 64.0, 32767, 66)
    xf = q.astype(np.float32).reshape(-1).view(np.complex64)
    conf = dict(GPS, acq_delay_samples=2100.0, acq_doppler_hz=900.0, acq_samplestamp_samples=0, sample_counter=0)
    records, dwells = [], []
    for kind in ("conditioned", "pushed"):
        ring = gnsscorr.IqStream(gctx, capacity_samples=cap, max_window_samples=4000, iq_format=gnsscorr.GC_IQ_I16)
        if kind == "conditioned":
            ring.accept_quantised_output()
        cond = gnsscorr.Conditioner(gctx, ring, 4e6, 0.0, 1, np.ones(1, np.float32), gnsscorr.GC_IQ_F32) if kind == "conditioned" else None
        loop = gnsscorr.TrackingLoop(gctx, 1, 1023)
        loop.set_input_format(gnsscorr.GC_IQ_I16)
        loop.set_input_stream(0, ring)
        loop.start(0, _conf(gnsscorr, **conf), code)
        acq = gnsscorr.PcpsAcquisition(gctx, 1, 4_000_000, 1, 1, np.float32(4e6) * np.float32(0.001), 4000.0, 4, 5000, 250)
        acq.set_input_format(gnsscorr.GC_IQ_I16)
        acq.set_local_code(0, gnsscorr.gps_l1_ca_code_gen_complex_sampled(12, 4_000_000))
        got, pushed = [], 0
        for m in (4001, 3999, 2501, 4499, 5000):  # odd cuts: 15000 of the 20000 samples reach the loop before it has 3 records
            if cond:
                assert cond.push(xf[pushed:pushed + m]) == (pushed, m)
            else:
                assert ring.push(q[pushed:pushed + m].astype(np.int16)) == pushed
            pushed += m
            if len(got) < n_ep:
                got.extend(r.copy() for r in loop.run(n_ep - len(got))[0] if r["valid"])
        assert pushed == len(q) and len(got) == n_ep
        records.append(np.array(got))
        # samples [16000, 20000) live at ring positions 6999 .. 9000 and 0 .. 1997: the search reads through the mirror
        dwells.append(acq.dwell_stream(ring, 16000)[0])
        if cond:
            assert cond.output_info() == (gnsscorr.GC_IQ_I16, 1.0, 0)
            assert np.array_equal(ring.read(pushed - cap, cap), q[pushed - cap:].astype(np.int16))
            cond.close()
        acq.close()
        loop.close()
        ring.close()
    for name in records[0].dtype.names:
        assert np.array_equal(records[0][name], records[1][name]), name
    a, b = dwells
    assert (a.indext, a.doppler_hz, a.mag, a.test_statistics, a.acq_delay_samples) == (b.indext, b.doppler_hz, b.mag, b.test_statistics, b.acq_delay_samples)
    assert a.test_statistics > 0.0


def test_downstream_tracking_batch_on_a_conditioned_cbyte_ring(gctx, oracle):
    """The same for a cbyte ring and the tracking batch: 5 epochs of 4000 samples on a ring of 9001 (odd), pushed in odd cuts; the
    epochs at 8000 and 16000 cross the ring's end and read the mirror the conditioner's packed stores wrote."""
    import gnsscorr
    from helpers import open_loop_params
    n, n_epochs, cap = 4000, 5, 9001
    truth = dict(code_rate=1.023e6 * (1 + 905.0 / 1575.42e6), tau0=1023.0 - 2100.0 * 1.023e6 / 4e6, doppler=905.0, phi=0.4)
    code, q = _integer_signal(oracle, n * n_epochs, 12.0, 127, 67)
    xf = q.astype(np.float32).reshape(-1).view(np.complex64)
    shifts = np.array([-0.5, 0.0, 0.5], np.float32)
    recs = [gnsscorr.epoch_params(p["sample_offset"], float(p["rem_carr"]), float(p["phase_step"]), float(p["rem_code"]), float(p["code_step"]), n)
        for p in open_loop_params(truth, 4e6, 1023, n, n_epochs)]
    results = []
    for kind in ("conditioned", "pushed"):
        ring = gnsscorr.IqStream(gctx, capacity_samples=cap, max_window_samples=n, iq_format=gnsscorr.GC_IQ_I8)
        if kind == "conditioned":
            ring.accept_quantised_output()
        cond = gnsscorr.Conditioner(gctx, ring, 4e6, 0.0, 1, np.ones(1, np.float32), gnsscorr.GC_IQ_F32) if kind == "conditioned" else None
        b = gnsscorr.TrackingBatch(gctx, 1, 3, 1023)
        b.set_input_format(gnsscorr.GC_IQ_I8)
        b.set_code(0, code, shifts)
        b.set_input_stream(0, ring)
        out, pushed, done = [], 0, 0
        for m in (4001, 3999, 2501, 4499, 5000):
            if cond:
                assert cond.push(xf[pushed:pushed + m]) == (pushed, m)
            else:
                assert ring.push(q[pushed:pushed + m].astype(np.int8)) == pushed
            pushed += m
            while done < n_epochs and (done + 1) * n <= pushed:
                out.append(b.run(1, gnsscorr.epoch_params_array([[recs[done]]]))[0, 0].copy())
                done += 1
        assert done == n_epochs
        if cond:
            assert cond.output_info() == (gnsscorr.GC_IQ_I8, 1.0, 0)
            cond.close()
        results.append(np.array(out))
        b.close()
        ring.close()
    assert results[0].tobytes() == results[1].tobytes()
    assert np.abs(results[0][:, 1]).min() > 0.0
