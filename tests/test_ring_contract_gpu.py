"""GPU conformance tests of the ring contract: after every call of every writer of a gc_stream ring -- the host push, the conditioner
(with and without pulse blanking), the ring decimator, the ring resampler in both modes, the notch stage and the signal generator --
EVERY stored byte of the ring, of its mirror and of the slack behind it equals a host model (tests/ring_model.py), and the guard
bands in front of and behind the storage still hold their fill (gc_stream_debug_read_storage, gc_stream_debug_guards).

Each case runs twice.  One call into a ring that never wraps gives all outputs y; y is first held against the restatement and
the gate the producer's own test module uses (conditioner_ref / blanking_ref with conditioner_ref.error_bound, resampler_ref,
notch_ref through test_notch_gpu._compare, siggen_ref with test_siggen_gpu's gate; an integer ring against
conditioner_out_ref.quantise of the float ring's outputs, exactly), so that the model does not rest on the code under test alone.
Then a small ring of odd capacity is fed by the schedule of tests/ring_contract_cases.py, whose pieces start and end at odd
positions inside and outside the mirror part, include single samples at its corners and calls longer than the ring, and wrap it
several times (tests/test_ring_model.py checks that on the CPU); the model is fed the same slices of y.  What the value tests of
the stages cannot see shows here: a mirror that is stale, short or wrong at an odd end, and a store outside the piece.

A failure names the first storage position that differs and whether it lies in the ring, the mirror or the slack."""
import numpy as np
import pytest

import blanking_ref
import conditioner_out_ref as out_ref
import conditioner_ref
import resampler_ref
import ring_contract_cases as cases
import ring_model
import siggen_cases
import siggen_ref

pytestmark = pytest.mark.gpu
FS_IN = 16e6
CAP, WIN = cases.CAPACITY, cases.WINDOW
BIG = 1 << 14      # an output ring that holds a whole schedule (15626 outputs at most) without wrapping
SRC_CAP = 1 << 16  # a source ring that holds the whole source of a derived ring's schedule (46873 samples at most)
OUT_NAMES = ["GC_IQ_F32", "GC_IQ_I16", "GC_IQ_I8"]
COMPLEX_IN = ["GC_IQ_F32", "GC_IQ_I16", "GC_IQ_I8"]
REAL_IN = ["GC_RAW_REAL_F32", "GC_RAW_REAL_I16", "GC_RAW_REAL_I8", "GC_RAW_REAL_2BIT"]
_shared = {}  # references and unwrapped runs, computed once and shared; nobody changes them


def _fmt(name):
    import gnsscorr
    return getattr(gnsscorr, name)


def _ring(gctx, capacity, window, fmt, device_quantiser=False):
    """A ring; an integer ring that a conditioner, a ring decimator or the generator quantises into is opened for that."""
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, capacity_samples=capacity, max_window_samples=window, iq_format=fmt)
    return ring.accept_quantised_output() if device_quantiser and fmt != gnsscorr.GC_IQ_F32 else ring


def _close(*handles):
    for h in handles:
        h.close()


def _check_storage(ring, model, what):
    got = ring.read_storage(0, model.total)
    diff = model.first_difference(got)
    assert diff is None, "%s: storage position %d, in the %s, holds %s; the model holds %s; newest pieces (pos, len) %s" % ((what,) + diff + (model.pieces[-3:],))
    assert ring.guards_intact() == (True, True), "%s: (front, back) guard band intact: %s" % (what, ring.guards_intact())


def _conform(ring, window, y, out_heads, advance, what, clipped=None, required=None, tile=256):
    """advance(k) makes call k on the device; after each call the ring's head, its whole storage, both guard bands and (integer
    rings: clipped() = (the producer's count, the restated count of the outputs so far)) are asserted.  Returns the model."""
    import gnsscorr
    oldest, head, capacity = ring.info()
    assert (oldest, head) == (0, 0) and len(y) == out_heads[-1]
    dt, per = gnsscorr.IqStream._DTYPES[ring.iq_format]
    model = ring_model.RingModel(capacity, window, dt, per)
    _check_storage(ring, model, what + ", before the first call")  # zeroed storage, filled guard bands
    prev = 0
    for k, h in enumerate(out_heads):
        advance(k)
        assert ring.info()[:2] == (max(0, h - capacity), h), (what, k, ring.info(), h)
        model.append(y[prev:h])
        _check_storage(ring, model, "%s, call %d (outputs %d .. %d)" % (what, k, prev, h))
        if clipped is not None:
            got, want = clipped(h)
            assert got == want, "%s, call %d: %d clipped components counted, %d restated" % (what, k, got, want)
        prev = h
    if required is not None:
        missing = required - ring_model.classify(model.pieces, model.calls, capacity, window, tile)
        assert not missing, (what, sorted(missing))
    return model


def _scale_from(ref, out_fmt):
    """A scale that makes the largest components of the float64 restatement clip and most of them not: MAX / (0.6 peak)."""
    peak = max(np.abs(ref.real).max(), np.abs(ref.imag).max())
    return float(np.float32(out_ref.RANGES[out_fmt][1] / (0.6 * peak)))


def _component_error(y, ref):
    return float(max(np.abs(y.real - ref.real).max(), np.abs(y.imag - ref.imag).max()))


# ---- host push: validates the harness too ----

@pytest.mark.parametrize("fmt_name", OUT_NAMES)
def test_host_push(gctx, fmt_name):
    import gnsscorr
    fmt = _fmt(fmt_name)
    dt, per = gnsscorr.IqStream._DTYPES[fmt]
    out_heads = cases.heads(cases.INCREMENTS_NO_G)
    rng = np.random.Generator(np.random.PCG64(3))
    if per == 1:
        y = (rng.standard_normal(out_heads[-1]) + 1j * rng.standard_normal(out_heads[-1])).astype(np.complex64)
    else:
        y = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max + 1, size=(out_heads[-1], 2)).astype(dt)
    ring = _ring(gctx, CAP, WIN, fmt)
    bounds = [0] + out_heads
    _conform(ring, WIN, y, out_heads, lambda k: ring.push(y[bounds[k]:bounds[k + 1]]), "host push " + fmt_name, required=cases.REQUIRED["host"], tile=1)
    # the diagnostic read takes positions inside the storage alone, and what the resident window reads back is what it shows
    total = CAP + WIN + ring_model.SLACK
    assert len(ring.read_storage(total, 0)) == 0 and len(ring.read_storage(total - 1, 1)) == 1
    for first, n in ((total, 1), (0, total + 1), (total + 1, 0), (1 << 63, 1), ((1 << 64) - 1, 2)):
        with pytest.raises(gnsscorr.GnsscorrError) as e:
            ring.read_storage(first, n)
        assert e.value.status == gnsscorr.GC_ERR_INVALID and "outside the ring's storage" in str(e.value)
    head = out_heads[-1]
    pos = (head - 50) % CAP
    assert ring.read(head - 50, 50).tobytes() == ring.read_storage(pos, 50).tobytes() == y[head - 50:].tobytes()
    ring.close()


# ---- conditioner ----

def _cond_raw(in_name, n, seed):
    """(the raw stream as pushed, indexable by sample except GC_RAW_REAL_2BIT's packed bytes; the same stream in the layout
    conditioner_ref.to_complex takes): seeded noise plus a tone, scaled to the format as tests/test_conditioner_gpu.py does."""
    import gnsscorr
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5) + 2.0 * np.exp(2j * np.pi * 1.3e6 * np.arange(n) / FS_IN + 0.3j)
    kind, width = in_name.rsplit("_", 1)
    if in_name == "GC_RAW_REAL_2BIT":
        v = rng.integers(-2, 2, n).astype(np.int8)
        return gnsscorr.pack_2bit(v), np.stack([v, np.zeros_like(v)], axis=1)
    if kind == "GC_IQ":
        if width == "F32":
            raw = (x * 40.0).astype(np.complex64)
        else:
            scale, dt, lim = (1000.0, np.int16, 32767) if width == "I16" else (20.0, np.int8, 127)
            raw = np.clip(np.round(np.stack([x.real, x.imag], axis=1) * scale), -lim, lim).astype(dt)
        return raw, raw
    if width == "F32":
        raw = (x.real * 40.0).astype(np.float32)
        return raw, raw.astype(np.complex64)
    scale, dt, lim = (1000.0, np.int16, 32767) if width == "I16" else (20.0, np.int8, 127)
    raw = np.clip(np.round(x.real * scale), -lim, lim).astype(dt)
    return raw, np.stack([raw, np.zeros_like(raw)], axis=1)


def _cond_slice(in_name, raw, a, b):
    return raw[a // 4:b // 4] if in_name == "GC_RAW_REAL_2BIT" else raw[a:b]


def _cond_make(gctx, ring, case, scale):
    import gnsscorr
    cond = gnsscorr.Conditioner(gctx, ring, FS_IN, case["f"], case["D"], case["taps"], _fmt(case["in_name"]))
    if scale is not None:
        cond.set_output_scale(scale)
    if case["blanking"]:
        L, pfa, est, reset = case["blanking"]
        cond.set_pulse_blanking(pfa=pfa, length=L, segments_est=est, segments_reset=reset)
    return cond


def _cond_unwrapped(gctx, case, out_fmt, scale):
    """All outputs of the case from one push into a ring that never wraps, and the producer's output_info."""
    ring = _ring(gctx, BIG, WIN, out_fmt, device_quantiser=True)
    cond = _cond_make(gctx, ring, case, scale)
    n_out = case["out_heads"][-1]
    assert cond.push(_cond_slice(case["in_name"], case["raw"], 0, case["raw_heads"][-1])) == (0, n_out)
    y, info = ring.read(0, n_out), cond.output_info()
    _close(cond, ring)
    y.setflags(write=False)
    return y, info


def _cond_case(gctx, in_name, D, T, mix, blanking=False):
    """The schedule, the raw stream, the float64 restatement and the float ring's outputs of one configuration, the latter held
    against the former within conditioner_ref.error_bound: made once, shared by the three output formats."""
    key = ("conditioner", in_name, D, T, mix, blanking)
    if key not in _shared:
        from test_conditioner_gpu import _taps
        import gnsscorr
        case = dict(in_name=in_name, D=D, T=T, f=1.25e6 if mix else 0.0, taps=_taps(T, D), blanking=None)
        if blanking:
            from test_blanking_gpu import SHAPES, _case
            L, pfa, est, reset = SHAPES[0]
            raw, ref_b, _ = _case(L, pfa, est, reset, in_name[len("GC_IQ_"):])
            case["blanking"] = (L, pfa, est, reset)
            case["raw_heads"] = cases.segment_raw_heads(cases.SEGMENTS_NO_G_32, L)
            case["out_heads"] = cases.fir_out_heads(case["raw_heads"], D, segment=L)
            case["raw"] = raw[:case["raw_heads"][-1]]
            flags = ref_b["flags"][:case["raw_heads"][-1] // L]  # the decisions are causal: those of the whole stream's first segments
            assert 0 < flags.sum() < len(flags)
            as_complex, filtered = case["raw"], blanking_ref.apply(case["raw"], L, flags)
        else:
            two_bit = in_name == "GC_RAW_REAL_2BIT"
            case["out_heads"] = cases.heads(cases.INCREMENTS_2BIT if two_bit else cases.INCREMENTS_NO_G)
            case["raw_heads"] = cases.fir_raw_heads(case["out_heads"], D, multiple=4 if two_bit else 1)
            case["raw"], as_complex = _cond_raw(in_name, case["raw_heads"][-1], seed=100 + D)
            filtered = as_complex
        n_out = case["out_heads"][-1]
        case["ref"] = conditioner_ref.condition(filtered, case["taps"], D, case["f"], FS_IN, 0, n_out)
        y, info = _cond_unwrapped(gctx, case, gnsscorr.GC_IQ_F32, None)
        bound = conditioner_ref.error_bound(case["taps"], as_complex)
        err = _component_error(y, case["ref"])
        print("conditioner %s D=%d T=%d f=%g%s: max component error %.3e, bound %.3e" % (in_name, D, T, case["f"], " blanking" if blanking else "", err, bound))
        assert y.dtype == np.complex64 and err <= bound and info == (gnsscorr.GC_IQ_F32, 1.0, 0)
        assert np.abs(case["ref"]).max() > 100 * bound  # the gate can tell outputs from silence
        case["y"] = {"GC_IQ_F32": y}
        _shared[key] = case
    return _shared[key]


def _quantised(case, out_name, unwrapped):
    """The outputs of an integer ring: the unwrapped run of that format, equal to the restated epilogue of the float ring's
    outputs, with the restated count of clipped components.  Returns (y, scale)."""
    out_fmt = _fmt(out_name)
    scale = None if out_name == "GC_IQ_F32" else _scale_from(case["ref"], out_fmt)
    if out_name not in case["y"]:
        y, info = unwrapped(out_fmt, scale)
        want, n_clipped = out_ref.quantise(case["y"]["GC_IQ_F32"], out_fmt, scale)
        bad = np.flatnonzero(np.any(y != want, axis=1))
        assert bad.size == 0, "outputs %s ...: got %s, want %s" % (bad[:4], y[bad[:4]].tolist(), want[bad[:4]].tolist())
        assert info == (out_fmt, scale, n_clipped) and 0 < n_clipped < y.size // 4, (info, n_clipped)
        case["y"][out_name] = y
    return case["y"][out_name], scale


def _clipped_counter(producer, case, out_name, scale):
    if out_name == "GC_IQ_F32":
        return None
    out_fmt, y32 = _fmt(out_name), case["y"]["GC_IQ_F32"]
    return lambda head: (producer.output_info()[2], out_ref.quantise(y32[:head], out_fmt, scale)[1])


def _run_conditioner(gctx, in_name, out_name, D, T, mix, blanking=False):
    case = _cond_case(gctx, in_name, D, T, mix, blanking)
    y, scale = _quantised(case, out_name, lambda out_fmt, s: _cond_unwrapped(gctx, case, out_fmt, s))
    ring = _ring(gctx, CAP, WIN, _fmt(out_name), device_quantiser=True)
    cond = _cond_make(gctx, ring, case, scale)
    bounds = [0] + case["raw_heads"]
    heads_seen = []

    def advance(k):
        first, n_out = cond.push(_cond_slice(in_name, case["raw"], bounds[k], bounds[k + 1]))
        heads_seen.append(first + n_out)
    name = "conditioner-blanking" if blanking else "conditioner-2bit" if in_name == "GC_RAW_REAL_2BIT" else "conditioner"
    _conform(ring, WIN, y, case["out_heads"], advance, "%s %s -> %s D=%d T=%d mix=%s" % (name, in_name, out_name, D, T, mix),
        clipped=_clipped_counter(cond, case, out_name, scale), required=cases.REQUIRED[name], tile=cases.TILE["conditioner"])
    assert heads_seen == case["out_heads"]
    _close(cond, ring)


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("out_name", OUT_NAMES)
@pytest.mark.parametrize("in_name", COMPLEX_IN + REAL_IN)
def test_conditioner(gctx, in_name, out_name, mix):
    """Every instantiation of the store epilogue in the conditioner at D = 3, T = 7: seven input formats, three output formats,
    with and without the mixer."""
    _run_conditioner(gctx, in_name, out_name, 3, 7, mix)


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("out_name", OUT_NAMES)
@pytest.mark.parametrize("in_name", COMPLEX_IN)
def test_conditioner_without_filter_or_decimation(gctx, in_name, out_name, mix):
    _run_conditioner(gctx, in_name, out_name, 1, 1, mix)


def test_conditioner_with_pulse_blanking(gctx):
    """Blanking makes the head advance by whole segments of 32 raw samples (D = 1): the notch stage's segment schedule, into a
    cbyte ring."""
    _run_conditioner(gctx, "GC_IQ_I16", "GC_IQ_I8", 1, 7, True, blanking=True)


@pytest.mark.parametrize("out_name", OUT_NAMES)
def test_conditioner_tiles_of_512_and_1024(gctx, out_name):
    """The conditioner takes tiles of 512 and 1024 outputs (R = 2, 4 outputs per lane) only for pieces of about 2 x CUs x 512 and
    x 1024 outputs (tests/test_conditioner_out_gpu.py::test_tile_instantiations has the arithmetic): int8 input, D = 1, T = 3,
    each of the two sizes once as a piece at position 0 and once at an odd position behind the mirror part, on a ring of
    301 + n4 samples."""
    import gnsscorr
    import torch
    want_groups = 2 * torch.cuda.get_device_properties(0).multi_processor_count
    capacity, window, pushes, n2, n4 = cases.tile_pushes(want_groups)
    out_heads = cases.heads(pushes)
    n = out_heads[-1]
    assert n4 < (1 << 21)  # each push is one chunk of raw samples: one launch per piece
    key = ("tiles", want_groups)
    if key not in _shared:
        raw = np.random.Generator(np.random.PCG64(8)).integers(-100, 101, size=(n, 2)).astype(np.int8)
        case = dict(in_name="GC_IQ_I8", D=1, T=3, f=0.0, taps=np.array([0.5, 1.0, -0.25], np.float32), blanking=None, raw=raw, raw_heads=out_heads,
            out_heads=out_heads)
        case["ref"] = conditioner_ref.condition(raw, case["taps"], 1, 0.0, FS_IN)
        ring = _ring(gctx, n + 256, window, gnsscorr.GC_IQ_F32)
        cond = _cond_make(gctx, ring, case, None)
        assert cond.push(raw) == (0, n)
        y = ring.read(0, n)
        _close(cond, ring)
        err, bound = _component_error(y, case["ref"]), conditioner_ref.error_bound(case["taps"], raw)
        print("conditioner tiles: max component error %.3e, bound %.3e" % (err, bound))
        assert err <= bound
        case["y"] = {"GC_IQ_F32": y}
        _shared[key] = case
    case = _shared[key]

    def unwrapped(out_fmt, scale):
        ring = _ring(gctx, n + 256, window, out_fmt, device_quantiser=True)
        cond = _cond_make(gctx, ring, case, scale)
        assert cond.push(case["raw"]) == (0, n)
        got = ring.read(0, n), cond.output_info()
        _close(cond, ring)
        return got
    y, scale = _quantised(case, out_name, unwrapped)
    ring = _ring(gctx, capacity, window, _fmt(out_name), device_quantiser=True)
    cond = _cond_make(gctx, ring, case, scale)
    bounds = [0] + out_heads
    model = _conform(ring, window, y, out_heads, lambda k: cond.push(case["raw"][bounds[k]:bounds[k + 1]]), "conditioner tiles -> " + out_name,
        clipped=_clipped_counter(cond, case, out_name, scale))
    assert model.pieces == [(0, n4), (n4, 301), (0, n2), (n2, n2), (2 * n2, capacity - 2 * n2), (0, 129), (129, n4)]
    _close(cond, ring)


# ---- ring decimator ----

def _source_raw(fmt_name, n, seed):
    """A source ring's samples in its format: tests/test_ring_resampler_gpu.py's noise plus a tone."""
    from test_ring_resampler_gpu import _raw
    return _raw(n, _fmt(fmt_name), seed)


def _derived_unwrapped(gctx, src_fmt, raw, out_fmt, make, n_out, quantiser=True):
    """One update of a derived ring on a source that holds all of `raw`, into a ring that never wraps.  quantiser: the stage
    quantises into an integer ring (the decimator); the resampler's direct mode moves bits into a plain one."""
    src = _ring(gctx, SRC_CAP, 64, src_fmt)
    out = _ring(gctx, BIG, WIN, out_fmt, device_quantiser=quantiser)
    stage = make(src, out)
    src.push(raw)
    assert stage.update() == (0, n_out)
    y = out.read(0, n_out)
    info = stage.output_info() if hasattr(stage, "output_info") else None
    _close(stage, out, src)
    y.setflags(write=False)
    return y, info


def _derived_conform(gctx, src_fmt, raw, src_heads, out_fmt, make, y, out_heads, what, capacity=CAP, clipped=None, required=None, tile=256, quantiser=True):
    src = _ring(gctx, SRC_CAP, 64, src_fmt)
    out = _ring(gctx, capacity, WIN, out_fmt, device_quantiser=quantiser)
    stage = make(src, out)
    bounds = [0] + src_heads
    seen = []

    def advance(k):
        src.push(raw[bounds[k]:bounds[k + 1]])
        first, n_out = stage.update()
        seen.append(first + n_out)
    _conform(out, WIN, y, out_heads, advance, what, clipped=None if clipped is None else clipped(stage), required=required, tile=tile)
    assert seen == out_heads
    _close(stage, out, src)


@pytest.mark.parametrize("D, T", [(1, 1), (3, 7)])
@pytest.mark.parametrize("out_name", OUT_NAMES)
@pytest.mark.parametrize("src_name", OUT_NAMES)
def test_ring_decimator(gctx, src_name, out_name, D, T):
    import gnsscorr
    src_fmt = _fmt(src_name)
    key = ("decimator", src_name, D, T)
    if key not in _shared:
        from test_conditioner_gpu import _taps
        case = dict(D=D, taps=_taps(T, D), out_heads=cases.heads(cases.INCREMENTS))
        case["src_heads"] = cases.fir_raw_heads(case["out_heads"], D)
        case["raw"] = _source_raw(src_name, case["src_heads"][-1], seed=200 + D)
        case["ref"] = conditioner_ref.condition(case["raw"], case["taps"], D, 0.0, FS_IN)
        y, info = _derived_unwrapped(gctx, src_fmt, case["raw"], gnsscorr.GC_IQ_F32, lambda s, o: gnsscorr.RingDecimator(gctx, s, D, case["taps"], o), case["out_heads"][-1])
        err, bound = _component_error(y, case["ref"]), conditioner_ref.error_bound(case["taps"], case["raw"])
        print("ring decimator %s D=%d T=%d: max component error %.3e, bound %.3e" % (src_name, D, T, err, bound))
        assert err <= bound and info == (gnsscorr.GC_IQ_F32, 1.0, 0) and np.abs(case["ref"]).max() > 100 * bound
        case["y"] = {"GC_IQ_F32": y}
        _shared[key] = case
    case = _shared[key]

    def make_with(scale):
        def make(s, o):
            dec = gnsscorr.RingDecimator(gctx, s, D, case["taps"], o)
            if scale is not None:
                dec.set_output_scale(scale)
            return dec
        return make
    y, scale = _quantised(case, out_name, lambda out_fmt, s: _derived_unwrapped(gctx, src_fmt, case["raw"], out_fmt, make_with(s), case["out_heads"][-1]))
    _derived_conform(gctx, src_fmt, case["raw"], case["src_heads"], _fmt(out_name), make_with(scale), y, case["out_heads"],
        "ring decimator %s -> %s D=%d T=%d" % (src_name, out_name, D, T), clipped=lambda dec: _clipped_counter(dec, case, out_name, scale),
        required=cases.REQUIRED["decimator"])


# ---- ring resampler ----

@pytest.mark.parametrize("direction", ["down", "up"])
@pytest.mark.parametrize("fmt_name", OUT_NAMES)
def test_ring_resampler_direct(gctx, fmt_name, direction):
    """Direct mode moves bits: its 8-, 4- and 2-byte stores, at 25 -> 10 and at 4 -> 5 (one or two outputs per source sample)."""
    import gnsscorr
    fmt = _fmt(fmt_name)
    fs_in, fs_out = cases.DIRECT_DOWN if direction == "down" else cases.DIRECT_UP
    kind, step = resampler_ref.direct_ratio(fs_in, fs_out)
    out_heads = cases.heads(cases.INCREMENTS)
    src_heads = cases.source_heads(lambda h: resampler_ref.available(kind, step, h), out_heads)
    raw = _source_raw(fmt_name, src_heads[-1], seed=300)

    def make(s, o):
        return gnsscorr.RingResampler(gctx, s, fs_in, fs_out, o, "direct")
    y, _ = _derived_unwrapped(gctx, fmt, raw, fmt, make, out_heads[-1], quantiser=False)
    want = resampler_ref.direct(raw, fs_in, fs_out)
    assert y.dtype == raw.dtype and y.shape == want.shape and y.tobytes() == want.tobytes()
    _derived_conform(gctx, fmt, raw, src_heads, fmt, make, y, out_heads, "ring resampler direct %s %s" % (fmt_name, direction),
        required=cases.REQUIRED["resampler-" + direction], quantiser=False)


@pytest.mark.parametrize("src_name", OUT_NAMES)
def test_ring_resampler_polyphase(gctx, src_name):
    import gnsscorr
    src_fmt = _fmt(src_name)
    fs_in, fs_out, phases = cases.POLYPHASE
    if "bank" not in _shared:
        _shared["bank"] = gnsscorr.resampler_design(fs_in, fs_out, phases)
    bank = _shared["bank"]
    kind, inc = resampler_ref.poly_ratio(fs_in, fs_out)
    out_heads = cases.heads(cases.INCREMENTS)
    src_heads = cases.source_heads(lambda h: resampler_ref.available(kind, inc, h), out_heads)
    raw = _source_raw(src_name, src_heads[-1], seed=400)

    def make(s, o):
        return gnsscorr.RingResampler(gctx, s, fs_in, fs_out, o, "polyphase", bank)
    y, _ = _derived_unwrapped(gctx, src_fmt, raw, gnsscorr.GC_IQ_F32, make, out_heads[-1])
    ref = resampler_ref.polyphase(raw, bank, fs_in, fs_out)
    err, bound = _component_error(y, ref), resampler_ref.error_bound(bank, raw)
    print("ring resampler polyphase %s P=%d T=%d: max component error %.3e, bound %.3e" % (src_name, bank.shape[0], bank.shape[1], err, bound))
    assert len(ref) == out_heads[-1] and err <= bound and np.abs(ref).max() > 100 * bound
    _derived_conform(gctx, src_fmt, raw, src_heads, gnsscorr.GC_IQ_F32, make, y, out_heads, "ring resampler polyphase from " + src_name,
        required=cases.REQUIRED["resampler-polyphase"])


# ---- notch stage ----

@pytest.mark.parametrize("name", ["full", "lite3", "full-33"])
def test_ring_notch(gctx, name):
    """Both of the stage's kernels store the mirror: the copy kernel for the segments that pass, the filter kernel for the filtered
    ones.  The stage appends whole segments, so it cannot reach the single-sample pieces (tests/ring_contract_cases.py,
    SEGMENT_CLASSES, has the reason); the wrap of an odd capacity still cuts its segments at odd positions."""
    import gnsscorr
    import test_notch_gpu as tn
    x, ref = tn._scene(name)
    args = tn._args(name)
    L = args["L"]
    oldest, y, st = tn._run(gctx, x, args, [len(x)])
    assert oldest == 0
    tn._compare(x, ref, y, st, L, name)
    src_heads = cases.segment_raw_heads(cases.SEGMENTS[L], L)
    out_heads = [h // L * L for h in src_heads]
    flags = ref["flags"][:out_heads[-1] // L]
    assert flags.any() and not flags.all()
    # of the segments that the three wraps cut, some are filtered and some pass: both kernels write pieces with a mirror part
    capacity = cases.SEGMENT_CAPACITY[L]
    assert out_heads[-1] > 3 * capacity
    at_wrap = [bool(ref["flags"][lap * capacity // L]) for lap in (1, 2, 3)]
    assert True in at_wrap and False in at_wrap, at_wrap
    y = y[:out_heads[-1]].copy()
    _derived_conform(gctx, gnsscorr.GC_IQ_F32, x, src_heads, gnsscorr.GC_IQ_F32, lambda s, o: tn._make(gctx, s, o, args), y, out_heads, "ring notch " + name,
        capacity=capacity, required=cases.REQUIRED["notch-%d" % L], tile=cases.TILE["notch"])


# ---- signal generator ----

@pytest.mark.parametrize("placement", ["hbm", "lds"])
@pytest.mark.parametrize("out_name", OUT_NAMES)
def test_signal_generator(gctx, out_name, placement):
    """The generator's own stores (two 16-byte words per lane with 8-byte stores at odd ends, 8-byte stores for the mirror) and the
    shared epilogue behind its tiles of 1024; noise on, an odd first scenario sample."""
    import gnsscorr
    sats, sigma, seed = siggen_cases.acquisition_scene(gnsscorr)
    t0 = 12345
    out_heads = cases.heads(cases.INCREMENTS)
    n = out_heads[-1]

    def make(ring, scale):
        gen = gnsscorr.SignalGenerator(gctx, ring, siggen_cases.FS, sats, noise_sigma=sigma, seed=seed, t0=t0, table_placement=placement)
        if scale is not None:
            gen.set_output_scale(scale)
        return gen

    def unwrapped(out_fmt, scale):
        ring = _ring(gctx, BIG, WIN, out_fmt, device_quantiser=True)
        gen = make(ring, scale)
        assert gen.generate(n) == 0
        got = ring.read(0, n), gen.output_info()
        _close(gen, ring)
        return got
    key = ("siggen", placement)
    if key not in _shared:
        if "siggen-ref" not in _shared:
            from test_siggen_gpu import _gate
            dicts = [siggen_ref.from_satellite(s, siggen_cases.FS) for s in sats]
            _shared["siggen-ref"] = (siggen_ref.generate(dicts, sigma, seed, t0, n), _gate(dict(dicts=dicts), sigma))
        ref, gate = _shared["siggen-ref"]
        y, info = unwrapped(gnsscorr.GC_IQ_F32, None)
        err = float(np.max(np.abs(y.astype(np.complex128) - ref)))
        print("signal generator, tables in %s: max |dev - ref| = %.3e, gate %.3e" % (placement, err, gate))
        assert y.dtype == np.complex64 and err <= gate and info == (gnsscorr.GC_IQ_F32, 1.0, 0) and np.abs(ref).max() > 0.5
        _shared[key] = dict(ref=ref, y={"GC_IQ_F32": y})
    case = _shared[key]
    y, scale = _quantised(case, out_name, unwrapped)
    ring = _ring(gctx, CAP, WIN, _fmt(out_name), device_quantiser=True)
    gen = make(ring, scale)
    firsts = []
    _conform(ring, WIN, y, out_heads, lambda k: firsts.append(gen.generate(cases.INCREMENTS[k])), "signal generator -> %s, tables in %s" % (out_name, placement),
        clipped=_clipped_counter(gen, case, out_name, scale), required=cases.REQUIRED["siggen"], tile=cases.TILE["siggen"])
    assert firsts == [0] + out_heads[:-1]
    _close(gen, ring)
