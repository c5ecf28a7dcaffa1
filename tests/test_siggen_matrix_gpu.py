"""GPU tests of the signal generator over the scene table of tests/siggen_cases.py (MATRIX): every signal kind the library constructs
(GPS L1 C/A, GLONASS L1, Galileo E1 and E5a), components on the imaginary axis, tables of 2 to 49104 entries in HBM and in LDS, 32
satellites, code periods shorter than a thread's run, and sample numbers at the carries of 2^32, 2^63 and 2^64.
tests/test_siggen_matrix_inputs.py shows, without a device, that each scene holds the events these tests are about.

What is compared:
  parity     complex64 device samples against the float64 restatement (tests/siggen_ref.py), max |dev - ref| <= the gate of
             tests/test_siggen_gpu.py, 1e-5 A + 2e-5 sigma (derived in that file's header for up to 32 accumulations)
  exact      complex64 VALUES (np.array_equal: -0.0 equals +0.0) under a carrier that is exactly 1
  cut / wrap the ring's bytes against the bytes of the uncut float ring
  integer    the int16 / int8 ring's bytes against the restated quantisation (tests/conditioner_out_ref.py) of the float ring's own
             device output -- the strided run of the integer kernels against the consecutive run of the float kernel
A mismatch names the first differing sample, its tile of 1024 and its lane in the tile."""
import numpy as np
import pytest

import conditioner_out_ref as out_ref
import siggen_cases as cases
import siggen_ref as ref
from test_siggen_gpu import _gate, _generate

pytestmark = pytest.mark.gpu
NAMES = tuple(cases.MATRIX)
CUT_CAPACITY, CUT_WINDOW = 1537, 512  # odd: the wrap and the mirror are crossed at odd positions


def _where(i):
    return "sample %d, tile %d, lane %d" % (i, i // 1024, i % 1024)


def _same_bytes(got, want, what):
    """Byte-identical arrays of one row per sample, or the first differing sample named."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() == want.tobytes():
        return
    rows = got.reshape(len(got), -1).view(np.uint8) != want.reshape(len(want), -1).view(np.uint8)
    i = int(np.flatnonzero(rows.any(axis=1))[0])
    pytest.fail("%s: %d samples differ, first at %s: %r against %r" % (what, int(rows.any(axis=1).sum()), _where(i), got[i], want[i]))


def _within(dev, want, gate, what):
    err = np.abs(dev.astype(np.complex128) - want)
    worst = float(err.max())
    print("%s: max |dev - ref| = %.3e, gate %.3e" % (what, worst, gate))
    if worst > gate:
        i = int(np.flatnonzero(err > gate)[0])
        pytest.fail("%s: %d samples beyond the gate %.3e, first at %s: %r against %r" % (what, int((err > gate).sum()), gate, _where(i), dev[i], want[i]))
    return worst


def _whole(gctx, scene, sigma=None, n=None, **kw):
    """One generate(n) into a ring that does not wrap, tables in HBM unless said otherwise; returns what the ring holds."""
    n = scene["n"] if n is None else n
    kw.setdefault("placement", "hbm")
    ring, gen = _generate(gctx, scene, [n], max(n + 11, 2000), scene["sigma"] if sigma is None else sigma, max_window=1000, **kw)
    got, info = ring.read(0, n), gen.output_info()
    gen.close()
    ring.close()
    return got, info


def _cut(gctx, scene, fmt=None, scale=None):
    """The scene's n samples in calls of 1, 1023, 1 and n - 1025 into a ring of 1537.  After every call the resident samples are
    read, so that what a later call evicts has been seen: returns (rows, covered, output_info) -- all n are covered unless the
    last call is longer than the ring (e5a), which evicts most of itself."""
    import gnsscorr
    n = scene["n"]
    fmt = gnsscorr.GC_IQ_F32 if fmt is None else fmt
    ring = gnsscorr.IqStream(gctx, capacity_samples=CUT_CAPACITY, max_window_samples=CUT_WINDOW, iq_format=fmt)
    if fmt != gnsscorr.GC_IQ_F32:
        ring.accept_quantised_output()
    gen = gnsscorr.SignalGenerator(gctx, ring, scene["fs"], scene["sats"], noise_sigma=scene["sigma"], seed=scene["seed"], t0=scene["t0"], table_placement="hbm")
    if scale is not None:
        gen.set_output_scale(scale)
    rows, covered, head = None, np.zeros(n, bool), 0
    for call in (1, 1023, 1, n - 1025):
        assert gen.generate(call) == head
        head += call
        first = max(0, head - CUT_CAPACITY)
        part = ring.read(first, head - first)
        if rows is None:
            rows = np.zeros((n,) + part.shape[1:], part.dtype)
        if covered[first:head].any():
            seen = covered[first:head]
            _same_bytes(part[seen], rows[first:head][seen], "%s: samples read again after a later call" % scene["name"])
        rows[first:head] = part
        covered[first:head] = True
    assert gen.info() == n and ring.info()[1] == n
    info = gen.output_info()
    gen.close()
    ring.close()
    return rows, covered, info


@pytest.fixture(scope="module")
def rows(gctx):
    """name -> (scene, the float ring's device samples of one uncut generate, the restatement): made once each, never changed."""
    import gnsscorr
    made = {}

    def get(name):
        if name not in made:
            scene = cases.scene_dict(gnsscorr, name)
            dev, _ = _whole(gctx, scene)
            want = ref.generate(scene["dicts"], scene["sigma"], scene["seed"], scene["t0"], scene["n"])
            for a in (dev, want):
                a.setflags(write=False)
            made[name] = (scene, dev, want)
        return made[name]
    return get


@pytest.fixture(scope="module")
def carrier_of_zero_is_exact(gctx):
    """The probe the exact test rests on: sample 0 of gps under Doppler 0, phase 0 and amplitude 1 is exactly its table entry times
    its symbol, i.e. the hardware's cos(0) is 1 and its sin(0) is 0."""
    import gnsscorr
    sats = cases.exact_variant(cases.matrix_scene(gnsscorr, "gps")[0])
    scene = cases.scene_dict(gnsscorr, "gps", sats=sats, sigma=0.0)
    dev, _ = _whole(gctx, scene, n=4)
    want = ref.generate(scene["dicts"], 0.0, scene["seed"], 0, 4).astype(np.complex64)
    exact = bool(dev[0] == want[0]) and abs(want[0]) == 1.0
    print("carrier probe: device sample 0 of gps is %r, the table entry times its symbol %r: %s" % (dev[0], want[0], "exact" if exact else "NOT exact"))
    return exact


@pytest.mark.parametrize("name", NAMES)
def test_parity_of_every_scene(rows, name):
    scene, dev, want = rows(name)
    assert dev.dtype == np.complex64 and dev.shape == (scene["n"],)
    _within(dev, want, _gate(scene, scene["sigma"]), "parity %s (A = %.4f, sigma = %.2f)" % (name, ref.amplitude_bound(scene["dicts"]), scene["sigma"]))
    assert np.abs(want).max() > 0.5 * ref.amplitude_bound(scene["dicts"]) / len(scene["dicts"]) ** 0.5  # the scene is not silence


@pytest.mark.parametrize("name", cases.SINGLE)
def test_exact_structure_under_a_carrier_of_one(gctx, carrier_of_zero_is_exact, name):
    """Doppler 0, carrier phase 0, amplitude 1, no noise: the sample IS table entry x gain x symbol x secondary symbol on its axis,
    so the table index, the symbols and the axis of every sample are pinned with no tolerance.  Should the probe find the
    hardware's cos(0) or sin(0) inexact, the parity gate stands in."""
    import gnsscorr
    sats = cases.exact_variant(cases.matrix_scene(gnsscorr, name)[0])
    scene = cases.scene_dict(gnsscorr, name, sats=sats, sigma=0.0)
    dev, _ = _whole(gctx, scene)
    want = ref.generate(scene["dicts"], 0.0, scene["seed"], 0, scene["n"])
    axes = [comp["axis"] for comp in scene["dicts"][0]["comps"]]
    assert np.any(want.real != 0.0) == (0 in axes) and np.any(want.imag != 0.0) == (1 in axes)
    if not carrier_of_zero_is_exact:
        _within(dev, want, _gate(scene, 0.0), "structure %s, gated" % name)
        return
    want = want.astype(np.complex64)
    if not np.array_equal(dev, want):
        i = int(np.flatnonzero(dev != want)[0])
        pytest.fail("structure %s: %d samples differ, first at %s: %r against %r" % (name, int((dev != want).sum()), _where(i), dev[i], want[i]))


@pytest.mark.parametrize("name", NAMES)
def test_cut_and_wrap_of_every_scene(gctx, rows, name):
    scene, dev, _ = rows(name)
    n = scene["n"]
    got, covered, _ = _cut(gctx, scene)
    assert covered[:1025].all() and covered[n - CUT_CAPACITY:].all() and (covered.all() or name == "e5a")
    _same_bytes(got[n - CUT_CAPACITY:], dev[n - CUT_CAPACITY:], "cut %s, the resident tail" % name)
    _same_bytes(got[covered], dev[covered], "cut %s, samples evicted before the end" % name)


@pytest.mark.parametrize("fmt_name", ["GC_IQ_I16", "GC_IQ_I8"])
@pytest.mark.parametrize("name", NAMES)
def test_integer_rings_of_every_scene(gctx, rows, name, fmt_name):
    """The strided run of the integer kernels against the consecutive run of the float kernel, cut and wrapped as above."""
    import gnsscorr
    fmt = getattr(gnsscorr, fmt_name)
    scene, dev, _ = rows(name)
    n = scene["n"]
    scale = cases.SCALES[name][fmt - 1]
    want, clipped = out_ref.quantise(dev, fmt, scale)
    got, covered, info = _cut(gctx, scene, fmt=fmt, scale=scale)
    print("%s %s: %d of %d components clipped at scale %g" % (name, fmt_name, info[2], 2 * n, scale))
    assert covered[:1025].all() and covered[n - CUT_CAPACITY:].all() and (covered.all() or name == "e5a")
    _same_bytes(got[covered], want[covered], "%s %s" % (fmt_name, name))
    assert info == (fmt, scale, clipped)
    assert 0 < clipped < 2 * n // 4


@pytest.mark.parametrize("name", ["mix_lds", "two_axes_small"])
def test_table_placement_changes_no_bit(gctx, rows, name):
    import gnsscorr
    scene, dev, _ = rows(name)
    for placement in ("lds", "auto"):
        got, _ = _whole(gctx, scene, placement=placement)
        _same_bytes(got, dev, "%s, float ring, tables %s against hbm" % (name, placement))
    scale = cases.SCALES[name][0]
    ints = {placement: _whole(gctx, scene, placement=placement, iq_format=gnsscorr.GC_IQ_I16, scale=scale) for placement in ("hbm", "lds", "auto")}
    for placement in ("lds", "auto"):
        _same_bytes(ints[placement][0], ints["hbm"][0], "%s, int16 ring, tables %s against hbm" % (name, placement))
        assert ints[placement][1] == ints["hbm"][1]
    _same_bytes(ints["hbm"][0], out_ref.quantise(dev, gnsscorr.GC_IQ_I16, scale)[0], "%s, int16 ring in one call" % name)


def test_tables_beyond_lds_are_refused_and_the_ring_stays_free(gctx, rows):
    import gnsscorr
    scene, dev, _ = rows("mix32")
    ring = gnsscorr.IqStream(gctx, capacity_samples=2048, max_window_samples=512)
    with pytest.raises(gnsscorr.GnsscorrError, match="do not fit in LDS") as e:
        gnsscorr.SignalGenerator(gctx, ring, scene["fs"], scene["sats"], noise_sigma=scene["sigma"], seed=scene["seed"], table_placement="lds")
    assert e.value.status == gnsscorr.GC_ERR_INVALID
    gen = gnsscorr.SignalGenerator(gctx, ring, scene["fs"], scene["sats"], noise_sigma=scene["sigma"], seed=scene["seed"], table_placement="hbm")
    assert gen.generate(1029) == 0
    _same_bytes(ring.read(0, 1029), dev[:1029], "mix32 on the ring the refused generator left")
    gen.close()
    ring.close()


@pytest.mark.parametrize("t0", cases.SAMPLE_NUMBER_EDGES)
def test_sample_numbers_at_the_carries(gctx, rows, t0):
    """mix_lds from a start whose sample numbers cross 2^32 (the Philox counter's high word, the carry of t x step), 2^63 or wrap
    2^64 inside the first tile: the float ring against the restatement, the int16 ring against the float ring.  The same samples
    in calls of 1, 1023, 1 and the rest put the carry at another place of a thread's run."""
    import gnsscorr
    scene, zero, _ = rows("mix_lds")
    n = cases.EDGE_N
    scene = dict(scene, t0=t0)
    dev, _ = _whole(gctx, scene, n=n, t0=t0)
    want = ref.generate(scene["dicts"], scene["sigma"], scene["seed"], t0, n)
    gate = _gate(scene, scene["sigma"])
    _within(dev, want, gate, "t0 = %d" % t0)
    assert np.max(np.abs(dev.astype(np.complex128) - zero[:n])) > 0.5 * ref.amplitude_bound(scene["dicts"])  # another stretch than the one from 0
    ring, gen = _generate(gctx, scene, [1, 1023, 1, n - 1025], n + 11, scene["sigma"], t0=t0, max_window=500, placement="hbm")
    _same_bytes(ring.read(0, n), dev, "t0 = %d, float ring in four calls" % t0)
    gen.close()
    ring.close()
    scale = cases.SCALES["mix_lds"][0]
    quantised, clipped = out_ref.quantise(dev, gnsscorr.GC_IQ_I16, scale)
    for calls in ([n], [1, 1023, 1, n - 1025]):
        ring, gen = _generate(gctx, scene, calls, n + 11, scene["sigma"], iq_format=gnsscorr.GC_IQ_I16, scale=scale, t0=t0, max_window=500, placement="hbm")
        _same_bytes(ring.read(0, n), quantised, "t0 = %d, int16 ring in calls of %r" % (t0, calls))
        assert gen.output_info() == (gnsscorr.GC_IQ_I16, scale, clipped)
        gen.close()
        ring.close()


@pytest.fixture(scope="module")
def mix32_without_noise(gctx):
    import gnsscorr
    scene = cases.scene_dict(gnsscorr, "mix32", sigma=0.0)
    dev, _ = _whole(gctx, scene)
    dev.setflags(write=False)
    return scene, dev


@pytest.mark.parametrize("s", [0, 15, 31])
def test_a_satellite_does_not_depend_on_its_neighbours(gctx, mix32_without_noise, s):
    """mix32 without noise, and the same 32 descriptors with every amplitude but that of satellite s at 0 -- s keeps its index,
    which its data symbols are a function of, and its place behind the other tables.  Satellite s on its own is its restatement,
    and the full scene less that is the restatement of the other 31, within the gate of those 31: a descriptor or a table read at
    the wrong index moves energy between satellites and shows in one or the other."""
    import gnsscorr
    scene, full = mix32_without_noise
    sats = cases.matrix_scene(gnsscorr, "mix32")[0]
    for i, sat in enumerate(sats):
        if i != s:
            sat.c.amplitude = 0.0
    alone_scene = cases.scene_dict(gnsscorr, "mix32", sats=sats, sigma=0.0)
    alone, _ = _whole(gctx, alone_scene)
    n = scene["n"]
    assert ref.amplitude_bound(alone_scene["dicts"]) == pytest.approx(ref.amplitude_bound([scene["dicts"][s]]))
    _within(alone, ref.satellite(scene["dicts"][s], s, scene["seed"], 0, n), _gate(alone_scene, 0.0), "mix32, satellite %d alone" % s)
    others = [dict(d, amplitude=0.0) if i == s else d for i, d in enumerate(scene["dicts"])]
    rest = full.astype(np.complex128) - alone.astype(np.complex128)
    err = np.abs(rest - ref.generate(others, 0.0, scene["seed"], 0, n))
    gate = 1e-5 * ref.amplitude_bound(others)
    print("mix32 less satellite %d: max |dev - ref| = %.3e, gate %.3e" % (s, float(err.max()), gate))
    assert err.max() <= gate, _where(int(np.flatnonzero(err > gate)[0]))
