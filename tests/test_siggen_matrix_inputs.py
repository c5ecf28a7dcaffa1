"""CPU tests (no GPU) that hold the signal generator's scene table (tests/siggen_cases.py, MATRIX) to its preconditions, on the numpy
restatement (tests/siggen_ref.py) alone: the events tests/test_siggen_matrix_gpu.py is about -- a data-symbol change, a sign change
of every secondary code, a code-period wrap inside a run of consecutive and of strided samples, the sample-number carries -- really
fall inside the samples it generates, and every satellite is large enough against the parity gate for one wrong sign to show.  So
the device test cannot pass vacuously.  The restatement's axis branch is held to an independent evaluation in Python integers."""
import cmath
import functools

import numpy as np
import pytest

import conditioner_out_ref as out_ref
import siggen_cases as cases
import siggen_ref as ref

NAMES = tuple(cases.MATRIX)


@functools.lru_cache(maxsize=None)
def _scene(name):
    """The row, and (k, f, e) of every satellite over the row's samples: computed once, never changed."""
    import gnsscorr
    scene = cases.scene_dict(gnsscorr, name)
    t = ref._times(scene["t0"], scene["n"])
    scene["phases"] = [ref.code_phase(d, t) for d in scene["dicts"]]
    return scene


def _components(scene):
    """(satellite index, component index, satellite dict, component dict, k of every sample) of every component of the scene."""
    for s, (d, (k, _, _)) in enumerate(zip(scene["dicts"], scene["phases"])):
        for c, comp in enumerate(d["comps"]):
            yield s, c, d, comp, k


def _is_e5a_i_of_a_short_scene(scene, d, c):
    """The I component of an E5a satellite in a scene of one code-period wrap: its symbol change and the sign change of its
    secondary code cannot share a boundary (siggen_cases.matrix_e5a), so it has one of the two; the e5a row, with two wraps, has both."""
    return scene["name"] == "mix32" and d["table_len"] == 10230 and c == 0


def _symbol_change(scene, s, c, comp, k):
    kk = k + np.uint64(comp["period_offset"])
    j = kk // np.uint64(comp["periods_per_symbol"])
    at = np.flatnonzero(j[1:] != j[:-1])
    sym = ref.symbols(scene["seed"], j, s, c)
    return len(np.unique(j)) >= 2 and any(sym[i] != sym[i + 1] for i in at)


def _secondary_sign_change(comp, k):
    sec = np.asarray(comp["secondary"], np.int64)
    idx = ((k + np.uint64(comp["period_offset"])) % np.uint64(len(sec))).astype(np.int64)
    at = np.flatnonzero(k[1:] != k[:-1])
    return any(sec[idx[i]] != sec[idx[i + 1]] for i in at)


@pytest.mark.parametrize("name", NAMES)
def test_every_data_component_changes_its_symbol(name):
    scene = _scene(name)
    seen = 0
    for s, c, d, comp, k in _components(scene):
        if comp["periods_per_symbol"] == 0 or name == "long_period":  # long_period is the scene without a wrap: one symbol
            continue
        seen += 1
        if _is_e5a_i_of_a_short_scene(scene, d, c):
            assert _symbol_change(scene, s, c, comp, k) or _secondary_sign_change(comp, k), (s, c)
        else:
            assert _symbol_change(scene, s, c, comp, k), (s, c)
    assert seen > 0 or name in ("q_only", "long_period")
    if name == "mix32":
        e5a_i = [(s, c, comp, k) for s, c, d, comp, k in _components(scene) if _is_e5a_i_of_a_short_scene(scene, d, c)]
        assert len(e5a_i) == 8
        assert sum(_symbol_change(scene, s, c, comp, k) for s, c, comp, k in e5a_i) == 4
        assert sum(_secondary_sign_change(comp, k) for s, c, comp, k in e5a_i) == 4


@pytest.mark.parametrize("name", NAMES)
def test_every_secondary_code_changes_sign_at_a_period_boundary(name):
    scene = _scene(name)
    for s, c, d, comp, k in _components(scene):
        if comp["secondary"] is None or _is_e5a_i_of_a_short_scene(scene, d, c):
            continue
        assert _secondary_sign_change(comp, k), (s, c)
    lens = sorted({len(comp["secondary"]) for _, _, _, comp, _ in _components(scene) if comp["secondary"] is not None})
    want = dict(e1=[25], e5a=[20, 100], two_axes_small=[3, 100], short_period=[5], very_short_period=[5], mix32=[20, 25, 100], mix_lds=[3, 100])
    assert lens == want.get(name, [])


@pytest.mark.parametrize("name", NAMES)
def test_period_wraps_fall_inside_the_runs_of_both_kernels(name):
    """Every satellite (not only one of the scene): a wrap between two of a thread's four consecutive float samples, and between
    its samples i and i + 256 of one tile of the integer kernels.  long_period has none, and reads another entry at every sample."""
    scene = _scene(name)
    n = scene["n"]
    i = np.arange(n - 1)
    strided = np.arange(n - 256)
    strided = strided[strided % 1024 < 768]
    for s, (k, _, e) in enumerate(scene["phases"]):
        if name == "long_period":
            assert len(np.unique(k)) == 1 and len(np.unique(e)) >= 1000
            continue
        assert np.any((k[1:] != k[:-1]) & (i % 4 < 3)), s
        assert np.any(k[strided] != k[strided + 256]), s


@pytest.mark.parametrize("name, periods_in_256", [("short_period", 69), ("very_short_period", 186)])
def test_short_periods_wrap_inside_a_run(name, periods_in_256):
    """Four consecutive samples span 3 / 3.7 of short_period's code period: one boundary at most, so the run with two boundaries
    is very_short_period's (every one of its runs has two or three)."""
    scene = _scene(name)
    k = scene["phases"][0][0]
    first = np.arange(0, scene["n"] - 3, 4)
    crossed = (k[first + 3] - k[first]).astype(np.int64)
    assert (int(crossed.min()), int(crossed.max())) == ((0, 1) if name == "short_period" else (2, 3))
    step = scene["dicts"][0]["code_step_q"]
    assert int(ref.mulhi(np.uint64(step), np.uint64(256))) == (step * 256) >> 64 == periods_in_256 and step > 1 << 56
    # and a symbol is refreshed at every place of a run: a wrap in front of each of the samples 4 i + 1, 4 i + 2, 4 i + 3
    i = np.arange(scene["n"] - 1)
    for r in range(3):
        assert np.any((k[1:] != k[:-1]) & (i % 4 == r))


def test_sample_number_edges_fall_inside_a_tile():
    for t0, carry in zip(cases.SAMPLE_NUMBER_EDGES, (1 << 32, 1 << 63, 1 << 64)):
        crossing = carry - t0  # the first sample at or beyond the carry
        assert 0 < crossing < cases.EDGE_N and crossing % 1024 != 0
    t = ref._times(cases.SAMPLE_NUMBER_EDGES[2], cases.EDGE_N)
    assert int(t[599]) == (1 << 64) - 1 and int(t[600]) == 0 and int(t[-1]) == cases.EDGE_N - 601  # the restatement's times wrap


def test_sample_number_edges_are_other_stretches_of_the_scene():
    """What test_siggen_matrix_gpu.py asserts of the device, here of the restatement: each edge's samples differ from those that
    start at 0 by more than half the amplitude bound."""
    scene = _scene("mix_lds")
    a = ref.amplitude_bound(scene["dicts"])
    zero = ref.generate(scene["dicts"], scene["sigma"], scene["seed"], 0, cases.EDGE_N)
    for t0 in cases.SAMPLE_NUMBER_EDGES:
        x = ref.generate(scene["dicts"], scene["sigma"], scene["seed"], t0, cases.EDGE_N)
        assert np.max(np.abs(x - zero)) > 0.5 * a


def test_table_sizes_on_both_sides_of_the_lds_limit():
    total = {name: sum(d["table_len"] * len(d["comps"]) for d in _scene(name)["dicts"]) for name in ("mix32", "mix_lds", "two_axes_small")}
    assert total == dict(mix32=8 * (1023 + 511 + 2 * 49104 + 2 * 10230), mix_lds=1023 + 511 + 2 * 4092 + 7, two_axes_small=2 * 4092)
    assert total["mix32"] > cases.LDS_FLOATS >= total["mix_lds"] > total["two_axes_small"]
    mix32 = _scene("mix32")
    assert len(mix32["sats"]) == 32 and [d["table_len"] for d in mix32["dicts"]] == [1023] * 8 + [511] * 8 + [49104] * 8 + [10230] * 8
    amplitudes = [d["amplitude"] for d in mix32["dicts"]]
    assert min(amplitudes) == pytest.approx(0.05) and max(amplitudes) == pytest.approx(0.2)
    for key in ("code_phase0_q", "carr_step_q", "carr_phase0_q"):
        assert len({d[key] for d in mix32["dicts"]}) == 32  # GLONASS: distinct channels, and every Doppler, phase and offset differs
    assert len({s.c.doppler_hz - (-4000.0 + 258.5 * i) for i, s in enumerate(mix32["sats"]) if 8 <= i < 16}) == 8


@pytest.mark.parametrize("name", NAMES)
def test_every_satellite_is_visible_to_the_gate(name):
    """One wrong sign on one component of one satellite moves a sample by 2 amplitude |gain| |table entry|: at least 20 gates."""
    scene = _scene(name)
    gate = 1e-5 * ref.amplitude_bound(scene["dicts"]) + 2e-5 * scene["sigma"]
    for s, d in enumerate(scene["dicts"]):
        least = min(abs(comp["gain"]) * float(np.min(np.abs(comp["table"]))) for comp in d["comps"])
        assert 2.0 * d["amplitude"] * least >= 20.0 * gate, (s, d["amplitude"], least, gate)


def test_the_rows_are_what_the_table_says():
    for name in NAMES:
        scene = _scene(name)
        assert (scene["n"], scene["t0"]) == (cases.E5A_N if name == "e5a" else cases.MATRIX_N, 0) and scene["n"] % 2 == 1 and scene["n"] % 1024 == 453
        assert (scene["sigma"] > 0.0) == name.startswith("mix")
    axes = {name: [[comp["axis"] for comp in d["comps"]] for d in _scene(name)["dicts"]] for name in NAMES}
    assert (axes["e5a"], axes["q_only"], axes["two_axes_small"], axes["short_period"]) == ([[0, 1]], [[1]], [[1, 0]], [[0, 1]])
    assert [d["table_len"] for name in cases.SINGLE for d in _scene(name)["dicts"]] == [1023, 511, 49104, 10230, 7, 4092, 2, 2, 49104]
    glo = _scene("glonass")["sats"][0]
    assert glo.c.doppler_hz == 562500.0 * -7 + 250.0
    e1 = _scene("e1")["dicts"][0]
    assert [comp["gain"] for comp in e1["comps"]] == [1.0, -1.0] and [comp["periods_per_symbol"] for comp in e1["comps"]] == [1, 0]
    q = _scene("q_only")["dicts"][0]["comps"][0]
    assert q["gain"] < 0.0 and not np.any(np.abs(q["table"]) == 1.0)
    e5a = _scene("e5a")
    assert len(np.unique(e5a["phases"][0][0])) == 3 and int(np.flatnonzero(np.diff(e5a["phases"][0][0].astype(np.int64)))[1]) + 1 >= e5a["n"] - 1537
    # the exact variant keeps every code word and turns the carrier into 1
    import gnsscorr
    for name in cases.SINGLE:
        sats = cases.exact_variant(cases.matrix_scene(gnsscorr, name)[0])
        d = ref.from_satellite(sats[0], _scene(name)["fs"])
        was = _scene(name)["dicts"][0]
        assert (d["code_step_q"], d["code_phase0_q"], d["carr_step_q"], d["carr_phase0_q"], d["amplitude"]) == (was["code_step_q"], was["code_phase0_q"], 0, 0, 1.0)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fmt", [out_ref.GC_IQ_I16, out_ref.GC_IQ_I8])
def test_the_scales_clip_some_components_and_fewer_than_a_quarter(name, fmt):
    scene = _scene(name)
    x = ref.generate(scene["dicts"], scene["sigma"], scene["seed"], 0, scene["n"]).astype(np.complex64)
    _, clipped = out_ref.quantise(x, fmt, cases.SCALES[name][fmt - 1])
    assert 0 < clipped < 2 * scene["n"] // 4, clipped


def _independent(d, s, seed, t):
    """Sample t of satellite d (index s) in Python integers and one complex exponential, the axis placed by hand."""
    t &= ref.M64
    u = d["code_phase0_q"] + t * d["code_step_q"]
    k, f = u >> 64, u & ref.M64
    e = (f * d["table_len"]) >> 64
    re = im = 0.0
    for c, comp in enumerate(d["comps"]):
        v = float(comp["table"][e]) * comp["gain"]
        kk = (k + comp["period_offset"]) & ref.M64
        if comp["periods_per_symbol"]:
            v *= float(ref.symbols(seed, np.array([kk // comp["periods_per_symbol"]], np.uint64), s, c)[0])
        if comp["secondary"] is not None:
            v *= int(comp["secondary"][kk % len(comp["secondary"])])
        if comp["axis"] == 1:
            im += v
        else:
            re += v
    theta = (d["carr_phase0_q"] + t * d["carr_step_q"]) & ref.M64
    return d["amplitude"] * complex(re, im) * cmath.exp(2j * cmath.pi * (theta / 2.0 ** 64))


@pytest.mark.parametrize("name", ["e5a", "q_only"])
def test_generate_equals_an_independent_evaluation(name):
    """About 20 sample numbers: the ends, both sides of every period wrap (where the symbols and secondary codes change), and a few
    in between.  A swapped axis would give j v for v: as far off as the sample is large."""
    scene = _scene(name)
    d, n = scene["dicts"][0], scene["n"]
    k = scene["phases"][0][0]
    wraps = [int(i) for i in np.flatnonzero(k[1:] != k[:-1])][:4]
    at = sorted({0, 1, 2, 3, 255, 256, 1023, 1024, n // 2, n - 2, n - 1} | {i + o for i in wraps for o in (0, 1, 2)})
    assert wraps and 15 <= len(at) <= 25
    x = ref.generate(scene["dicts"], 0.0, scene["seed"], 0, n)
    for i in at:
        want = _independent(d, 0, scene["seed"], i)
        assert abs(x[i] - want) <= 1e-12 and abs(want) > 0.05, (i, x[i], want)
    # and at the sample-number carries
    for t0 in cases.SAMPLE_NUMBER_EDGES:
        x = ref.generate(scene["dicts"], 0.0, scene["seed"], t0 + 500, 210)
        for i in (0, 12, 13, 14, 99, 100, 101, 199, 200, 201, 209):  # the carries are at 13, 100 and 200
            assert abs(x[i] - _independent(d, 0, scene["seed"], t0 + 500 + i)) <= 1e-12, (t0, i)
