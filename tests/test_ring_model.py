"""CPU tests (no GPU) of the host model of a ring's storage (tests/ring_model.py) and of the schedules the ring contract tests
commit (tests/ring_contract_cases.py): the model against the one-line definition of the layout in gc_stream.hip, and every
producer's schedule against the piece classes required of it."""
import numpy as np
import pytest

import resampler_ref
import ring_contract_cases as cases
import ring_model


def _by_definition(capacity, window, samples):
    """Sample a lives at a % capacity and, when that is < max_window, also at capacity + a % capacity: one sample at a time."""
    storage = np.zeros(capacity + window + ring_model.SLACK, samples.dtype)
    for a, v in enumerate(samples):
        p = a % capacity
        storage[p] = v
        if p < window:
            storage[capacity + p] = v
    return storage


@pytest.mark.parametrize("capacity, window", [(3001, 96), (64, 32), (101, 7), (20, 1), (3011, 96)])
def test_model_is_the_definition_on_random_schedules(capacity, window):
    rng = np.random.Generator(np.random.PCG64(capacity))
    for trial in range(6):
        calls = [int(n) for n in rng.integers(0, 2 * capacity + 2, 12)] + [1, capacity, capacity + 1]
        rng.shuffle(calls)
        x = (np.arange(sum(calls)) + 1).astype(np.int32)  # no sample is zero, no two are equal
        m = ring_model.RingModel(capacity, window, np.int32)
        first = 0
        for n in calls:
            m.append(x[first:first + n])
            first += n
            assert m.head == first
            assert np.array_equal(m.storage, _by_definition(capacity, window, x[:first])), (trial, n)
            assert not m.storage[capacity + window:].any()  # the slack
        assert m.calls == calls and sum(n for _, n in m.pieces) == len(x)
        assert all(n > 0 and pos + n <= capacity for pos, n in m.pieces)


def _by_definition_from(capacity, window, origin, samples):
    """The same with sample number origin + i for samples[i]: Python integers, one sample at a time."""
    storage = np.zeros(capacity + window + ring_model.SLACK, samples.dtype)
    for i, v in enumerate(samples):
        p = (origin + i) % capacity
        storage[p] = v
        if p < window:
            storage[capacity + p] = v
    return storage


@pytest.mark.parametrize("origin", [0, 1, 3000, (1 << 31) - 49, (1 << 32) - 1501, (1 << 40) + 12345, (1 << 53) + 1, 1 << 62])
@pytest.mark.parametrize("capacity, window", [(3001, 96), (101, 7), (20, 1)])
def test_model_with_an_origin_is_the_definition(capacity, window, origin):
    """Positions, mirror parts and the resident range of pushes that start at an origin, on schedules that wrap the ring more than
    twice behind it."""
    rng = np.random.Generator(np.random.PCG64(capacity + origin % 1000))
    calls = [int(n) for n in rng.integers(0, capacity + 1, 10)] + [1, capacity, capacity - 1]
    rng.shuffle(calls)
    assert sum(calls) > 2 * capacity
    x = (np.arange(sum(calls)) + 1).astype(np.int32)
    m = ring_model.RingModel(capacity, window, np.int32, origin=origin)
    assert m.resident() == (origin, origin) and not m.storage.any()
    first = 0
    for n in calls:
        at = len(m.pieces)
        m.append(x[first:first + n])
        if n:
            assert m.pieces[at][0] == (origin + first) % capacity == m.position(origin + first)
        first += n
        assert isinstance(m.head, int) and m.head == origin + first
        assert m.resident() == (max(origin, origin + first - capacity), origin + first)
        assert np.array_equal(m.storage, _by_definition_from(capacity, window, origin, x[:first])), n
        assert not m.storage[capacity + window:].any()
    assert sum(n for _, n in m.pieces) == len(x) and all(n > 0 and pos + n <= capacity for pos, n in m.pieces)
    # a ring at origin 0 that first receives origin % capacity other samples holds the later ones at the same positions
    lead = origin % capacity
    twin = ring_model.RingModel(capacity, window, np.int32)
    twin.append(np.full(lead, -7, np.int32))
    twin.append(x)
    assert twin.head - lead == m.head - origin
    keep = min(len(x), capacity)  # the newest `keep` samples are resident in both
    for i in range(len(x) - keep, len(x)):
        assert m.position(origin + i) == twin.position(lead + i)
    assert np.array_equal(twin.storage, m.storage)  # more than a ring's worth was appended: nothing of the lead is left


def test_two_component_samples_and_the_first_difference():
    m = ring_model.RingModel(10, 4, np.int16, per=2)
    x = np.arange(1, 27, dtype=np.int16).reshape(13, 2)
    m.append(x)
    assert m.pieces == [(0, 10), (0, 3)] and m.storage.shape == (16, 2)
    assert np.array_equal(m.storage[:3], x[10:]) and np.array_equal(m.storage[10:13], x[10:]) and np.array_equal(m.storage[3:10], x[3:10])
    assert np.array_equal(m.storage[13], x[3]) and not m.storage[14:].any()
    assert m.first_difference(m.storage.copy()) is None
    for p, region in ((2, "ring"), (9, "ring"), (10, "mirror"), (13, "mirror"), (14, "slack"), (15, "slack")):
        got = m.storage.copy()
        got[15, 1] ^= 1
        got[p, 1] ^= 0x100  # one bit of one byte
        assert m.first_difference(got)[:2] == (p, region)


def _reached(name, increments, capacity=cases.CAPACITY, tile=None):
    got = cases.classes(increments, capacity, cases.WINDOW, cases.TILE[name.split("-")[0]] if tile is None else tile)
    missing = cases.REQUIRED[name] - got
    assert not missing, "%s: the schedule does not reach %s" % (name, sorted(missing))
    return got


def test_the_output_schedules_reach_their_classes():
    assert cases.heads(cases.INCREMENTS)[-1] == cases.heads(cases.INCREMENTS_NO_G)[-1] == 15625
    assert cases.CAPACITY % 2 == 1 and 2 * cases.WINDOW <= cases.CAPACITY
    assert _reached("host", cases.INCREMENTS_NO_G) == cases.ALL - {"G"}
    assert _reached("siggen", cases.INCREMENTS) == cases.ALL
    for name in ("decimator", "resampler-down", "resampler-up", "resampler-polyphase"):
        _reached(name, cases.INCREMENTS)
    assert "G" not in _reached("conditioner", cases.INCREMENTS_NO_G)
    assert max(cases.INCREMENTS_NO_G) <= cases.CAPACITY and max(cases.INCREMENTS_2BIT) <= cases.CAPACITY


@pytest.mark.parametrize("D", [1, 3])
def test_fir_stages_reach_the_output_heads(D):
    """Conditioner and ring decimator: ceil(raw / D) outputs; the committed raw counts give the committed heads."""
    want = cases.heads(cases.INCREMENTS)
    raw = cases.fir_raw_heads(want, D)
    assert cases.fir_out_heads(raw, D) == want and all(b > a for a, b in zip(raw, raw[1:]))


def test_two_bit_schedule():
    """Whole bytes per push: every raw head is a multiple of 4 and still makes the committed heads at D = 3."""
    want = cases.heads(cases.INCREMENTS_2BIT)
    raw = cases.fir_raw_heads(want, 3, multiple=4)
    assert all(r % 4 == 0 for r in raw) and cases.fir_out_heads(raw, 3) == want
    _reached("conditioner-2bit", cases.INCREMENTS_2BIT, tile=cases.TILE["conditioner"])
    with pytest.raises(AssertionError):
        cases.fir_raw_heads([3001], 3, multiple=4)  # why the shared schedule does not serve this format


@pytest.mark.parametrize("name, pair", [("resampler-down", cases.DIRECT_DOWN), ("resampler-up", cases.DIRECT_UP), ("resampler-polyphase", cases.POLYPHASE[:2])])
def test_resampler_source_heads_complete_exactly_the_output_heads(name, pair):
    """An up-ratio completes one or two outputs per source sample, so not every head exists: the committed pair reaches all of them."""
    kind, step = resampler_ref.poly_ratio(*pair) if name == "resampler-polyphase" else resampler_ref.direct_ratio(*pair)
    want = cases.heads(cases.INCREMENTS)
    src = cases.source_heads(lambda h: resampler_ref.available(kind, step, h), want)
    assert [resampler_ref.available(kind, step, h) for h in src] == want
    assert all(b > a for a, b in zip(src, src[1:])) and src[-1] < (1 << 16)  # fits the source ring of the GPU test unwrapped
    _reached(name, np.diff([0] + [resampler_ref.available(kind, step, h) for h in src]).tolist())
    if name == "resampler-up":
        kind2, step2 = resampler_ref.direct_ratio(2.5e6, 6.625e6)
        with pytest.raises(AssertionError):
            cases.source_heads(lambda h: resampler_ref.available(kind2, step2, h), want)  # two or three outputs per source sample


@pytest.mark.parametrize("L", [32, 33])
def test_segment_schedules(L):
    """The notch stage: whole segments of L outputs per update, floor(source head / L) of them."""
    capacity = cases.SEGMENT_CAPACITY[L]
    assert capacity % 2 == 1 and capacity % L != 0
    src = cases.segment_raw_heads(cases.SEGMENTS[L], L)
    out = [h // L * L for h in src]
    assert out == [L * s for s in cases.heads(cases.SEGMENTS[L])] and src[-1] <= 16384
    got = _reached("notch-%d" % L, np.diff([0] + out).tolist(), capacity=capacity)
    assert not got & {"F_window-1", "F_window"}
    if L == 33:
        # why this case has a capacity of its own: on 3001 the wrap cuts its segments at even positions only
        assert not {"B", "E"} & cases.classes([L * s for s in cases.SEGMENTS[33]], 3001, cases.WINDOW, 256)


def test_blanking_schedule():
    """Pulse blanking at D = 1 and L = 32 appends whole segments, at most capacity outputs per push."""
    L = 32
    src = cases.segment_raw_heads(cases.SEGMENTS_NO_G_32, L)
    out = cases.fir_out_heads(src, 1, segment=L)
    assert out == [L * s for s in cases.heads(cases.SEGMENTS_NO_G_32)] and out[-1] == L * sum(cases.SEGMENTS[32])
    inc = np.diff([0] + out).tolist()
    assert max(inc) <= cases.CAPACITY
    _reached("conditioner-blanking", inc, tile=cases.TILE["conditioner"])


@pytest.mark.parametrize("compute_units", [256, 304, 64])
def test_tile_pushes(compute_units):
    capacity, window, pushes, n2, n4 = cases.tile_pushes(2 * compute_units)
    m = ring_model.RingModel(capacity, window, np.int8)
    for n in pushes:
        assert 0 < n <= capacity
        m.append(np.zeros(n, np.int8))
    at = {n: sorted(pos for pos, k in m.pieces if k == n) for n in (n2, n4)}
    for n in (n2, n4):
        assert len(at[n]) == 2 and at[n][0] == 0 and at[n][1] % 2 == 1 and at[n][1] >= window, at
    assert capacity == 301 + n4 and window == 128 and m.pieces == list(zip([p for p, _ in m.pieces], pushes))  # no push is cut
