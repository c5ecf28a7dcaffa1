"""CPU tests (no GPU) of the restatements that take a source with an origin (resampler_ref.direct_from / polyphase_from,
conditioner_ref.decimate_from) and of the case table of the origin tests (tests/ring_origin_cases.py).

A long run at small indices is sliced: the variant given (k, samples[k:]) must return the existing function's outputs from the
first whole-window output on -- the same samples moved, the same float64 sums -- for several k, multiples of the decimation and
not.  At large origins, where no long run exists, the variant is held against a direct evaluation in Python integers."""
import numpy as np
import pytest

import conditioner_ref
import resampler_ref
import ring_origin_cases as cases

ORIGINS = (0, 1, 2, 3, 7, 64, 333, 1000, 1001, 4099)


def _raw(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)


@pytest.mark.parametrize("D, T", [(1, 1), (3, 7), (4, 33), (5, 2), (7, 300)])
def test_decimator_from_an_origin_is_a_slice_of_the_long_run(D, T):
    raw = _raw(6000, 1)
    taps = np.random.Generator(np.random.PCG64(2)).standard_normal(T).astype(np.float32)
    whole = conditioner_ref.condition(raw, taps, D, 0.0, 1.0)
    for k in ORIGINS:
        m0, y = conditioner_ref.decimate_from(k, raw[k:], taps, D)
        assert m0 * D - (T - 1) >= k and (m0 == 0 or (m0 - 1) * D - (T - 1) < k)
        assert m0 + len(y) == len(whole) and len(y) > 0
        if k == 0 and T > 1:
            # outputs whose window reaches in front of sample 0 belong to a ring at origin 0 alone
            assert m0 == -(-(T - 1) // D) > 0
        assert np.array_equal(y, whole[m0:]), (k, m0)
        # a head in the middle of the run: the outputs it completes, no more
        head = k + (len(raw) - k) // 2
        m0h, yh = conditioner_ref.decimate_from(k, raw[k:], taps, D, head=head)
        assert m0h == m0 and m0 + len(yh) == max(m0, -(-head // D)) and np.array_equal(yh, whole[m0:m0 + len(yh)])


@pytest.mark.parametrize("fs_in, fs_out", [(25e6, 10e6), (4e6, 5e6), (2.5e6, 6.625e6), (4e6, 4e6), (16e6, 2.048e6)])
def test_direct_resampler_from_an_origin_is_a_slice_of_the_long_run(fs_in, fs_out):
    raw = _raw(6000, 3)
    kind, step = resampler_ref.direct_ratio(fs_in, fs_out)
    whole = resampler_ref.direct(raw, fs_in, fs_out)
    for k in ORIGINS:
        m0, y = resampler_ref.direct_from(k, raw[k:], fs_in, fs_out)
        n = resampler_ref.source_index(kind, step, [m0, max(m0 - 1, 0)])
        assert n[0] >= k and (m0 == 0 or n[1] < k)
        assert m0 + len(y) == len(whole) and y.tobytes() == whole[m0:].tobytes(), (k, m0)
        head = k + (len(raw) - k) // 3
        m0h, yh = resampler_ref.direct_from(k, raw[k:], fs_in, fs_out, head=head)
        assert m0h == m0 and m0 + len(yh) == max(m0, resampler_ref.available(kind, step, head)) and yh.tobytes() == whole[m0:m0 + len(yh)].tobytes()


@pytest.mark.parametrize("fs_in, fs_out, P, T", [(25e6, 10e6, 32, 11), (4e6, 5e6, 16, 6), (16e6, 2.048e6, 8, 24)])
def test_polyphase_resampler_from_an_origin_is_a_slice_of_the_long_run(fs_in, fs_out, P, T):
    raw = _raw(6000, 4)
    bank = np.random.Generator(np.random.PCG64(5)).standard_normal((P, T)).astype(np.float32)
    kind, inc = resampler_ref.poly_ratio(fs_in, fs_out)
    whole = resampler_ref.polyphase(raw, bank, fs_in, fs_out)
    for k in ORIGINS:
        m0, y = resampler_ref.polyphase_from(k, raw[k:], bank, fs_in, fs_out)
        n = resampler_ref.source_index(kind, inc, [m0, max(m0 - 1, 0)])
        assert n[0] - (T - 1) >= k and (m0 == 0 or n[1] - (T - 1) < k)
        assert m0 + len(y) == len(whole) and np.array_equal(y, whole[m0:]), (k, m0)


@pytest.mark.parametrize("origin", [(1 << 32) - 1501, (1 << 40) + 12345, (1 << 53) + 1])
def test_the_variants_at_large_origins_against_python_integers(origin):
    raw = _raw(500, 6)
    # direct, down: sample by sample
    for fs_in, fs_out in ((25e6, 10e6), (4e6, 5e6), (4e6, 4e6)):
        kind, step = resampler_ref.direct_ratio(fs_in, fs_out)
        m0, y = resampler_ref.direct_from(origin, raw, fs_in, fs_out)
        assert isinstance(m0, int) and len(y) > 100
        for j in (0, 1, len(y) // 2, len(y) - 1):
            m = m0 + j
            n = -((-m * resampler_ref.M) // step) if kind == resampler_ref.DOWN else ((m + 1) * step) // resampler_ref.M if kind == resampler_ref.UP else m
            assert y[j] == raw[n - origin]
        assert m0 == 0 or resampler_ref._exact_source_index(kind, step, [m0 - 1])[0] < origin
    D, T = 3, 7
    taps = np.arange(1, T + 1, dtype=np.float32)
    m0, y = conditioner_ref.decimate_from(origin, raw, taps, D)
    assert m0 == (origin + T - 1 + D - 1) // D and m0 * D - (T - 1) >= origin > (m0 - 1) * D - (T - 1)
    for j in (0, len(y) - 1):
        want = sum(float(taps[k]) * complex(raw[(m0 + j) * D - k - origin]) for k in range(T))
        assert abs(y[j] - want) <= 1e-12 * abs(want)
    assert m0 + len(y) == -(-(origin + len(raw)) // D)


def test_the_case_table_keeps_its_own_conditions():
    """What tests/ring_origin_cases.py asserts about itself at import, once more where a failure is a test's."""
    cases.check()
    assert len(cases.ORIGIN_NAMES) == 4
