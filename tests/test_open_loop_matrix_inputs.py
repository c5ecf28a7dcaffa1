"""CPU check of the open-loop matrix's inputs (tests/open_loop_matrix_cases.py).  The matrix compares every instantiation of
trk_multicorrelator_kernel with a float64 restatement at the fuzz test's bar, which only means something while
* the matrix launches every instantiation a caller can reach (read from the headers, not restated here);
* the restatement is the reference's arithmetic: against the compiled oracle it stays inside the same bar, by a wide margin;
* the bar is small against one sample: a stray, missing or wrongly signed sample then misses it by an order of magnitude;
* every window takes the branch of trk_epoch / trk_loop it is in the table for (computed from the record with the kernel's formulas)."""
import numpy as np
import pytest

import open_loop_matrix_cases as M


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    return M.build_selftest(tmp_path_factory.mktemp("open_loop_matrix"))


def test_matrix_keys_are_the_reachable_instantiations(selftest):
    want, have = M.reachable(selftest), M.matrix_keys()
    assert len(want) == 88
    assert have == want, "never launched: %s; not reachable: %s" % (sorted(want - have), sorted(have - want))


def test_restatement_agrees_with_the_compiled_oracle(oracle):
    worst = {}
    for launch in M.all_float_launches(oracle):
        ref, orc, bar = M.reference(oracle, launch), M.compiled(oracle, launch), M.bars(oracle, launch)
        for ch, recs in enumerate(launch.recs):
            for k, r in enumerate(recs):
                err = float(np.max(np.abs(orc[ch][k] - ref[ch][k])))
                assert err <= bar[ch][k], (launch.table, launch.mode, launch.fmt, launch.n_taps, ch, k, r.n, err, bar[ch][k])
                if r.n:
                    key = (launch.mode, launch.fmt)
                    worst[key] = max(worst.get(key, 0.0), err / bar[ch][k])
    for key in sorted(worst):
        print("oracle against restatement, worst error / bar, %-12s %s: %.3f" % (key + (worst[key],)))
    assert set(worst) == {(m, f) for m, f in M.BATCH if m != "sc16"} | {("hd_resampler", "f32")}


def test_a_sample_is_ten_bars(oracle):
    """bar <= 0.1 median |x| over the window, for every window of two samples and more."""
    for launch in M.all_float_launches(oracle):
        clean = M.samples(oracle, launch.stream, launch.fmt, launch.mode in M.HD)[1]
        bar = M.bars(oracle, launch)
        for ch, recs in enumerate(launch.recs):
            for k, r in enumerate(recs):
                if r.n >= 2:
                    first = launch.binds[ch] + r.offset
                    med = float(np.median(np.abs(clean[first:first + r.n])))
                    assert bar[ch][k] <= 0.1 * med, (launch.table, launch.mode, launch.fmt, launch.n_taps, ch, k, r.n, bar[ch][k], med)


def test_16bit_inputs_never_saturate_a_running_sum(oracle):
    """The device sums in 32 bits and saturates once; the reference saturates its running sum.  They are the same number while no
    running sum leaves the int16 range, which these inputs are scaled for."""
    launches = [M.matrix_launch(oracle, "sc16", "i16", t) for t in M.TAPS] + [M.resync_launch(oracle, "sc16", "i16")]
    launches += [M.level1_call(oracle, "sc16", t, n) for t in M.TAPS for n in M.LEVEL1_N]
    for launch in launches:
        out, exact = M.compiled(oracle, launch)
        assert np.array_equal(out.astype(np.int32), exact), (launch.table, launch.n_taps)
    q = M.samples(oracle, "clean", "sc16")[0]
    assert 40 < np.abs(q.astype(np.int32)).max() < 200


def test_quantised_streams_use_their_range(oracle):
    for stream in ("matrix", "clean"):
        q16, q8 = M.samples(oracle, stream, "i16")[1], M.samples(oracle, stream, "i8")[1]
        assert 600 < np.abs(q16.view(np.float32)).max() < 32767
        assert np.abs(q8.view(np.float32)).max() <= 127 and np.mean(np.abs(q8.view(np.float32)) == 127) < 1e-4
    # poison everywhere outside the windows, none inside
    for hd in (False, True):
        q = M.samples(oracle, "matrix", "f32", hd)[0]
        inside = M._inside(hd)
        assert np.all(np.isfinite(q[inside])) and not np.any(np.isfinite(q[~inside]).all(axis=1))
        assert inside.sum() == sum(M.n_of(n, tag, "hd_full" if hd else "plain") for _, n, _, tag in M.WINDOWS)  # the windows are disjoint
        q = M.samples(oracle, "matrix", "i8", hd)[0]
        assert np.all(np.abs(q[~inside].astype(np.int32)) == 127)


def _rows(launch):
    """(channel, epoch, WINDOWS row) of the matrix launch."""
    k = [0, 0]
    for row in M.WINDOWS:
        yield row[0], k[row[0]], row
        k[row[0]] += 1


@pytest.mark.parametrize("mode", ["plain", "hd_full", "complex"])
def test_every_matrix_window_takes_its_branch(oracle, selftest, mode):
    for n_taps in M.TAPS:
        launch = M.matrix_launch(oracle, mode, "f32", n_taps)
        assert [len(r) for r in launch.recs] == [11, 11]
        words = 2 if mode == "complex" else 1
        for n_slices in M.SLICINGS:
            got_slices, lds = M.plan(selftest, launch, n_slices)
            assert (got_slices, lds) == (n_slices, words * (1023 + M.LDS_MARGIN))  # windows below 4096 samples: the whole table's worth of LDS
            seen = set()
            for ch, k, (_, n, res, tag) in _rows(launch):
                r = launch.recs[ch][k]
                p = M.epoch_path(launch, ch, k, n_slices, lds)
                n_full = sum(p["full"])
                assert p["a"] == res and r.n == M.n_of(n, tag, mode)
                whole = p["lc0"] == 0 and p["lc1"] == p["n_chunks"]  # both ragged ends may be fetched as whole chunks
                if tag == "empty":
                    assert r.n == 0 and res % 2 == 1 and p["n_chunks"] == 1 and n_full == 0
                elif tag == "tiny":
                    assert p["n_chunks"] == 1 and n_full == 0 and whole
                elif tag == "edge":
                    assert (p["n_chunks"], n_full) == M.EDGE_CHUNKS[n, res] and whole
                    if n_slices == 3 and p["n_chunks"] == 2:
                        assert [s[2] == "none" for s in p["slices"]] == [False, False, True]  # an empty third slice
                    seen.add((n, res))
                elif tag == "aligned":
                    assert res == 0 and p["full"] == [True] * 4 and whole
                elif tag == "odd":
                    assert res % 2 == 1 and p["full"] == [False, True, True, True, False] and whole
                elif tag in ("ragged", "fast", "first", "last"):
                    # head, chunks 1..4 full, tail (2597 + a < 6 * 512: a ragged head leaves four full chunks, not five: two pairs through
                    # the queue.  Its odd leftover: the "odd" window, the 3-slice cut -- head + one full chunk, one full chunk + tail --
                    # and the 513-sample window at an aligned start)
                    assert res % 2 == 1 and p["full"] == [False, True, True, True, True, False]
                    if n_slices == 3:
                        assert [s[:2] for s in p["slices"]] == [(0, 2), (2, 4), (4, 6)]
                    if tag == "first":
                        assert r.offset == 0 and p["lc0"] == 1 and p["lc1"] == 6  # head: load_masked
                    elif tag == "last":
                        assert r.offset + r.n == launch.n_iq[ch] and p["lc0"] == 0 and p["lc1"] == 5  # tail: load_masked
                    else:
                        assert whole
                    if tag == "fast" and mode != "hd_full":
                        # one slice: more chips than the LDS holds, the modulo path on the whole table; three: windows again
                        assert [s[2] for s in p["slices"]] == (["lds_table"] if n_slices == 1 else ["window"] * 3)
                if tag != "fast" and r.n:
                    assert all(s[2] in ("window", "none") for s in p["slices"]), (tag, p)
                if mode in M.HD and r.n:
                    assert max(M.tap_delays(launch.shifts, r.params.code_phase_step_chips)) < r.n
            assert seen == set(M.EDGE_CHUNKS)
    # every record of a channel differs from every other in each of the four scalars
    for recs in M.matrix_records(oracle, mode):
        for name in ("rem_carr", "pstep", "rem_code", "cstep"):
            assert len({r.args[name] for r in recs}) == len(recs)


def test_resync_window_passes_the_64th_chunk(oracle, selftest):
    for mode, fmt in M.RESYNC:
        launch = M.resync_launch(oracle, mode, fmt)
        assert M.plan(selftest, launch, 1)[0] == 1
        p = M.epoch_path(launch, 0, 0, 1, M.plan(selftest, launch, 1)[1])
        # head, then the interior loop re-evaluates the rotators at chunk 64 of 67
        assert p["a"] == 1 and p["n_chunks"] == 67 and p["full"] == [False] + [True] * 65 + [False] and p["slices"] == [(0, 67, "lds_table")]
        assert abs(launch.recs[0][0].args["pstep"] - 1.3) < 1e-6


def test_table_path_launch_has_less_lds_than_the_table(oracle, selftest):
    for mode, fmt, n_taps in M.TABLE_PATHS:
        launch = M.table_launch(oracle, mode, fmt, n_taps)
        words = 2 if mode == "complex" else 1
        n_slices, lds = M.plan(selftest, launch, 2)
        L = M.TABLE_L[mode]
        assert words * (L + M.LDS_MARGIN) <= M.LDS_TABLE_FLOATS  # a batch accepts the code
        assert n_slices == 2 and lds < words * L, (mode, n_taps, lds)
        tables = [[s[2] for s in M.epoch_path(launch, 0, k, 2, lds)["slices"]] for k in range(3)]
        assert tables == [["window"] * 2, ["global_table"] * 2, ["global_table"] * 2], (mode, n_taps, tables)
        r = launch.recs[0]
        assert r[2].n * r[2].params.code_phase_step_chips > 3 * L and r[2].args["rem_code"] > 0  # several periods, from a negative chip


def test_tiny_code_window_wraps_more_than_twice(oracle, selftest):
    for mode, fmt in M.TINY:
        launch = M.tiny_launch(oracle, mode, fmt)
        lds = M.plan(selftest, launch, 1)[1]
        assert lds == (2 if mode == "complex" else 1) * (M.TINY_L + M.LDS_MARGIN)
        assert [M.epoch_path(launch, 0, k, 1, lds)["slices"][0][2] for k in range(2)] == ["window_mod", "window"]


def test_level1_calls_start_on_an_odd_sample(oracle):
    for mode in M.LEVEL1_MODES:
        for n in M.LEVEL1_N:
            launch = M.level1_call(oracle, mode, 3, n)
            p = M.epoch_path(launch, 0, 0, 1, 1023 + M.LDS_MARGIN, align=2)
            assert p["a"] == 1 and p["n_chunks"] == (2 if n == 513 else 6)
