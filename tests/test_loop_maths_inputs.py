"""CPU check of the loop-maths matrix's inputs (tests/loop_maths_cases.py): every channel of tests/test_loop_maths_gpu.py through the
restatement alone, held to the preconditions the GPU test leans on -- a channel that drifted off its branch would test nothing there --
and the replay run on the restatement's own records, where it must reproduce everything with no libm shift at all."""
import numpy as np
import pytest

import loop_maths_cases as L

CASES = [(taps, c["name"]) for taps in (3, 5) for c in L.channels(taps)]


def _ids(v):
    return str(v)


def test_the_table_is_the_matrix():
    for taps in (3, 5):
        ch = L.channels(taps)
        assert [sum(c["group"] == g for c in ch) for g in "ABCD"] == [24, 8, 2, 1]
        assert len({c["name"] for c in ch}) == len(ch)
        a = {(c["conf"]["dll_filter_order"], c["conf"]["pll_filter_order"], c["conf"]["enable_fll_pull_in"], c["conf"]["enable_fll_steady_state"])
            for c in ch if c["group"] == "A"}
        assert a == {(d, p, i, s) for d in (1, 2, 3) for p in (2, 3) for i in (0, 1) for s in (0, 1)}
        for c in ch:
            if c["group"] == "B":
                y, k = c["sync"], c["conf"]
                assert y["extend_correlation_symbols"] == 3 and y["symbols_per_bit"] == 1
                assert y["pll_bw_narrow_hz"] != k["pll_bw_hz"] and y["dll_bw_narrow_hz"] != k["dll_bw_hz"] and y["early_late_space_narrow_chips"] != k["early_late_space_chips"]
                assert taps == 3 or y["very_early_late_space_narrow_chips"] != k["very_early_late_space_chips"]
            # a plain engine's channels share the pilot mode
            assert (c["engine"] == "pilot") == bool(c["sync"] and c["sync"]["track_pilot"])


@pytest.mark.parametrize("taps,name", CASES, ids=_ids)
def test_channel_meets_its_preconditions(oracle, taps, name):
    c = next(c for c in L.channels(taps) if c["name"] == name)
    ref = L.reference(oracle, taps, name)
    group, conf = c["group"], c["conf"]
    assert len(ref) == L.N_EP and all(r["valid"] == 1 for r in ref)
    states = [r["state"] for r in ref]  # after each period
    ext = c["sync"]["extend_correlation_symbols"] if c["sync"] else 1
    if group in "AD":
        assert set(states) == {2} and not any(r["integrating"] for r in ref)
    elif ext == 1:
        assert ref[0]["state_in"] == 2 and set(states) == {4}
    else:
        # wide for one period, then ext - 1 integrating periods and a loop update, over and over
        assert ref[0]["state_in"] == 2 and states == [([3] * (ext - 1) + [4])[k % ext] for k in range(L.N_EP)]
        assert [r["integrating"] for r in ref[1:]] == [int((k % ext) != ext - 1) for k in range(L.N_EP - 1)]
    # the pull-in transitory ends inside the run, with room on both sides
    first_after = [r["pull_in"] for r in ref].index(False)
    assert 24 <= first_after <= 48 and all(r["pull_in"] for r in ref[:first_after]) and not any(r["pull_in"] for r in ref[first_after:])
    # block length floor(K): K never within 1e-3 samples of a whole one (the closed-loop matrix's rule)
    margin = min(min(r["rem_code_samples"], 1.0 - r["rem_code_samples"]) for r in ref)
    assert margin >= 1e-3, margin
    updates = [r for r in ref if not r["integrating"]]
    if group == "D":
        # zeros in, so the discriminators are 0 and the filters' outputs constant by construction: this channel is about the branches
        assert all(np.all(r["corr"] == 0) for r in ref) and all(r["perr"] == 0.0 and r["cerr"] == 0.0 for r in ref)
        assert all(np.isnan(r["cn0"]) and np.isnan(r["lock_test"]) for r in ref[11:])
    else:
        assert abs(ref[-1]["doppler"] - L.SIGNALS[taps][1]) <= 3.0, ref[-1]["doppler"]
        assert len({r["cfilt"] for r in updates}) > len(updates) // 2 and len({r["doppler"] for r in updates}) > len(updates) // 2
        prompt = np.mean([abs(r["accu"][2]) for r in updates[-8:]])
        assert prompt >= 0.5 * ext * L.M.AMP * L.N, prompt  # on the peak
    # the FLL's three call shapes
    fll = [(r["pull_in"] and conf["enable_fll_pull_in"], conf["enable_fll_steady_state"]) for r in updates]
    if conf["enable_fll_pull_in"]:
        assert sum(1 for p, s in fll if p) >= 20
    if conf["enable_fll_steady_state"]:
        assert sum(1 for p, s in fll if s and not p) >= 10
    if not conf["enable_fll_steady_state"]:
        assert sum(1 for p, s in fll if not p) >= 10


def test_every_filter_order_is_met_before_and_after_a_redesign(oracle):
    for taps in (3, 5):
        before, after = set(), set()
        for c in L.channels(taps):
            if not (c["sync"] and c["sync"]["extend_correlation_symbols"] > 1):
                continue
            ref = L.reference(oracle, taps, c["name"])
            orders = (c["conf"]["dll_filter_order"], c["conf"]["pll_filter_order"])
            if any(r["state_in"] == 2 and not r["integrating"] for r in ref):
                before.add(orders)
            if sum(1 for r in ref if r["state_in"] == 4) >= 20:
                after.add(orders)
        for seen in (before, after):
            assert {d for d, p in seen} == {1, 2, 3} and {p for d, p in seen} == {2, 3}, (taps, seen)


def test_replay_reproduces_the_restatement_without_any_shift(oracle):
    """The replay of tests/test_loop_maths_gpu.py on records made from the restatement's own output: every stage exact, every libm
    distance 0, and every branch of the coverage count met."""
    total = dict.fromkeys(L.BRANCHES, 0)
    for taps in (3, 5):
        for c in L.channels(taps):
            rec = L.records_of(L.reference(oracle, taps, c["name"]), taps)
            dist, seen = L.replay(rec, c, taps, gate=0)
            assert not any(dist.values()), (c["name"], dist)
            for k, v in seen.items():
                total[k] += v
    assert all(v > 0 for v in total.values()), total


def test_replay_notices_a_wrong_record(oracle):
    """One ulp in one recorded output of an IEEE-only stage is a failure of the replay."""
    c = next(c for c in L.channels(5) if c["name"] == "B-dll3-pll3")
    good = L.records_of(L.reference(oracle, 5, c["name"]), 5)
    for field in ("code_error_filt_chips", "code_error_chips", "carrier_doppler_hz", "carrier_lock_test", "rem_code_phase_samples", "acc_carrier_phase_rad"):
        rec = good.copy()
        k = 50 if field != "carrier_lock_test" else int(np.flatnonzero(np.diff(good["carrier_lock_test"]) != 0)[0]) + 1
        k = k if not good["integrating"][k] else k + int(np.flatnonzero(good["integrating"][k:] == 0)[0])
        rec[field][k:] = np.nextafter(rec[field][k:], np.inf, dtype=rec[field].dtype)
        with pytest.raises(AssertionError):
            L.replay(rec, c, 5, gate=3)
