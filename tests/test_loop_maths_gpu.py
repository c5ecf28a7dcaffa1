"""The loop maths of trk_loop_device.hpp on the device, in every configuration of tests/loop_maths_cases.py: all three orders of the
code loop filter and both of the carrier loop filter, the FLL in each mode across the end of the pull-in transitory, the narrow-stage
re-design of both filters, pilot tracking (four-quadrant PLL), and an all-zero input.  tests/test_loop_maths_inputs.py holds the same
channels to their preconditions on the CPU.

All channels of a tap count are slots of one plain engine and one run(96), the two pilot channels of a second one (a plain engine's
channels share the pilot mode): four launches.  Per channel:

1. Trajectory: _compare(records, closed_loop_ref.run(...)) at its fixed-scenario gates; the all-zero channel field by field, NaN equal
   to NaN.
2. Replay (loop_maths_cases.replay): the restatement -- pinned to the reference's compiled loop filter, discriminators and lock
   detectors by tests/test_loop_filter_pin.py -- is fed the device's own recorded accumulators, discriminator outputs and previous
   records, one period at a time, and must give the device's recorded outputs.  Stages of + - * / and sqrt only are compared bit for
   bit: code_error_filt_chips (through the re-design), carr_error_filt_hz / carrier_doppler_hz in PLL-only periods, carrier_lock_test,
   the VEMLP code_error_chips, the accumulators, code_freq_chips, current_prn_length_samples, sample_counter, rem_code_phase_samples,
   acc_carrier_phase_rad, state and extend_count.  A stage behind a libm call -- atanf / atan2f in carr_phase_error_hz, hypotf in the
   E-minus-L code_error_chips, the double atan2 of the FLL discriminator, the double log10 of cn0_db_hz -- must be reproduced with
   that call's result moved by at most G ulp of its own type, G = U_CPU + 2: what numpy's libm may differ from the reference's glibc
   (test_loop_filter_pin.U_CPU) plus the 2 ulp this project grants a device libm result
   (test_device_carrier_filter_against_the_pinned_filter).  The FLL leg is held to more than an interval: the carrier filter must
   give the recorded output, bit for bit, for one of the 2 G + 1 shifted inputs, and goes on from that state.
3. Coverage: periods per branch over all records; none may be empty.
The largest shift needed per libm function is printed (DESIGN.md section 4 records it)."""
import numpy as np
import pytest

import loop_maths_cases as L
from test_loop_filter_pin import U_CPU
from test_loop_sync_gpu import _compare, _conf, _sync

pytestmark = pytest.mark.gpu

G = U_CPU + 2
CASES = [(taps, c["name"]) for taps in (3, 5) for c in L.channels(taps)]


@pytest.fixture(scope="module")
def records(gctx):
    """(taps, channel name) -> the device's 96 records, from the four engine runs; never modified."""
    import gnsscorr
    import torch
    out = {}
    for taps, engine in L.ENGINES:
        chans = L.engine_channels(taps, engine)
        s = L.signal(taps)
        dev = {b: torch.from_numpy(np.ascontiguousarray(s[b]).view(np.float32)).cuda() for b in {c["buffer"] for c in chans}}
        loop = gnsscorr.TrackingLoop(gctx, len(chans), s["code"].size)
        for ch, c in enumerate(chans):
            loop.set_input_dev(ch, dev[c["buffer"]].data_ptr(), s[c["buffer"]].size)
            loop.set_sync(ch, _sync(gnsscorr, c["sync"]) if c["sync"] else None, s["data_code"] if engine == "pilot" else None)
            loop.start(ch, _conf(gnsscorr, **c["conf"]), s["code"])
        rec = loop.run(L.N_EP)
        loop.close()
        for ch, c in enumerate(chans):
            out[taps, c["name"]] = rec[ch].copy()
            out[taps, c["name"]].flags.writeable = False
    return out


@pytest.fixture(scope="module")
def replayed(records):
    """(taps, channel name) -> (libm distances, branch counts) or the replay's AssertionError."""
    out = {}
    for taps in (3, 5):
        for c in L.channels(taps):
            try:
                out[taps, c["name"]] = L.replay(records[taps, c["name"]], c, taps, gate=G)
            except AssertionError as e:
                out[taps, c["name"]] = e
    worst = dict.fromkeys(L.LIBM, 0)
    for r in out.values():
        if not isinstance(r, AssertionError):
            worst = {k: max(v, r[0][k]) for k, v in worst.items()}
    print("loop maths on the device, largest shift of a libm result that reproduces the records [ulp] (gate %d): %s" % (G, worst))
    return out


@pytest.mark.parametrize("taps,name", CASES, ids=str)
def test_trajectory_equals_the_cpu_restatement(records, oracle, taps, name):
    rec, ref = records[taps, name], L.reference(oracle, taps, name)
    assert np.all(rec["valid"] == 1)
    if not name.startswith("D-"):
        _compare(rec, ref, taps)
        return
    want = L.records_of(ref, taps)
    for field in rec.dtype.names:
        a, b = rec[field], want[field]
        same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
        assert np.all(same), (field, np.argwhere(~same)[:3])
    assert np.all(np.isnan(rec["cn0_db_hz"][11:])) and np.all(np.isnan(rec["carrier_lock_test"][11:])) and np.all(rec["state"] == 2)


@pytest.mark.parametrize("taps,name", CASES, ids=str)
def test_replay_of_the_device_records_through_the_pinned_maths(replayed, taps, name):
    r = replayed[taps, name]
    if isinstance(r, AssertionError):
        raise r
    dist, seen = r
    print("%d taps %s: libm shifts %s" % (taps, name, {k: v for k, v in dist.items() if v}))
    assert max(dist.values()) <= G


def test_every_branch_is_met(replayed):
    total = dict.fromkeys(L.BRANCHES, 0)
    for r in replayed.values():
        assert not isinstance(r, AssertionError), r
        for k, v in r[1].items():
            total[k] += v
    print("periods per branch:", total)
    assert all(v > 0 for v in total.values()), total
