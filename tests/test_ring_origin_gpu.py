"""GPU tests of everything that reads a gc_stream ring, and of the two index-driven ring stages, at the absolute sample numbers of
a stream that has been running for minutes and hours: rings whose origin (IqStream.set_origin, gc_stream_debug_set_origin) lies
just below 2^31 and 2^32 -- so that the boundary falls inside the first window or block -- and at 2^40 + 12345 and 2^53 + 1
(tests/ring_origin_cases.py has the table and what it asserts about itself).

Readers -- TrackingBatch, TrackingLoop, acquisition of every engine kind, FineDoppler, IqStream.read -- are held to BIT IDENTITY with
a small-index twin: a second ring of the same capacity, max_window and format at origin 0 that first receives lead = G % capacity
samples of unrelated noise and then the identical blocks, so that every sample lies at the same storage position in both rings,
mirror included.  An engine driven with indices G + k on the ring under test and lead + k on the twin must return identical bytes;
fields that ARE absolute sample numbers must differ by exactly G - lead, compared as Python integers.  One case per engine is also
held against its CPU reference at the tolerance of that engine's own test file, so that two equally wrong runs cannot pass.

The ring decimator and the ring resampler are held against their restatements evaluated at absolute indices
(conditioner_ref.decimate_from, resampler_ref.direct_from / polyphase_from): first_out and n_out of every update against the
exact-integer model, and every stored byte of the output ring, mirror and slack included, against tests/ring_model.py.

Requests whose first + length passes 2^64, and a read floor above the head, are host-side refusals: status and message are
asserted, and that a following valid call gives the twin's bytes."""
import numpy as np
import pytest

import conditioner_ref
import resampler_ref
import ring_model
import ring_origin_cases as cases
from helpers import rel_err, synth_stream

pytestmark = pytest.mark.gpu
FMT_NAMES = ["GC_IQ_F32", "GC_IQ_I16", "GC_IQ_I8"]
U64 = 1 << 64
_shared = {}  # scenes and references, computed once and shared; nobody changes them


def _fmt(name):
    import gnsscorr
    return getattr(gnsscorr, name)


def _noise(n, fmt_name, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    if fmt_name == "GC_IQ_F32":
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    dt = np.int16 if fmt_name == "GC_IQ_I16" else np.int8
    return rng.integers(np.iinfo(dt).min, np.iinfo(dt).max + 1, size=(n, 2)).astype(dt)


def _quantise(x, fmt_name, scale):
    """complex64 -> the samples as pushed in the format, and the complex64 values those samples are."""
    if fmt_name == "GC_IQ_F32":
        return x, x
    dt = np.int16 if fmt_name == "GC_IQ_I16" else np.int8
    lim = np.iinfo(dt).max
    q = np.clip(np.round(x.view(np.float32).reshape(-1, 2) * scale), -lim, lim).astype(dt)
    return q, (q[:, 0].astype(np.float32) + 1j * q[:, 1].astype(np.float32)).astype(np.complex64)


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _refused(status, *texts):
    """Context manager: the call is refused with `status` and a message that holds every text."""
    import gnsscorr

    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(gnsscorr.GnsscorrError)
            self.e = self.cm.__enter__()
            return self.e

        def __exit__(self, *exc):
            out = self.cm.__exit__(*exc)
            assert self.e.value.status == status, (self.e.value.status, str(self.e.value))
            for t in texts:
                assert t in str(self.e.value), (t, str(self.e.value))
            return out
    return Ctx()


class Twins:
    """The ring under test at origin G and its small-index twin; push() feeds both and the host model of the first."""

    def __init__(self, gctx, case, origin_name, fmt_name="GC_IQ_F32"):
        import gnsscorr
        c = cases.CASES[case]
        self.C, self.W, self.fmt_name = c["capacity"], c["window"], fmt_name
        self.G = cases.origin(origin_name, c["a"])
        self.lead = cases.lead(self.G, self.C)
        self.shift = self.G - self.lead
        fmt = _fmt(fmt_name)
        self.ring = gnsscorr.IqStream(gctx, self.C, self.W, fmt)
        assert self.ring.set_origin(self.G) is self.ring
        self.twin = gnsscorr.IqStream(gctx, self.C, self.W, fmt)
        dt, per = gnsscorr.IqStream._DTYPES[fmt]
        self.model = ring_model.RingModel(self.C, self.W, dt, per, origin=self.G)
        assert self.ring.info() == (self.G, self.G, self.C)
        self.check_storage("after set_origin")  # the storage stays zero-filled
        if self.lead:
            assert self.twin.push(_noise(self.lead, fmt_name, 999)) == 0
        self.pushed = 0

    def push(self, block):
        n = len(block)
        assert self.ring.push(block) == self.G + self.pushed and self.twin.push(block) == self.lead + self.pushed
        self.model.append(np.asarray(block))
        self.pushed += n
        assert self.ring.info() == self.model.resident() + (self.C,), (self.ring.info(), self.model.resident())
        assert self.twin.info()[:2] == (max(0, self.lead + self.pushed - self.C), self.lead + self.pushed)

    def check_storage(self, what):
        got = self.ring.read_storage(0, self.model.total)
        diff = self.model.first_difference(got)
        assert diff is None, "%s: storage position %d, in the %s, holds %s; the model holds %s" % ((what,) + diff)
        assert self.ring.guards_intact() == (True, True), (what, self.ring.guards_intact())

    def finish(self, case=None):
        """Every stored byte against the model, both rings' guard bands, and -- once more than a ring's worth has been pushed, so
        that nothing of the twin's lead is left -- the twin's storage against the ring's."""
        self.check_storage("at the end")
        assert self.twin.guards_intact() == (True, True)
        if self.pushed >= self.C + self.W:
            assert _same_bytes(self.twin.read_storage(0, self.model.total), self.ring.read_storage(0, self.model.total))
        if case is not None and cases.CASES[case]["streaming"]:
            assert self.pushed >= 2 * self.C, (self.pushed, self.C)  # the ring wrapped at least twice behind the origin
        self.ring.close()
        self.twin.close()


# ---- the hook itself, IqStream.read / info / read_storage / guards_intact ------------------------------------------------------

@pytest.mark.parametrize("fmt_name", FMT_NAMES)
@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_stream_read_info_and_storage_across_the_boundary(gctx, origin_name, fmt_name):
    import gnsscorr
    t = Twins(gctx, "stream", origin_name, fmt_name)
    G, C = t.G, t.C
    # allowed once, on an empty ring: a second origin changes nothing
    with _refused(gnsscorr.GC_ERR_STATE, "gc_stream_debug_set_origin", "origin already"):
        t.ring.set_origin(G + 1)
    assert t.ring.info() == (G, G, C)
    # nothing is resident yet: the empty window at the origin reads, everything else is refused
    assert len(t.ring.read(G, 0)) == 0
    for first, n in ((G - 1, 1), (G, 1), (0, 1), (G - 1, 0)):
        with _refused(gnsscorr.GC_ERR_STATE, "not resident"):
            t.ring.read(first, n)
    x = _noise(cases.CASES["stream"]["pushed"], fmt_name, 7)
    sizes = [1, 96, 95, 1500, 3001, 2, 3000, 97, 1203]
    at = 0
    k = 0
    while at < len(x):
        n = min(sizes[k % len(sizes)], len(x) - at)
        k += 1
        t.push(x[at:at + n])
        at += n
        t.check_storage("push %d" % k)
        oldest, head, _ = t.ring.info()
        assert (oldest, head) == (max(G, G + at - C), G + at) and isinstance(head, int)
        lo = oldest - G
        # the whole resident range, the newest and the oldest sample, and the same window of the twin
        assert _same_bytes(t.ring.read(oldest, head - oldest), x[lo:at])
        assert _same_bytes(t.ring.read(head - 1, 1), x[at - 1:at]) and _same_bytes(t.ring.read(oldest, 1), x[lo:lo + 1])
        assert _same_bytes(t.twin.read(oldest - t.shift, head - oldest), x[lo:at])
        if origin_name in cases.BOUNDARY and oldest < cases.BOUNDARY[origin_name] < head:
            b = cases.BOUNDARY[origin_name]
            w = min(b - oldest, head - b, 40)
            assert w > 0 and _same_bytes(t.ring.read(b - w, 2 * w), x[b - w - G:b + w - G])
        # below the resident range (and below the origin), above the head, and a sum that passes 2^64
        for first, n in ((oldest - 1, 1), (G - 1, 1), (oldest - 1, 0), (head, 1), (head - 1, 2), (head + 1, 0), (U64 - 1, 2), (U64 - 1, 1), (U64 - 40, 96),
                (t.lead + lo, 1)):
            with _refused(gnsscorr.GC_ERR_STATE, "gc_stream_read", "not resident"):
                t.ring.read(first, n)
    if origin_name in cases.BOUNDARY:
        assert G < cases.BOUNDARY[origin_name] < G + at
    with _refused(gnsscorr.GC_ERR_STATE, "gc_stream_debug_set_origin"):
        t.ring.set_origin(0)
    t.finish("stream")


def test_the_hook_refuses_what_it_must(gctx):
    import gnsscorr
    ring = gnsscorr.IqStream(gctx, 3001, 96)
    with _refused(gnsscorr.GC_ERR_INVALID, "gc_stream_debug_set_origin", "2^62"):
        ring.set_origin((1 << 62) + 1)
    with _refused(gnsscorr.GC_ERR_INVALID, "gc_stream_debug_set_origin", "2^62"):
        ring.set_origin(U64 - 1)
    assert ring.info() == (0, 0, 3001)
    ring.set_origin(1 << 62)  # the largest one
    assert ring.info() == (1 << 62, 1 << 62, 3001)
    x = _noise(100, "GC_IQ_F32", 1)
    assert ring.push(x) == 1 << 62 and _same_bytes(ring.read(1 << 62, 100), x)
    assert _same_bytes(ring.read_storage((1 << 62) % 3001, 50), x[:50])
    ring.close()
    # a ring that holds samples; a ring with a producer on the device; origin 0 counts as an origin
    ring = gnsscorr.IqStream(gctx, 3001, 96)
    ring.push(x)
    with _refused(gnsscorr.GC_ERR_STATE, "gc_stream_debug_set_origin", "pushed"):
        ring.set_origin(5)
    assert ring.info() == (0, 100, 3001)
    out = gnsscorr.IqStream(gctx, 3001, 96)
    dec = gnsscorr.RingDecimator(gctx, ring, 2, np.ones(3, np.float32), out)
    with _refused(gnsscorr.GC_ERR_STATE, "gc_stream_debug_set_origin", "producer"):
        out.set_origin(5)
    assert dec.update() == (0, 50) and out.info()[:2] == (0, 50)
    dec.close()
    out.close()
    ring.close()
    ring = gnsscorr.IqStream(gctx, 3001, 96).set_origin(0)
    with _refused(gnsscorr.GC_ERR_STATE, "gc_stream_debug_set_origin"):
        ring.set_origin(0)
    assert ring.push(x) == 0 and ring.info() == (0, 100, 3001)
    ring.close()


# ---- TrackingBatch on a ring ---------------------------------------------------------------------------------------------------

FS, N, L = 4_000_000, 4000, 1023
TRK_EPOCHS, TRK_PUSH, TRK_PUSHES = 6, 6 * N + 7, 4
TRK_TOL = 1e-4  # tests/test_tracking_gpu.py: max_t |gpu[t] - oracle[t]| / |P_oracle|
SHIFTS = np.array([-0.5, 0.0, 0.5], np.float32)


def _trk_scene(oracle, fmt_name):
    """Two satellites in one stream; after push k both channels correlate six windows, channel ch's at rel = k PUSH + ch + e N (so
    odd and even starts).  Returns (samples as pushed, codes, rel[k][ch][e], scalars, oracle outputs [k][ch][e][tap])."""
    key = ("trk", fmt_name)
    if key not in _shared:
        codes = [oracle.gps_l1_ca_code(p).astype(np.float32) for p in (2, 5)]
        sig, truth = synth_stream(codes, FS, TRK_PUSHES * TRK_PUSH, seed=41, cn0_db_hz=(46.0, 48.0))
        raw, clean = _quantise(sig, fmt_name, 300.0 if fmt_name == "GC_IQ_I16" else 25.0)
        rel, args = [], []
        want = np.zeros((TRK_PUSHES, 2, TRK_EPOCHS, 3), np.complex64)
        for k in range(TRK_PUSHES):
            rel.append([[k * TRK_PUSH + ch + e * N for e in range(TRK_EPOCHS)] for ch in range(2)])
            args.append([[None] * TRK_EPOCHS for _ in range(2)])
            for ch in range(2):
                tr = truth[ch]
                step = tr["code_rate"] / FS
                for e, start in enumerate(rel[k][ch]):
                    rem = -((tr["tau0"] + start * step) % L)
                    rem = rem + L if rem < -L / 2 else rem
                    a = (np.float32((tr["phi"] + 2 * np.pi * tr["doppler"] * start / FS) % (2 * np.pi)), np.float32(2 * np.pi * tr["doppler"] / FS), np.float32(rem),
                        np.float32(step))
                    args[k][ch][e] = a
                    want[k, ch, e] = oracle.multicorrelator(clean[start:], codes[ch], SHIFTS, a[0], a[1], a[2], a[3], N)
                    assert start % 2 == (k + ch) % 2 and start + N <= (k + 1) * TRK_PUSH
        want.setflags(write=False)
        _shared[key] = (raw, codes, rel, args, want)
    return _shared[key]


def _records(gnsscorr, base, rel, args):
    """EPOCH_DTYPE records [ch][e] of one push with `base` added to every window start; sample_offset is set from a Python integer."""
    recs = gnsscorr.epoch_params_array([[gnsscorr.epoch_params(base + s, float(a[0]), float(a[1]), float(a[2]), float(a[3]), N) for s, a in zip(rel[ch], args[ch])]
        for ch in range(2)])
    assert [int(v) for v in recs["sample_offset"]] == [base + s for ch in range(2) for s in rel[ch]]
    return recs


@pytest.mark.parametrize("slices", ["auto", 3])
@pytest.mark.parametrize("fmt_name", FMT_NAMES)
@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_tracking_batch(gctx, oracle, origin_name, fmt_name, slices):
    """Two channels on one ring, six epochs per launch, windows before and after the ring wraps (and across its end, through the
    mirror): run() with host records, and run_dev() with device records behind set_read_floor(G + ...)."""
    import gnsscorr
    import torch
    raw, codes, rel, args, want = _trk_scene(oracle, fmt_name)
    t = Twins(gctx, "tracking", origin_name, fmt_name)
    batches = []
    for ring in (t.ring, t.twin):
        b = gnsscorr.TrackingBatch(gctx, 2, 3, L)
        if fmt_name != "GC_IQ_F32":
            b.set_input_format(_fmt(fmt_name))
        if slices != "auto":
            b.set_slices(slices)
        for ch in range(2):
            b.set_code(ch, codes[ch], SHIFTS)
            b.set_input_stream(ch, ring)
        batches.append(b)
    stream = torch.cuda.Stream()
    worst = 0.0
    wrapped_windows = 0
    for k in range(TRK_PUSHES):
        t.push(raw[k * TRK_PUSH:(k + 1) * TRK_PUSH])
        outs, outs_dev = [], []
        for b, base in zip(batches, (t.G, t.lead)):
            recs = _records(gnsscorr, base, rel[k], args[k])
            outs.append(b.run(TRK_EPOCHS, recs))
            d_recs = torch.from_numpy(recs.view(np.uint8).copy()).cuda()
            d_out = torch.zeros(2 * TRK_EPOCHS * 3, 2, device="cuda", dtype=torch.float32)
            b.set_read_floor(base + k * TRK_PUSH)
            b.run_dev(TRK_EPOCHS, d_recs.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            outs_dev.append(d_out.cpu().numpy().view(np.complex64).reshape(2, TRK_EPOCHS, 3))
        assert _same_bytes(outs[0], outs[1]), (k, np.flatnonzero(np.any(outs[0] != outs[1], axis=2).reshape(-1)))
        assert _same_bytes(outs_dev[0], outs_dev[1]), k
        # the anchor: the float ring against the CPU oracle (the twin's bytes are the ring's, so both are held)
        for got in ((outs[0], outs_dev[0]) if fmt_name == "GC_IQ_F32" else ()):
            for ch in range(2):
                for e in range(TRK_EPOCHS):
                    worst = max(worst, rel_err(got[ch, e], want[k, ch, e], 1))
        wrapped_windows += sum((t.G + s) % t.C + N > t.C for ch in range(2) for s in rel[k][ch])
    print("tracking batch %s %s slices=%s: worst relative error against the oracle %.3e (bound %.1e)" % (origin_name, fmt_name, slices, worst, TRK_TOL))
    assert worst <= TRK_TOL and (worst > 0.0) == (fmt_name == "GC_IQ_F32")
    assert wrapped_windows >= 2  # windows that cross the ring's end and are read through the mirror
    if origin_name in cases.BOUNDARY:
        assert t.G + rel[0][0][0] < cases.BOUNDARY[origin_name] < t.G + rel[0][0][0] + N  # inside the first correlated window
    for b in batches:
        b.close()
    t.finish("tracking")


# ---- TrackingLoop --------------------------------------------------------------------------------------------------------------

LOOP_EPOCHS = 40


def _loop_scene(oracle):
    if "loop" not in _shared:
        from test_closed_loop_gpu import _signal
        code, x = _signal(oracle, 9, 4e6, N * (LOOP_EPOCHS + 3), 55, -2210.0, 777.0)
        x.setflags(write=False)
        _shared["loop"] = (code, x)
    return _shared["loop"]


def _loop_conf(origin):
    from test_closed_loop_gpu import GPS
    return dict(GPS, acq_delay_samples=777.0, acq_doppler_hz=-2200.0, acq_samplestamp_samples=origin, sample_counter=origin)


def _loop_block_run(gctx, oracle, origin):
    """The closed loop on the capture held as one block, its counters moved by `origin` (computed once per origin)."""
    key = ("loop-block", origin)
    if key not in _shared:
        import gnsscorr
        import torch
        from test_closed_loop_gpu import _conf
        code, x = _loop_scene(oracle)
        d = torch.from_numpy(x.view(np.float32).copy()).cuda()
        loop = gnsscorr.TrackingLoop(gctx, 1, L)
        loop.set_input_dev(0, d.data_ptr(), x.size)
        loop.start(0, _conf(gnsscorr, **_loop_conf(origin)), code)
        rec = loop.run(LOOP_EPOCHS)[0]
        loop.close()
        rec.setflags(write=False)
        _shared[key] = rec
    return _shared[key]


def _records_differ_by(got, want, shift, what):
    """Every field of the records is identical but sample_counter, which differs by exactly `shift` (Python integers)."""
    assert len(got) == len(want), (what, len(got), len(want))
    for name in want.dtype.names:
        if name == "sample_counter":
            assert [int(v) for v in got[name]] == [int(v) + shift for v in want[name]], what
        else:
            assert _same_bytes(got[name], want[name]), (what, name)


def _against_the_cpu_loop(oracle, rec, shift, what):
    """The anchor of the loop engine: LOOP_EPOCHS valid records against tests/closed_loop_ref.py run on the capture from counter 0,
    at the gates of tests/test_closed_loop_gpu.py::test_closed_loop_matches_cpu_restatement; sample_counter, moved by `shift`,
    exactly (the same block boundaries every epoch)."""
    if "loop-ref" not in _shared:
        from closed_loop_ref import run as ref_run
        code, x = _loop_scene(oracle)
        _shared["loop-ref"] = ref_run(oracle, x, code, _loop_conf(0), LOOP_EPOCHS)
    ref = _shared["loop-ref"]
    assert len(rec) == len(ref) == LOOP_EPOCHS and np.all(rec["valid"] == 1) and np.all(rec["state"] == 2)
    worst_d = worst_p = 0.0
    for k in range(LOOP_EPOCHS):
        r, g = ref[k], rec[k]
        assert int(g["sample_counter"]) == r["sample_counter"] + shift and int(g["current_prn_length_samples"]) == r["cur"], (what, k)
        gp = g["corr"][2] + 1j * g["corr"][3]
        worst_p = max(worst_p, abs(gp - r["corr"][1]) / abs(r["corr"][1]))
        worst_d = max(worst_d, abs(float(g["carrier_doppler_hz"]) - r["doppler"]))
        assert abs(float(g["code_freq_chips"]) - r["code_freq"]) < 0.2
    print("closed loop %s: worst prompt error %.3e (gate 2e-3), worst Doppler error %.3e Hz (gate 0.05)" % (what, worst_p, worst_d))
    assert worst_p < 2e-3 and worst_d < 0.05


def test_tracking_loop_block_input_against_the_cpu_loop(gctx, oracle):
    _against_the_cpu_loop(oracle, _loop_block_run(gctx, oracle, 0), 0, "block input")


@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_tracking_loop_block_input_with_moved_counters(gctx, oracle, origin_name):
    """(a) conf.sample_counter and acq_samplestamp_samples moved by the origin: the same records but for sample_counter."""
    G = cases.origin(origin_name, cases.CASES["loop"]["a"])
    want = _loop_block_run(gctx, oracle, 0)
    got = _loop_block_run(gctx, oracle, G)
    _records_differ_by(got, want, G, origin_name)
    assert int(got["sample_counter"][-1]) > G + (LOOP_EPOCHS - 1) * N


@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_tracking_loop_on_a_ring(gctx, oracle, origin_name):
    """(b) the plain 3-tap engine in "push a block, run" steps over 40 code periods, and (c) at the end the channel is left behind
    by the stream: the refusal names the sample the channel stands at."""
    import gnsscorr
    from test_closed_loop_gpu import _conf
    code, x = _loop_scene(oracle)
    t = Twins(gctx, "loop", origin_name)
    loops = []
    for ring, base in ((t.ring, t.G), (t.twin, t.lead)):
        loop = gnsscorr.TrackingLoop(gctx, 1, L)
        loop.set_input_stream(0, ring)
        loop.start(0, _conf(gnsscorr, **_loop_conf(base)), code)
        loops.append(loop)
    got = [[], []]
    stand = [t.G, t.lead]  # the sample each channel stands at: the counter of the newest record, valid or not
    at = 0
    while at < x.size:
        m = min(6500, x.size - at)  # 1.6 code periods per push: a launch sees one or two complete periods
        t.push(x[at:at + m])
        at += m
        recs = [loop.run(3)[0] for loop in loops]
        _records_differ_by(recs[0][recs[0]["valid"] == 1], recs[1][recs[1]["valid"] == 1], t.shift, (origin_name, at))
        assert _same_bytes(recs[0]["valid"], recs[1]["valid"])
        for i in range(2):
            got[i].extend(r.copy() for r in recs[i] if r["valid"])
            stand[i] = int(recs[i]["sample_counter"][-1])
    got = [np.array(g[:LOOP_EPOCHS]) for g in got]
    assert len(got[0]) == LOOP_EPOCHS and at >= 2 * t.C
    # the anchor: the CPU loop on the capture, counters moved by the origin.  (Not the bytes of a block-input run: a window's
    # position in the ring's storage decides how its samples fall into the kernel's aligned chunks, hence the order of its sums.)
    _against_the_cpu_loop(oracle, got[0], t.G, "ring " + origin_name)
    if origin_name in cases.BOUNDARY:
        assert int(got[0]["sample_counter"][0]) > cases.BOUNDARY[origin_name] > t.G  # inside the first period
    # (c) the stream moves on without the channel
    assert stand[0] - stand[1] == t.shift and t.G + x.size - 2 * N < stand[0] <= t.G + x.size
    zeros = np.zeros(6000, np.complex64)
    for _ in range(6):
        t.push(zeros)
    assert t.ring.info()[0] > stand[0]
    for loop, at_sample in zip(loops, stand):
        with _refused(gnsscorr.GC_ERR_STATE, "gc_trk_loop_run", "fell behind the ring", "(at sample %d)" % at_sample):
            loop.run(1)
    for loop in loops:
        loop.close()
    t.finish("loop")


@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_mixed_tracking_loop_on_a_ring(gctx, origin_name):
    """(b) a mixed engine with one GPS L1 C/A slot and one Galileo E1 slot (the set-up of tests/test_mixed_loop_gpu.py), 10 ms per
    push, 42 Galileo periods."""
    import gnsscorr
    import test_mixed_loop_gpu as tm
    fs, n_ep, blk, n_blk = 4e6, 12, 40000, 17
    if "mixed" not in _shared:
        kinds = [k for k in tm._kinds(gnsscorr, fs) if k[0] in ("gps", "gal_data")]
        _shared["mixed"] = (kinds, tm._stream(kinds, fs, blk * n_blk, seed=9))
    kinds, x = _shared["mixed"]
    assert [k[0] for k in kinds] == ["gps", "gal_data"] and blk * n_blk == cases.CASES["loop-mixed"]["pushed"]
    t = Twins(gctx, "loop-mixed", origin_name)
    engines = []
    for ring, base in ((t.ring, t.G), (t.twin, t.lead)):
        eng = gnsscorr.TrackingLoop(gctx, len(kinds), max(k[2].size for k in kinds), mixed=True)
        for ch, (name, c, code, sync, dc, dop, delay) in enumerate(kinds):
            eng.set_input_stream(ch, ring)
            eng.set_sync(ch, sync, dc)
            eng.start(ch, tm._conf(gnsscorr, **dict(c, acq_delay_samples=float(delay), acq_doppler_hz=dop + 3.0, acq_samplestamp_samples=base, sample_counter=base)), code)
        engines.append(eng)
    valid = [0, 0]
    for k in range(n_blk):
        t.push(x[k * blk:(k + 1) * blk])
        a, b = (eng.run(n_ep) for eng in engines)
        for ch in range(len(kinds)):
            assert _same_bytes(a[ch]["valid"], b[ch]["valid"])
            va, vb = a[ch][a[ch]["valid"] == 1], b[ch][b[ch]["valid"] == 1]
            _records_differ_by(va, vb, t.shift, (origin_name, kinds[ch][0], k))
            # records that are not valid hold no position of their own: identical but for the counter they carry along
            _records_differ_by(a[ch][a[ch]["valid"] != 1], b[ch][b[ch]["valid"] != 1], t.shift, (origin_name, kinds[ch][0], k, "idle"))
            valid[ch] += len(va)
            if len(va):
                assert t.G < int(va["sample_counter"][-1]) <= t.G + (k + 1) * blk
    assert valid[0] >= 4 * 40 and valid[1] >= 40, valid
    for eng in engines:
        eng.close()
    t.finish("loop-mixed")


# ---- acquisition from a ring ---------------------------------------------------------------------------------------------------

ACQ_TOL = 1e-4  # tests/test_acquisition_gpu.py: rows and columns exact, magnitudes within 1e-4 relative


def _acq_stream(fmt_name="GC_IQ_F32"):
    """Noise with the first code of tests/test_acq_engine_kinds_gpu.py repeated in it, a known delay and one Doppler bin off zero."""
    key = ("acq", fmt_name)
    if key not in _shared:
        import test_acq_engine_kinds_gpu as ek
        n = cases.CASES["acquisition"]["pushed"]
        rng = np.random.Generator(np.random.PCG64(21))
        a, _ = ek.codes()
        i = np.arange(n)
        x = (0.5 * a[(i - 123) % ek.SPM] * np.exp(2j * np.pi * 500.0 * i / (ek.SPM * 1000)) + (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * np.sqrt(0.5)).astype(np.complex64)
        raw, clean = _quantise(x, fmt_name, 30.0)
        clean.setflags(write=False)
        _shared[key] = (raw, clean)
    return _shared[key]


def _acq_bits(acq, res):
    import test_acq_engine_kinds_gpu as ek
    return tuple(np.array(getattr(res[0], f)).tobytes() for f in ek.FIELDS), acq.grid(0).tobytes()


def _acq_close_to(res, host):
    """A dwell from the ring against the same engine kind's dwell on the block in host memory, at the acquisition tests' bars."""
    r, q = res[0], host[0]
    assert (r.indext, r.doppler_hz, r.doppler_index) == (q.indext, q.doppler_hz, q.doppler_index)
    assert r.mag == pytest.approx(q.mag, rel=ACQ_TOL) and r.test_statistics == pytest.approx(q.test_statistics, rel=2 * ACQ_TOL)
    assert r.input_power == pytest.approx(q.input_power, rel=ACQ_TOL)


def _target(t, block, n_blocks):
    """The first rel >= 2 capacity, odd as an absolute index, whose block crosses the ring's end."""
    rel = 2 * t.C
    while (t.G + rel) % t.C != t.C - block // 2 + 1 or (t.G + rel) % 2 == 0:
        rel += 1
    assert rel + n_blocks * block <= cases.CASES["acquisition"]["pushed"]
    return rel


@pytest.mark.parametrize("kind", ["plain", "paired", "quicksync", "tong", "caf"])
@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_dwell_stream_of_every_engine_kind(gctx, origin_name, kind):
    """Two consecutive dwells on the first blocks behind the origin (the boundary lies inside the first), then, after the ring has
    wrapped twice, two on blocks at an odd index of which the first crosses the ring's end."""
    import test_acq_engine_kinds_gpu as ek
    case = "acquisition-quicksync" if kind == "quicksync" else "acquisition"
    raw, x = _acq_stream()
    t = Twins(gctx, case, origin_name)
    engines = [ek.engine(gctx, kind) for _ in range(3)]  # the ring's, the twin's, one that takes its blocks from host memory
    for acq in engines:
        ek.set_codes(acq, kind)
    B = engines[0].consumed_samples
    assert B == cases.CASES[case]["first"]
    at = 0

    def push_to(n):
        nonlocal at
        while at < n:
            m = min(1700, n - at)
            t.push(raw[at:at + m])
            at += m

    def dwell(rel):
        got = engines[0].dwell_stream(t.ring, t.G + rel)
        twin = engines[1].dwell_stream(t.twin, t.lead + rel)
        assert _acq_bits(engines[0], got) == _acq_bits(engines[1], twin), (origin_name, kind, rel)
        _acq_close_to(got, engines[2].dwell(x[rel:rel + B]))
        return got
    push_to(2 * B + 100)
    first = dwell(0)
    dwell(B)
    if origin_name in cases.BOUNDARY:
        assert t.G < cases.BOUNDARY[origin_name] < t.G + B
    if kind == "tong":
        for acq in engines:
            acq.reset()  # tong_max_dwells is 3: the second pair of dwells is a search of its own
    rel = _target(t, B, 2)
    push_to(rel + 2 * B)
    assert (t.G + rel) % 2 == 1 and (t.G + rel) % t.C + B > t.C and at >= 2 * t.C
    dwell(rel)
    dwell(rel + B)
    assert first[0].mag > 0
    for acq in engines:
        acq.close()
    push_to(len(raw))
    t.finish(case)


@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_tong_search_stream_with_three_dwells(gctx, origin_name):
    import test_acq_engine_kinds_gpu as ek
    raw, x = _acq_stream()
    t = Twins(gctx, "acquisition", origin_name)
    engines = [ek.engine(gctx, "tong") for _ in range(3)]
    for acq in engines:
        ek.set_codes(acq, "tong")
    B = engines[0].consumed_samples
    at = 0

    def push_to(n):
        nonlocal at
        while at < n:
            m = min(1700, n - at)
            t.push(raw[at:at + m])
            at += m

    def search(rel):
        got, st = engines[0].tong_search_stream(t.ring, t.G + rel, 3)
        twin, st_twin = engines[1].tong_search_stream(t.twin, t.lead + rel, 3)
        assert _acq_bits(engines[0], got) == _acq_bits(engines[1], twin), (origin_name, rel)
        status = [(s.state, s.tong_count, s.dwell_count) for s in st]
        assert status == [(s.state, s.tong_count, s.dwell_count) for s in st_twin] and status[0][2] >= 1
        host = None
        for d in range(3):  # the same three dwells on the blocks in host memory: a decided satellite ignores the later ones there too
            host = engines[2].dwell(x[rel + d * B:rel + (d + 1) * B])
        _acq_close_to(got, host)
        host_status = [(s.state, s.tong_count, s.dwell_count) for s in engines[2].tong_status()]
        assert host_status == status
        return status
    push_to(1600)
    search(0)
    for acq in engines:
        acq.reset()
    rel = _target(t, B, 3)
    push_to(rel + 3 * B)
    search(rel)
    for acq in engines:
        acq.close()
    push_to(len(raw))
    t.finish("acquisition")


@pytest.mark.parametrize("fmt_name", ["GC_IQ_I16"])
@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_dwell_stream_from_an_integer_ring_against_the_oracle(gctx, oracle, origin_name, fmt_name):
    """The anchor of the acquisition engine: a plain PCPS engine (no second step) on a cshort ring, two blocks behind the origin and
    one across the ring's end, against the twin bit for bit and against the CPU oracle on the samples' values at the bars of
    tests/test_acquisition_gpu.py."""
    import gnsscorr
    import test_acq_engine_kinds_gpu as ek
    from test_acquisition_gpu import _check, _conf
    raw, x = _acq_stream(fmt_name)
    conf = _conf(ek.SPM * 1000, 1, 1, float(ek.SPM), ek.DMAX, ek.DSTEP)
    a, _ = ek.codes()
    orc = oracle.pcps(**conf)
    orc.set_local_code(a[:ek.SPM])
    t = Twins(gctx, "acquisition", origin_name, fmt_name)
    engines = []
    for _ in range(2):
        acq = gnsscorr.PcpsAcquisition(gctx, 1, **conf)
        acq.set_input_format(_fmt(fmt_name))
        acq.set_local_code(0, a)
        engines.append(acq)
    B = engines[0].consumed_samples
    at = 0

    def push_to(n):
        nonlocal at
        while at < n:
            m = min(1700, n - at)
            t.push(raw[at:at + m])
            at += m
    push_to(1600)
    rel2 = _target(t, B, 1)
    for rel in (0, B, rel2):
        push_to(rel + B)
        got = engines[0].dwell_stream(t.ring, t.G + rel)
        twin = engines[1].dwell_stream(t.twin, t.lead + rel)
        assert _acq_bits(engines[0], got) == _acq_bits(engines[1], twin), (origin_name, rel)
        q = orc.core(np.ascontiguousarray(x[rel:rel + B]))
        _check(got[0], q)
        grid, ref = engines[0].grid(0), orc.grid()
        assert np.max(np.abs(grid - ref)) <= ACQ_TOL * ref.max()
    assert got[0].test_statistics > 0
    for acq in engines:
        acq.close()
    push_to(len(raw))
    t.finish("acquisition")


# ---- FineDoppler.estimate_stream -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("origin_name", cases.ORIGIN_NAMES)
def test_fine_doppler_estimate_stream(gctx, origin_name):
    """The smallest (N, P, Z) of fine_doppler_cases.MATRIX: the reader whose absolute index reaches the device.  The block lies
    behind the origin (the boundary inside it), then, after two wraps, at an odd index across the ring's end; the results against
    the twin's bit for bit and against the restatement at fine_doppler_cases.check's bars."""
    import fine_doppler_cases as fc
    import fine_doppler_ref as ref
    from test_fine_doppler_gpu import check_all, engine
    N, P, Z = min(fc.MATRIX)
    assert (N, P, Z) == (2000, 1, 1)
    blk = fc.block(N, P, Z)
    recs = fc.records(blk, ref.EXACT)
    n = P * N
    c = cases.CASES["fine-doppler"]
    assert n == c["first"] and n > c["window"]
    t = Twins(gctx, "fine-doppler", origin_name)
    fds = [engine(gctx, blk, ref.EXACT) for _ in range(2)]
    block = blk.x[:n]

    def estimate(rel):
        got = fds[0].estimate_stream(t.ring, t.G + rel, blk.requests)
        twin = fds[1].estimate_stream(t.twin, t.lead + rel, blk.requests)
        assert [fc.result_bits(r) for r in got] == [fc.result_bits(r) for r in twin], (origin_name, rel)
        assert [fds[0].spectrum(i).tobytes() for i in range(len(got))] == [fds[1].spectrum(i).tobytes() for i in range(len(got))]
        check_all(fds[0], got, recs)
    t.push(block)
    estimate(0)
    if origin_name in cases.BOUNDARY:
        assert t.G < cases.BOUNDARY[origin_name] < t.G + n
    # noise up to an odd index whose block crosses the ring's end, behind two wraps
    rel = 2 * t.C + n
    while (t.G + rel) % t.C != t.C - n // 2 + 1 or (t.G + rel) % 2 == 0:
        rel += 1
    fill = _noise(rel - n, "GC_IQ_F32", 5)
    for at in range(0, len(fill), 3000):
        t.push(fill[at:at + 3000])
    t.push(block)
    assert t.pushed == rel + n <= c["pushed"] and (t.G + rel) % 2 == 1 and (t.G + rel) % t.C + n > t.C
    estimate(rel)
    for fd in fds:
        fd.close()
    t.finish("fine-doppler")


# ---- the ring decimator and the ring resampler on a source with an origin -------------------------------------------------------

SRC_PUSHES = [1, 300, 151, 2999, 5700, 2, 4001, 3000, 1867]  # 18021 = 3 x 6007 samples: the source wraps three times; no push evicts the
# history (at most 299 samples) the next update still reads


def _stage_source(fmt_name):
    key = ("stage-src", fmt_name)
    if key not in _shared:
        from test_ring_resampler_gpu import _raw
        assert sum(SRC_PUSHES) == cases.CASES["stage-source"]["pushed"]
        raw = _raw(sum(SRC_PUSHES), _fmt(fmt_name), 77)
        raw.setflags(write=False)
        _shared[key] = raw
    return _shared[key]


def _run_stage(gctx, origin_name, src_fmt_name, out_fmt_name, make, reference, first_output, available, what, quantiser=False, compare=None):
    """make(src, out) -> the stage; reference(G, raw) -> (m0, every output the whole source completes, in the output ring's
    format or as complex128 for `compare`); first_output(G) and available(head): the exact-integer model.  After each update:
    first_out and n_out, the output ring's resident range, and every stored byte of the output ring against the model."""
    import gnsscorr
    c = cases.CASES["stage-source"]
    G = cases.origin(origin_name, c["a"])
    raw = _stage_source(src_fmt_name)
    src = gnsscorr.IqStream(gctx, c["capacity"], c["window"], _fmt(src_fmt_name)).set_origin(G)
    out_fmt = _fmt(out_fmt_name)
    out = gnsscorr.IqStream(gctx, cases.STAGE_OUT_CAPACITY, cases.STAGE_OUT_WINDOW, out_fmt)
    if quantiser and out_fmt != gnsscorr.GC_IQ_F32:
        out.accept_quantised_output()
    stage = make(src, out)
    m0 = first_output(G)
    assert isinstance(m0, int) and m0 > 0
    # the output ring has received the first whole-window output as its own origin
    assert out.info() == (m0, m0, cases.STAGE_OUT_CAPACITY)
    m0_ref, y = reference(G, raw)
    assert m0_ref == m0
    dt, per = gnsscorr.IqStream._DTYPES[out_fmt]
    model = ring_model.RingModel(cases.STAGE_OUT_CAPACITY, cases.STAGE_OUT_WINDOW, dt, per, origin=m0)
    stored = None if compare is None else np.zeros(len(y), np.complex64)
    pushed, head_m = 0, m0
    for k, n in enumerate(SRC_PUSHES):
        assert src.push(raw[pushed:pushed + n]) == G + pushed
        pushed += n
        first, n_out = stage.update()
        want_head = max(m0, available(G + pushed))
        assert (first, n_out) == (head_m, want_head - head_m), (what, k, (first, n_out), (head_m, want_head - head_m))
        lo, hi = head_m - m0, want_head - m0
        if compare is None:
            model.append(y[lo:hi])
        else:
            # a float ring: what the device stored, held against the float64 reference within the bound, is what the model holds
            if hi > lo:
                got = out.read(want_head - min(hi - lo, cases.STAGE_OUT_CAPACITY), min(hi - lo, cases.STAGE_OUT_CAPACITY))
                stored[hi - len(got):hi] = got
                if hi - lo > len(got):  # a call of more than the ring holds: the older outputs are evicted unseen; the reference stands in
                    stored[lo:hi - len(got)] = y[lo:hi - len(got)].astype(np.complex64)
                compare(got, y[hi - len(got):hi], "%s, update %d" % (what, k))
            model.append(stored[lo:hi])
        head_m = want_head
        assert out.info()[:2] == model.resident() == (max(m0, head_m - cases.STAGE_OUT_CAPACITY), head_m)
        assert stage.info() == (G + pushed, head_m)
        diff = model.first_difference(out.read_storage(0, model.total))
        assert diff is None, "%s, update %d: storage position %d, in the %s, holds %s; the model holds %s" % ((what, k) + diff)
        assert out.guards_intact() == (True, True) and src.guards_intact() == (True, True)
    assert pushed >= 2 * c["capacity"] and head_m - m0 == len(y) and head_m - m0 >= 2 * cases.STAGE_OUT_CAPACITY
    # nothing below the output ring's origin is resident to a reader
    with pytest.raises(gnsscorr.GnsscorrError):
        out.read(m0 - 1, 1)
    stage.close()
    out.close()
    src.close()


@pytest.mark.parametrize("src_fmt_name, out_fmt_name, D, T", [("GC_IQ_F32", "GC_IQ_F32", 3, 7), ("GC_IQ_I16", "GC_IQ_F32", 2, 300), ("GC_IQ_F32", "GC_IQ_I16", 3, 7)])
@pytest.mark.parametrize("origin_name", cases.STAGE_ORIGIN_NAMES)
def test_ring_decimator_on_a_source_with_an_origin(gctx, origin_name, src_fmt_name, out_fmt_name, D, T):
    """Decimations that do not divide the origin; 300 taps are more than one tile's history; f32 output and one i16 output, which is
    the restated quantisation (conditioner_out_ref) of the float ring's outputs."""
    import gnsscorr
    import conditioner_out_ref as out_ref
    from test_conditioner_gpu import _taps
    taps = _taps(T, D)
    G = cases.origin(origin_name, cases.CASES["stage-source"]["a"])
    assert G % D != 0
    raw = _stage_source(src_fmt_name)
    m0, ref = conditioner_ref.decimate_from(G, raw, taps, D)
    bound = conditioner_ref.error_bound(taps, raw)
    assert np.abs(ref).max() > 100 * bound
    worst = [0.0]

    def compare(got, want, what):
        err = float(max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()))
        worst[0] = max(worst[0], err)
        assert err <= bound, (what, err, bound)

    def make(scale):
        def f(src, out):
            dec = gnsscorr.RingDecimator(gctx, src, D, taps, out)
            if scale is not None:
                dec.set_output_scale(scale)
            return dec
        return f
    first_output = lambda g: -(-(g + T - 1) // D)
    available = lambda head: -(-head // D)
    what = "ring decimator %s %s -> %s D=%d T=%d" % (origin_name, src_fmt_name, out_fmt_name, D, T)
    if out_fmt_name == "GC_IQ_F32":
        _run_stage(gctx, origin_name, src_fmt_name, out_fmt_name, make(None), lambda g, r: (m0, ref), first_output, available, what, compare=compare)
        print("%s: max component error %.3e, bound %.3e" % (what, worst[0], bound))
        return
    # the integer ring: first the float ring's outputs from one update on a source that holds everything, held to the bound; the
    # integer ring must hold exactly their restated quantisation
    peak = max(np.abs(ref.real).max(), np.abs(ref.imag).max())
    scale = float(np.float32(out_ref.RANGES[_fmt(out_fmt_name)][1] / (0.6 * peak)))
    src = gnsscorr.IqStream(gctx, 32771, 64, _fmt(src_fmt_name)).set_origin(G)
    out = gnsscorr.IqStream(gctx, 8209, 96)
    dec = gnsscorr.RingDecimator(gctx, src, D, taps, out)
    src.push(raw)
    assert dec.update() == (m0, len(ref)) and len(ref) < 8209
    y32 = out.read(m0, len(ref))
    compare(y32, ref, what + ", float ring")
    for h in (dec, out, src):
        h.close()
    yq, n_clipped = out_ref.quantise(y32, _fmt(out_fmt_name), scale)
    assert 0 < n_clipped < yq.size // 4
    _run_stage(gctx, origin_name, src_fmt_name, out_fmt_name, make(scale), lambda g, r: (m0, yq), first_output, available, what, quantiser=True)


@pytest.mark.parametrize("fmt_name, fs_in, fs_out", [("GC_IQ_F32", 25e6, 10e6), ("GC_IQ_I16", 4e6, 5e6), ("GC_IQ_I8", 4e6, 4e6), ("GC_IQ_I8", 25e6, 10e6)])
@pytest.mark.parametrize("origin_name", cases.STAGE_ORIGIN_NAMES)
def test_ring_resampler_direct_on_a_source_with_an_origin(gctx, origin_name, fmt_name, fs_in, fs_out):
    """DOWN, UP and IDENTITY move bits: the output ring holds raw[n_m] exactly."""
    import gnsscorr
    kind, step = resampler_ref.direct_ratio(fs_in, fs_out)
    _run_stage(gctx, origin_name, fmt_name, fmt_name, lambda s, o: gnsscorr.RingResampler(gctx, s, fs_in, fs_out, o, "direct"),
        lambda g, r: resampler_ref.direct_from(g, r, fs_in, fs_out), lambda g: resampler_ref.first_output(kind, step, g),
        lambda head: resampler_ref.available(kind, step, head), "ring resampler direct %s %s %g -> %g" % (origin_name, fmt_name, fs_in, fs_out))


@pytest.mark.parametrize("src_fmt_name", ["GC_IQ_F32", "GC_IQ_I16"])
@pytest.mark.parametrize("origin_name", cases.STAGE_ORIGIN_NAMES)
def test_ring_resampler_polyphase_on_a_source_with_an_origin(gctx, origin_name, src_fmt_name):
    """POLY against the float64 bank sum at absolute indices, within resampler_ref.error_bound."""
    import gnsscorr
    import ring_contract_cases as rc
    fs_in, fs_out, phases = rc.POLYPHASE
    if "bank" not in _shared:
        _shared["bank"] = gnsscorr.resampler_design(fs_in, fs_out, phases)
    bank = _shared["bank"]
    kind, inc = resampler_ref.poly_ratio(fs_in, fs_out)
    raw = _stage_source(src_fmt_name)
    bound = resampler_ref.error_bound(bank, raw)
    worst = [0.0]

    def compare(got, want, what):
        err = float(max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()))
        worst[0] = max(worst[0], err)
        assert err <= bound, (what, err, bound)
    what = "ring resampler polyphase %s from %s" % (origin_name, src_fmt_name)
    _run_stage(gctx, origin_name, src_fmt_name, "GC_IQ_F32", lambda s, o: gnsscorr.RingResampler(gctx, s, fs_in, fs_out, o, "polyphase", bank),
        lambda g, r: resampler_ref.polyphase_from(g, r, bank, fs_in, fs_out), lambda g: resampler_ref.first_output(kind, inc, g, bank.shape[1]),
        lambda head: resampler_ref.available(kind, inc, head), what, compare=compare)
    print("%s: max component error %.3e, bound %.3e" % (what, worst[0], bound))


def test_stages_that_keep_to_origin_zero_say_so(gctx):
    """RingNotch on a source with an origin is GC_ERR_STATE and the message names the origin -- not "no longer holds sample 0" --;
    a decimator on a source that has evicted since its origin is refused; a conditioner takes no output ring with an origin."""
    import gnsscorr
    G = (1 << 40) + 12345
    src = gnsscorr.IqStream(gctx, 6007, 64).set_origin(G)
    out = gnsscorr.IqStream(gctx, 3001, 96)
    with _refused(gnsscorr.GC_ERR_STATE, "gc_ring_notch_create", "origin %d" % G) as e:
        gnsscorr.RingNotch(gctx, src, out)
    assert "sample 0 (" not in str(e.value)
    assert out.info() == (0, 0, 3001) and src.info() == (G, G, 6007)
    # the output ring is still free: a decimator takes it, and then holds it
    dec = gnsscorr.RingDecimator(gctx, src, 3, np.ones(7, np.float32), out)
    assert out.info()[:2] == (-(-(G + 6) // 3),) * 2
    out2 = gnsscorr.IqStream(gctx, 3001, 96)
    x = _noise(6007, "GC_IQ_F32", 2)
    src.push(x)
    src.push(x[:10])  # ten samples evicted since the origin
    for make in (lambda: gnsscorr.RingDecimator(gctx, src, 3, np.ones(7, np.float32), out2), lambda: gnsscorr.RingResampler(gctx, src, 25e6, 10e6, out2, "direct")):
        with _refused(gnsscorr.GC_ERR_STATE, "no longer holds its origin", str(G), str(G + 10)):
            make()
    assert out2.info() == (0, 0, 3001)
    with _refused(gnsscorr.GC_ERR_STATE, "fell behind"):
        dec.update()  # the decimator's own first window has been evicted as well
    dec.close()
    # a conditioner and a signal generator number their own input: no output ring with an origin
    ring = gnsscorr.IqStream(gctx, 3001, 96).set_origin(G)
    with pytest.raises(gnsscorr.GnsscorrError):
        gnsscorr.Conditioner(gctx, ring, 16e6, 0.0, 1, np.ones(1, np.float32))
    # nor does a derived stage: its output ring receives the origin from the stage
    src0 = gnsscorr.IqStream(gctx, 6007, 64)
    with _refused(gnsscorr.GC_ERR_STATE, "gc_ring_decimator_create", "the output ring has an origin of its own (%d)" % G):
        gnsscorr.RingDecimator(gctx, src0, 3, np.ones(7, np.float32), ring)
    src0.close()
    assert ring.info() == (G, G, 3001)
    assert ring.push(x[:5]) == G  # and the ring is still the host's to push into
    for h in (ring, out2, out, src):
        h.close()


# ---- requests that pass 2^64, and a read floor above the head -------------------------------------------------------------------

def test_tracking_batch_refuses_windows_that_pass_2_64_and_floors_above_the_head(gctx, oracle):
    import gnsscorr
    import torch
    raw, codes, rel, args, want = _trk_scene(oracle, "GC_IQ_F32")
    t = Twins(gctx, "tracking", "2^40+12345")
    batches = []
    for ring in (t.ring, t.twin):
        b = gnsscorr.TrackingBatch(gctx, 2, 3, L)
        for ch in range(2):
            b.set_code(ch, codes[ch], SHIFTS)
            b.set_input_stream(ch, ring)
        batches.append(b)
    t.push(raw[:TRK_PUSH])
    good = _records(gnsscorr, t.G, rel[0], args[0])
    for first in (U64 - 1, U64 - N, U64 - N + 1, U64 - (N - 1) // 2, (1 << 63) + t.G):
        bad = good.copy()
        bad["sample_offset"][7] = first
        assert int(bad["sample_offset"][7]) == first
        with _refused(gnsscorr.GC_ERR_INVALID, "gc_trk_batch_run: job 7 window [%d, +%d)" % (first, N), "not inside the stream's resident samples [%d, %d)" % (t.G, t.G + TRK_PUSH)):
            batches[0].run(TRK_EPOCHS, bad)
    # a block input is checked the same way
    d = torch.from_numpy(raw[:2 * N].view(np.float32).copy()).cuda()
    lin = gnsscorr.TrackingBatch(gctx, 1, 3, L)
    lin.set_code(0, codes[0], SHIFTS)
    lin.set_input_dev(0, d.data_ptr(), 2 * N)
    with _refused(gnsscorr.GC_ERR_INVALID, "gc_trk_batch_run: job 0 window", "exceeds the channel's %d samples" % (2 * N)):
        lin.run(1, gnsscorr.epoch_params_array([[gnsscorr.epoch_params(U64 - 5, 0.0, 0.0, 0.0, 0.25, N)]]))
    lin.close()
    # a read floor above the head protects nothing: refused, for run_dev (which has nothing else to go by)
    # (the device records are those of the second push, whose windows the valid calls below read)
    d_recs = [torch.from_numpy(_records(gnsscorr, base, rel[1], args[1]).view(np.uint8).copy()).cuda() for base in (t.G, t.lead)]
    d_out = [torch.zeros(2 * TRK_EPOCHS * 3, 2, device="cuda", dtype=torch.float32) for _ in range(2)]
    stream = torch.cuda.Stream()
    for floor in (t.G + TRK_PUSH + 1, U64 - 2, 1 << 63):
        batches[0].set_read_floor(floor)
        with _refused(gnsscorr.GC_ERR_INVALID, "gc_trk_batch_run", "read floor %d lies above" % floor, "[%d, %d)" % (t.G, t.G + TRK_PUSH)):
            batches[0].run_dev(TRK_EPOCHS, d_recs[0].data_ptr(), d_out[0].data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert not d_out[0].any()  # nothing was enqueued for the refused requests
    # the push that a floor above the head would not have held back; a floor below the resident range is refused as ever; then the
    # valid calls, floor at the start of the second push, give the twin's bytes
    t.push(raw[TRK_PUSH:2 * TRK_PUSH])
    assert t.ring.info()[0] > t.G
    batches[0].set_read_floor(t.G)
    with _refused(gnsscorr.GC_ERR_STATE, "fell behind"):
        batches[0].run_dev(TRK_EPOCHS, d_recs[0].data_ptr(), d_out[0].data_ptr(), stream.cuda_stream)
    for b, base, dr, do in zip(batches, (t.G, t.lead), d_recs, d_out):
        b.set_read_floor(base + TRK_PUSH)
        b.run_dev(TRK_EPOCHS, dr.data_ptr(), do.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert _same_bytes(d_out[0].cpu().numpy(), d_out[1].cpu().numpy()) and d_out[0].any()
    outs = [b.run(TRK_EPOCHS, _records(gnsscorr, base, rel[1], args[1])) for b, base in zip(batches, (t.G, t.lead))]
    assert _same_bytes(outs[0], outs[1])
    worst = max(rel_err(outs[0][ch, e], want[1, ch, e], 1) for ch in range(2) for e in range(TRK_EPOCHS))
    assert worst <= TRK_TOL
    for b in batches:
        b.close()
    t.finish()


def test_acquisition_and_fine_doppler_refuse_blocks_that_pass_2_64(gctx):
    import gnsscorr
    import fine_doppler_cases as fc
    import fine_doppler_ref as ref
    import test_acq_engine_kinds_gpu as ek
    from test_fine_doppler_gpu import engine
    raw, x = _acq_stream()
    t = Twins(gctx, "acquisition", "2^40+12345")
    t.push(raw[:1700])
    head = t.G + 1700
    for kind, entry in (("plain", "gc_acq_dwell_stream"), ("quicksync", "gc_acq_dwell_stream"), ("tong", "gc_acq_tong_search_stream")):
        engines = [ek.engine(gctx, kind) for _ in range(2)]
        for acq in engines:
            ek.set_codes(acq, kind)
        B = engines[0].consumed_samples
        n = 3 if kind == "tong" else 1

        def search(acq, ring, first):
            if kind == "tong":
                res, st = acq.tong_search_stream(ring, first, 3)
                return res, [(s.state, s.tong_count, s.dwell_count) for s in st]
            return acq.dwell_stream(ring, first), None
        for first in (U64 - 1, U64 - n * B, U64 - n * B + 1, U64 - B // 2, (1 << 63) + t.G, head - n * B + 1, head):
            with _refused(gnsscorr.GC_ERR_INVALID, entry + ": blocks [%d, +%d)" % (first, n * B), "not inside the stream's resident samples [%d, %d)" % (t.G, head)):
                search(engines[0], t.ring, first)
        # the refused requests left nothing behind: the valid call gives the bytes of the twin's engine, which saw none of them
        got, st = search(engines[0], t.ring, t.G + 101)
        twin, st_twin = search(engines[1], t.twin, t.lead + 101)
        assert _acq_bits(engines[0], got) == _acq_bits(engines[1], twin) and st == st_twin and np.any(engines[0].grid(0))
        for acq in engines:
            acq.close()
    t.finish()
    blk = fc.block(2000, 1, 1)
    t = Twins(gctx, "fine-doppler", "2^40+12345")
    t.push(blk.x[:2000])
    t.push(blk.x[:700])
    head = t.G + 2700
    fds = [engine(gctx, blk, ref.EXACT) for _ in range(2)]
    for first in (U64 - 1, U64 - 2000, U64 - 1999, U64 - 1000, (1 << 63) + t.G, head - 1999, head):
        with _refused(gnsscorr.GC_ERR_INVALID, "gc_fine_doppler_estimate_stream: block [%d, +2000)" % first, "not inside the stream's resident samples [%d, %d)" % (t.G, head)):
            fds[0].estimate_stream(t.ring, first, blk.requests)
    got = fds[0].estimate_stream(t.ring, t.G, blk.requests)
    twin = fds[1].estimate_stream(t.twin, t.lead, blk.requests)
    assert [fc.result_bits(r) for r in got] == [fc.result_bits(r) for r in twin]
    assert [fds[0].spectrum(i).tobytes() for i in range(6)] == [fds[1].spectrum(i).tobytes() for i in range(6)]
    for r, rec in zip(got, fc.records(blk, ref.EXACT)):
        assert r.bin == rec.bin
    for fd in fds:
        fd.close()
    t.finish()
