"""Case table of the origin tests (tests/test_ring_origin_gpu.py): rings that start at the sample numbers of a stream that has been
running for minutes and hours (IqStream.set_origin, gc_stream_debug_set_origin), read by every ring reader and by the two
index-driven ring stages.  Pure Python integers; test infrastructure only.

Origins, per case with its own odd `a` of about half the case's first window or block, so that the boundary falls INSIDE a correlated
window or an acquisition block, not between two:

    2^31 - a      the first absolute index that does not fit in 31 bits lies inside the first window
    2^32 - a      the same for 32 bits
    2^40 + 12345  a pure cast detector: 32-bit truncation anywhere puts an index 2^40 samples away
    2^53 + 1      a pure cast detector: odd and not representable in a double, so an index that passes through double / float, or
                  through NumPy's uint64 + int promotion (float64) in the Python layer, comes out even

What the table asserts about itself (check(), at import and in tests/test_ring_origin_ref.py), so that no case hides the failure it
is for: no capacity divides 2^31 or 2^32 -- with a power-of-two capacity a truncated index lands on the right position --; for the
two boundary origins origin < boundary < origin + samples pushed; every streaming case wraps its ring at least twice behind the
origin."""

ORIGIN_NAMES = ("2^31-a", "2^32-a", "2^40+12345", "2^53+1")
BOUNDARY = {"2^31-a": 1 << 31, "2^32-a": 1 << 32}
STAGE_ORIGIN_NAMES = ("2^32-a", "2^40+12345")


def origin(name, a):
    assert a % 2 == 1
    return {"2^31-a": (1 << 31) - a, "2^32-a": (1 << 32) - a, "2^40+12345": (1 << 40) + 12345, "2^53+1": (1 << 53) + 1}[name]


# name -> capacity: samples in the ring; window: its max_window; first: the first window or block (samples); a: see above;
#         pushed: samples pushed behind the origin; streaming: the case pushes on while it reads
CASES = {
    # TrackingBatch: 4 Msps, N = 4000, L = 1023; four pushes of 6 N + 7 samples, six epochs of two channels after each
    "tracking": dict(capacity=26003, window=4000, first=4000, a=2001, pushed=4 * (6 * 4000 + 7), streaming=True),
    # TrackingLoop on a ring: one code period is 4000 samples, 6500 per push, 43 periods
    "loop": dict(capacity=24001, window=4000, first=4000, a=2001, pushed=43 * 4000, streaming=True),
    # the mixed loop: GPS L1 C/A (4000) and Galileo E1 (16000 per period), 10 ms per push
    "loop-mixed": dict(capacity=100003, window=20000, first=4000, a=2001, pushed=17 * 40000, streaming=True),
    # acquisition: 500 samples per block (QuickSync: 1000), tests/test_acq_engine_kinds_gpu.py's engines
    "acquisition": dict(capacity=2203, window=1000, first=500, a=251, pushed=10900, streaming=True),
    "acquisition-quicksync": dict(capacity=2203, window=1000, first=1000, a=501, pushed=10900, streaming=True),
    # fine Doppler: (N, P, Z) = (2000, 1, 1), a block of 2000 samples, longer than the ring's max_window
    "fine-doppler": dict(capacity=5003, window=256, first=2000, a=1001, pushed=5 * 5003, streaming=True),
    # IqStream.read / info / read_storage alone
    "stream": dict(capacity=3001, window=96, first=96, a=49, pushed=3 * 3001 + 5, streaming=True),
    # the sources of the ring decimator and of the ring resampler (the output rings take tests/ring_contract_cases.py's shape)
    # (a = 153: neither stage origin is then a multiple of the decimations 2 and 3)
    "stage-source": dict(capacity=6007, window=64, first=305, a=153, pushed=3 * 6007, streaming=True),
}
# the output rings of the two stages
STAGE_OUT_CAPACITY, STAGE_OUT_WINDOW = 3001, 96


def lead(g, capacity):
    """Samples of unrelated noise the small-index twin (a ring at origin 0) receives first: every later sample then lies at the
    same storage position in both rings, mirror included."""
    return int(g) % int(capacity)


def check():
    for case, c in CASES.items():
        C = c["capacity"]
        assert (1 << 31) % C != 0 and (1 << 32) % C != 0 and C & (C - 1) != 0, case
        assert 2 * c["window"] <= C
        assert c["a"] % 2 == 1 and abs(2 * c["a"] - c["first"]) <= 2, case
        for name in ORIGIN_NAMES:
            g = origin(name, c["a"])
            assert g <= 1 << 62
            if name in BOUNDARY:
                assert g < BOUNDARY[name] < g + c["first"] <= g + c["pushed"], (case, name)
            # a truncated index must not fall on the right position by accident
            assert g % C != (g & 0xffffffff) % C or g < (1 << 32), (case, name)
            assert g % C != (g & 0x7fffffff) % C or g < (1 << 31), (case, name)
        if c["streaming"]:
            assert c["pushed"] >= 2 * C, case
    assert (1 << 31) % STAGE_OUT_CAPACITY != 0 and (1 << 32) % STAGE_OUT_CAPACITY != 0
    assert origin("2^53+1", 1) % 2 == 1 and int(float(origin("2^53+1", 1))) != origin("2^53+1", 1)


check()
