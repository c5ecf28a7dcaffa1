"""The schedules of the ring contract tests (tests/test_ring_contract_gpu.py on the device, tests/test_ring_model.py on the CPU): how
many outputs each call of a producer appends to a small odd ring, chosen so that the contiguous pieces the ring cuts them into
reach every piece class below, and how those output counts translate into the raw input of each producer.

Piece classes (pos, len: ring position and length of a piece; W = max_window; tile: the stage's largest tile of outputs -- 256 for
the conditioner at these sizes, 64-256 for the ring decimator and the resampler, 256 for the notch stage, 1024 for the generator):

  A             pos 0, len > W + 2 tiles: tiles that lie wholly behind the mirror part
  B             pos 0, odd len, ends inside the mirror part
  C             odd pos inside the mirror part, ends inside it
  D_even/D_odd  starts inside the mirror part, ends beyond it; the mirror part of the piece has even / odd length
  E             odd pos, ends exactly at an odd capacity
  F_*           one sample at capacity - 1, 0, W - 1, W
  G             one call of more than capacity outputs (where the stage accepts that)
  H             at least three wraps
"""
import bisect

import numpy as np

import ring_model

CAPACITY, WINDOW = 3001, 96
TILE = dict(host=1, conditioner=256, decimator=256, resampler=256, notch=256, siggen=1024)

# outputs per call; heads 45, 66, 166, 3000, 3001, 3002, 3096, 3097, 3098, 6002, 8502, 9502, 12055, 12125, 15625
INCREMENTS = [45, 21, 100, 2834, 1, 1, 94, 1, 1, 2904, 2500, 1000, 2553, 70, 3500]
# gc_stream_push and the conditioner refuse a call of more than capacity outputs: the last one in two
INCREMENTS_NO_G = INCREMENTS[:-1] + [3001, 499]
# GC_RAW_REAL_2BIT takes whole bytes, 4 raw samples, per push; with D = 3 the heads H = 1 (mod 4) have no raw count that is a
# multiple of 4 in [3 H - 2, 3 H], 3001 among them.  No head below is 1 (mod 4); the one-sample pieces at capacity - 1 and 0 come
# from a call of 2 that the wrap cuts, those at W - 1 and W in the fourth lap (heads 9098 -> 9099 -> 9100)
INCREMENTS_2BIT = [47, 19, 100, 2834, 2, 94, 2906, 2500, 501, 95, 1, 1, 2904, 51, 71, 3001, 499]

# The notch stage (and a conditioner with pulse blanking at D = 1) appends whole segments of L samples: calls in SEGMENTS.  An odd
# capacity does not divide by L, so the wrap still cuts segments, and its pieces start at 0 with any length and end at the capacity
# from any position.  With L = 33 and capacity 3001 every such cut falls on even positions for the first 16 laps (lap n leaves
# 2 n samples of the cut segment behind the wrap, and the part in front of it starts at 2968 + 2 n): that case takes capacity
# 3011, where the first cut is (3003, 8), (0, 25).
SEGMENTS = {32: [70, 23, 1, 2, 1, 90, 1, 2, 1, 96], 33: [70, 21, 1, 1, 2, 87, 1, 2, 1, 92]}
SEGMENT_CAPACITY = {32: 3001, 33: 3011}
# a conditioner refuses more than capacity outputs per push: the last call in two
SEGMENTS_NO_G_32 = SEGMENTS[32][:-1] + [93, 3]

ALL = frozenset(ring_model.CLASSES)
# One-sample pieces of a stage that appends whole segments exist only where the wrap cuts a segment one sample from its end, at
# capacity - 1 or 0 and never at W - 1 or W; the first such cut comes in the ninth lap for L = 32 (32 k = 3000 (mod 3001) first at
# k = 844), beyond the 16384 samples of the scenes the notch tests share.
SEGMENT_CLASSES = ALL - {"F_capacity-1", "F_0", "F_window-1", "F_window"}
REQUIRED = {
    "host": ALL - {"G"},              # gc_stream_push: at most capacity samples per call
    "conditioner": ALL - {"G"},       # gc_conditioner_push: at most capacity outputs per call
    "conditioner-2bit": ALL - {"G"},
    "conditioner-blanking": SEGMENT_CLASSES - {"G"},
    "decimator": ALL,
    "resampler-down": ALL,
    "resampler-up": ALL,
    "resampler-polyphase": ALL,
    "notch-32": SEGMENT_CLASSES,
    "notch-33": SEGMENT_CLASSES,
    "siggen": ALL,
}
DIRECT_DOWN = (25e6, 10e6)
DIRECT_UP = (4e6, 5e6)
POLYPHASE = (25e6, 10e6, 32)  # fs_in, fs_out, phases of gc_resampler_design


def heads(increments):
    return [int(h) for h in np.cumsum(increments)]


def classes(increments, capacity, window, tile):
    """The classes the calls reach, through the model's own cut."""
    m = ring_model.RingModel(capacity, window, np.int8)
    for n in increments:
        m.append(np.zeros(n, np.int8))
    return ring_model.classify(m.pieces, m.calls, capacity, window, tile)


def fir_raw_heads(out_heads, decimation, multiple=1):
    """Raw samples pushed so far that make ceil(raw / D) = H outputs, for each head H: the smallest such count, or with `multiple`
    the largest one that is a multiple of it (GC_RAW_REAL_2BIT: 4)."""
    D = int(decimation)
    raw = []
    for H in out_heads:
        r = (H - 1) * D + 1 if multiple == 1 else H * D // multiple * multiple
        assert (r + D - 1) // D == H, "no raw count that is a multiple of %d makes %d outputs at D = %d" % (multiple, H, D)
        raw.append(r)
    return raw


def fir_out_heads(raw_heads, decimation, segment=1):
    """ceil(decided / D), decided = raw for a conditioner or a ring decimator, whole segments of `segment` raw samples with pulse
    blanking."""
    D = int(decimation)
    return [(r // segment * segment + D - 1) // D for r in raw_heads]


def source_heads(available, out_heads, limit=1 << 20):
    """The smallest source head h with available(h) = H for each H (available: non-decreasing).  A head that an up-ratio skips
    is an error."""
    class _Seq:
        def __len__(self):
            return limit

        def __getitem__(self, h):
            return available(h)
    seq = _Seq()
    src = []
    for H in out_heads:
        h = bisect.bisect_left(seq, H)
        assert available(h) == H, "no source head completes exactly %d outputs (%d gives %d)" % (H, h, available(h))
        src.append(h)
    return src


def segment_raw_heads(segments, length, ragged=5):
    """Source samples pushed so far for a stage that appends whole segments: each call's segments and `ragged` samples of the next."""
    return [h * length + ragged for h in heads(segments)]


def tile_pushes(want_groups, window=128):
    """The conditioner's tiles of 512 and 1024 outputs (R = 2, 4) are chosen only for pieces of about want_groups * 512 and * 1024
    outputs (cond_tile_outputs; want_groups = 2 x compute units).  Returns (capacity, window, outputs per push, n2, n4) for D = 1:
    each of the two sizes occurs once as a piece at position 0 and once at an odd position at or beyond the window."""
    n2, n4 = (want_groups - 1) * 512 + 37, (want_groups - 1) * 1024 + 37
    capacity = 301 + n4
    pushes = [n4, 301, n2, n2, capacity - 2 * n2, 129, n4]
    return capacity, window, pushes, n2, n4
