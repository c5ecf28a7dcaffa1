"""Host model of the storage of a gc_stream ring (gnss-sdr-1_amd/csrc/gc_stream.hip), byte for byte: `capacity` samples of ring,
the mirror of its first `max_window` samples, and SLACK samples that nothing writes -- zero at first, as the library's.  Pure numpy;
test infrastructure only.

append(samples) is one call of a producer.  A call of more than `capacity` samples goes out in runs of at most `capacity` (the
derived rings' update and the signal generator do that; gc_stream_push and the conditioner refuse such a call), each run is
cut at the wrap as gc_stream_produce cuts it, and each piece (pos, len) is written to pos .. pos + len and, where pos < max_window,
its first min(len, max_window - pos) samples to capacity + pos as well.  Every piece and every call is recorded: classify() says
which of the piece classes a schedule has reached, tests/ring_contract_cases.py names them.

origin: the ring starts at that absolute sample number (gc_stream_debug_set_origin, or the origin a derived stage gives its output
ring) as if `origin` samples had been appended and evicted: the first piece lands at origin % capacity, the storage stays zero, and
resident() is [max(origin, head - capacity), head).  All of it in Python integers, whatever the size of the origin."""
import numpy as np

SLACK = 2
CLASSES = ("A", "B", "C", "D_even", "D_odd", "E", "F_capacity-1", "F_0", "F_window-1", "F_window", "G", "H")


class RingModel:
    def __init__(self, capacity, max_window, dtype, per=1, origin=0):
        """dtype / per: complex64 / 1 for a GC_IQ_F32 ring ([n] arrays), int16 or int8 / 2 for the integer rings ([n, 2])."""
        assert 0 < max_window and 2 * max_window <= capacity and int(origin) >= 0
        self.capacity, self.max_window = int(capacity), int(max_window)
        self.total = self.capacity + self.max_window + SLACK
        self.storage = np.zeros(self.total if per == 1 else (self.total, per), dtype)
        self.origin = int(origin)
        self.head = self.origin
        self.pieces = []  # (pos, len) of every contiguous piece, in order
        self.calls = []   # samples of every append

    def append(self, samples):
        samples = np.asarray(samples)
        assert samples.dtype == self.storage.dtype and samples.shape[1:] == self.storage.shape[1:], (samples.dtype, samples.shape)
        self.calls.append(len(samples))
        for first in range(0, len(samples), self.capacity):
            self._produce(samples[first:first + self.capacity])

    def _produce(self, samples):
        done = 0
        while done < len(samples):
            pos = self.head % self.capacity
            n = min(len(samples) - done, self.capacity - pos)
            piece = samples[done:done + n]
            self.storage[pos:pos + n] = piece
            if pos < self.max_window:
                m = min(n, self.max_window - pos)
                self.storage[self.capacity + pos:self.capacity + pos + m] = piece[:m]
            self.pieces.append((pos, n))
            self.head += n
            done += n

    def resident(self):
        """(oldest, head) as gc_stream_info reports them."""
        return max(self.origin, self.head - self.capacity), self.head

    def position(self, index):
        """Storage position of the absolute sample number `index`."""
        return int(index) % self.capacity

    def region(self, position):
        return "ring" if position < self.capacity else "mirror" if position < self.capacity + self.max_window else "slack"

    def first_difference(self, got):
        """None when `got` (the whole storage as read back) equals the model's bytes; else (position, region, got, want) of the
        first storage position that differs."""
        got = np.asarray(got)
        assert got.dtype == self.storage.dtype and got.shape == self.storage.shape, (got.dtype, got.shape, self.storage.shape)
        a = got.reshape(self.total, -1).view(np.uint8).reshape(self.total, -1)
        b = self.storage.reshape(self.total, -1).view(np.uint8).reshape(self.total, -1)
        bad = np.flatnonzero(np.any(a != b, axis=1))
        if bad.size == 0:
            return None
        p = int(bad[0])
        return p, self.region(p), got[p].tolist(), self.storage[p].tolist()


def classify(pieces, calls, capacity, max_window, tile):
    """The piece classes a schedule reaches (tests/ring_contract_cases.py describes them); tile: the stage's largest tile."""
    got = set()
    for pos, n in pieces:
        end = pos + n
        if pos == 0 and n > max_window + 2 * tile:
            got.add("A")
        if pos == 0 and n % 2 == 1 and end < max_window:
            got.add("B")
        if pos % 2 == 1 and pos < max_window and end < max_window:
            got.add("C")
        if 0 < pos < max_window < end:
            got.add("D_even" if (max_window - pos) % 2 == 0 else "D_odd")
        if pos % 2 == 1 and end == capacity and capacity % 2 == 1:
            got.add("E")
        if n == 1:
            for name, at in (("F_capacity-1", capacity - 1), ("F_0", 0), ("F_window-1", max_window - 1), ("F_window", max_window)):
                if pos == at:
                    got.add(name)
    if any(n > capacity for n in calls):
        got.add("G")
    if sum(n for _, n in pieces) >= 3 * capacity:
        got.add("H")
    return got
