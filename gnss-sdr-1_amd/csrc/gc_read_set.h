// gc_read_set.h -- the ring reads of one launch, released on every way out.
//
// A launch that reads stream rings reserves a reader slot on each of them (gc_reader_table.h) before its residency check and
// commits the slots behind its enqueue.  In between nothing may return without releasing them: a slot left `pending` blocks every
// later push that would evict below its floor, and the drain of the ring's teardown, for ever.  The set holds the tickets of one
// launch on the distinct rings it reads: add() reserves, commit() registers the enqueued launch on all of them, and the destructor
// cancels whatever was not committed -- an early return needs no clean-up of its own.
//
// Header-only and templated on the ring operations so that every exit path runs on the CPU (tests/read_set_selftest.cpp);
// gc_stream.h instantiates it for gc_stream.  Ops supplies ring_t, stream_t, ticket_t, FLOOR_OLDEST,
// begin(ring, stream, floor, &ticket), end(ring, stream, ticket), cancel(ring, ticket) and too_many_rings(bound).
// The tickets live in a fixed array (no allocation per launch): a launch reads at most MAX_RINGS distinct rings, add() answers
// Ops::too_many_rings (GC_ERR_INVALID) beyond that.
#ifndef GC_READ_SET_H
#define GC_READ_SET_H
#include "gnsscorr.h"
#include <cstdint>

template <class Ops, int MaxRings = 16>
class gc_read_set
{
public:
    typedef typename Ops::ring_t ring_t;
    typedef typename Ops::stream_t stream_t;
    typedef typename Ops::ticket_t ticket_t;
    static constexpr int MAX_RINGS = MaxRings;

    // `compute`: the stream the launch is enqueued on
    explicit gc_read_set(stream_t compute) : compute_(compute) {}
    gc_read_set(const gc_read_set&) = delete;
    gc_read_set& operator=(const gc_read_set&) = delete;
    ~gc_read_set()
    {
        for (int k = 0; k < n_; k++) Ops::cancel(ring_[k], ticket_[k]);
    }

    // Reserves a read of `ring` from `floor` on (Ops::FLOOR_OLDEST: from the oldest resident sample).  A ring that is already in
    // the set keeps one ticket with the lower of the floors, FLOOR_OLDEST below any of them: the lower reservation is taken first,
    // then the earlier one is given back.  On an error the set holds what it held before.
    gc_status add(ring_t* ring, uint64_t floor)
    {
        const int k = find(ring);
        if (k >= 0 && !below(floor, floor_[k])) return GC_OK;
        if (k < 0 && n_ == MaxRings) return Ops::too_many_rings(MaxRings);
        ticket_t t;
        const gc_status s = Ops::begin(ring, compute_, floor, &t);
        if (s != GC_OK) return s;
        const int at = k >= 0 ? k : n_++;
        if (k >= 0) Ops::cancel(ring, ticket_[k]);
        ring_[at] = ring;
        floor_[at] = floor;
        ticket_[at] = t;
        return GC_OK;
    }

    int size() const { return n_; }
    // index of `ring` in the set (order of the first add), or -1
    int find(const ring_t* ring) const
    {
        for (int k = 0; k < n_; k++)
            if (ring_[k] == ring) return k;
        return -1;
    }
    // the resident range as of the reservation (by ring: the ring must be in the set)
    const ticket_t& ticket(int k) const { return ticket_[k]; }
    const ticket_t& ticket(const ring_t* ring) const { return ticket_[find(ring)]; }

    // The launch has been enqueued: registers it on every ring (all of them are attempted) and returns the first error.
    gc_status commit()
    {
        gc_status out = GC_OK;
        for (int k = 0; k < n_; k++)
            {
                const gc_status s = Ops::end(ring_[k], compute_, ticket_[k]);
                if (s != GC_OK && out == GC_OK) out = s;
            }
        n_ = 0;
        return out;
    }

private:
    static_assert(Ops::FLOOR_OLDEST == ~0ull, "below() orders floors by floor + 1");
    static bool below(uint64_t a, uint64_t b) { return a + 1 < b + 1; }  // FLOOR_OLDEST (~0) + 1 wraps to 0: below every floor

    stream_t compute_;
    int n_ = 0;
    ring_t* ring_[MaxRings];
    uint64_t floor_[MaxRings];
    ticket_t ticket_[MaxRings];
};

#endif
