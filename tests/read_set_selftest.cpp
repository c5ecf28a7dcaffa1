// read_set_selftest.cpp -- every exit path of a launch's ring reads (gnss-sdr-1_amd/csrc/gc_read_set.h) on the host, with a fake ring
// that counts begin / end / cancel per ticket and fails the k-th begin or the k-th end on request.  After every scenario each ticket
// that was begun has been ended or cancelled exactly once, never both.  CPU only; built and run by tests/test_read_set.py.
#include "gc_read_set.h"
#include <cstdio>
#include <vector>

struct FakeTicket
{
    int id = -1;
    uint64_t floor = 0;
};
struct FakeRing
{
    int name;
};
struct Counts
{
    int ended = 0, cancelled = 0;
};
static std::vector<Counts> g_tickets;  // one entry per successful begin
static int g_begins = 0, g_ends = 0;   // calls, failed ones included
static int g_fail_begin = 0, g_fail_end = 0;  // 1-based call to fail (0: none)

struct FakeOps
{
    typedef FakeRing ring_t;
    typedef int stream_t;
    typedef FakeTicket ticket_t;
    static constexpr uint64_t FLOOR_OLDEST = ~0ull;
    static gc_status begin(FakeRing*, int, uint64_t floor, FakeTicket* t)
    {
        if (++g_begins == g_fail_begin) return GC_ERR_STATE;
        t->id = (int)g_tickets.size();
        t->floor = floor;
        g_tickets.push_back(Counts());
        return GC_OK;
    }
    static gc_status end(FakeRing*, int, const FakeTicket& t)
    {
        g_tickets[t.id].ended++;  // a failed end has still released the slot (gc_reader_table::commit)
        return ++g_ends == g_fail_end ? GC_ERR_HIP : GC_OK;
    }
    static void cancel(FakeRing*, const FakeTicket& t) { g_tickets[t.id].cancelled++; }
    static gc_status too_many_rings(int) { return GC_ERR_INVALID; }
};
typedef gc_read_set<FakeOps, 4> Set;

static int g_failures = 0;
#define CHECK(cond)                                                      \
    do                                                                   \
        {                                                                \
            if (!(cond))                                                 \
                {                                                        \
                    std::printf("line %d: %s\n", __LINE__, #cond);       \
                    g_failures++;                                        \
                }                                                        \
        }                                                                \
    while (0)

static void reset(int fail_begin = 0, int fail_end = 0)
{
    g_tickets.clear();
    g_begins = g_ends = 0;
    g_fail_begin = fail_begin;
    g_fail_end = fail_end;
}
// every ticket released exactly once; the totals of the scenario
static void released(int line, size_t n_tickets, int n_ended, int n_cancelled)
{
    int e = 0, c = 0;
    bool once = true;
    for (const Counts& t : g_tickets)
        {
            once = once && t.ended + t.cancelled == 1;
            e += t.ended;
            c += t.cancelled;
        }
    if (!once || g_tickets.size() != n_tickets || e != n_ended || c != n_cancelled)
        {
            std::printf("line %d: %zu tickets, %d ended, %d cancelled, each once: %d\n", line, g_tickets.size(), e, c, (int)once);
            g_failures++;
        }
}

int main()
{
    FakeRing r[5] = {{0}, {1}, {2}, {3}, {4}};
    // commit of 0, 1 and 3 rings
    for (int n : {0, 1, 3})
        {
            reset();
            {
                Set s(0);
                for (int k = 0; k < n; k++) CHECK(s.add(&r[k], 100 + k) == GC_OK);
                CHECK(s.size() == n);
                for (int k = 0; k < n; k++) CHECK(s.find(&r[k]) == k && s.ticket(k).floor == 100u + k && s.ticket(&r[k]).id == s.ticket(k).id);
                CHECK(s.find(&r[4]) == -1);
                CHECK(s.commit() == GC_OK);
            }  // the destructor after a commit releases nothing again
            released(__LINE__, n, n, 0);
        }
    // the same ring twice with two floors, in both orders: one ticket, the lower floor
    for (int order = 0; order < 2; order++)
        {
            reset();
            {
                Set s(0);
                CHECK(s.add(&r[0], order ? 50 : 70) == GC_OK);
                CHECK(s.add(&r[0], order ? 70 : 50) == GC_OK);
                CHECK(s.size() == 1 && s.ticket(0).floor == 50);
                CHECK(s.commit() == GC_OK);
            }
            // the higher floor first: the lower reservation replaces it (2 begun, 1 cancelled); the lower first: nothing to do
            released(__LINE__, order ? 1 : 2, 1, order ? 0 : 1);
        }
    // a floor and "oldest", in both orders: one ticket at "oldest"
    for (int order = 0; order < 2; order++)
        {
            reset();
            {
                Set s(0);
                CHECK(s.add(&r[0], order ? FakeOps::FLOOR_OLDEST : 70) == GC_OK);
                CHECK(s.add(&r[0], order ? 70 : FakeOps::FLOOR_OLDEST) == GC_OK);
                CHECK(s.add(&r[0], FakeOps::FLOOR_OLDEST) == GC_OK);
                CHECK(s.size() == 1 && s.ticket(0).floor == FakeOps::FLOOR_OLDEST);
                CHECK(s.commit() == GC_OK);
            }
            released(__LINE__, order ? 1 : 2, 1, order ? 0 : 1);
        }
    // a failing begin on the 2nd of 3 rings: the caller returns, the first ticket is cancelled once, nothing is ended
    reset(2);
    {
        Set s(0);
        CHECK(s.add(&r[0], 1) == GC_OK);
        CHECK(s.add(&r[1], 2) == GC_ERR_STATE);
        CHECK(s.size() == 1 && s.find(&r[1]) == -1);
    }
    released(__LINE__, 1, 0, 1);
    CHECK(g_ends == 0);
    // a failing begin of the lower floor of a ring that is in the set: the earlier ticket stays, and is committed
    reset(2);
    {
        Set s(0);
        CHECK(s.add(&r[0], 70) == GC_OK);
        CHECK(s.add(&r[0], 50) == GC_ERR_STATE);
        CHECK(s.size() == 1 && s.ticket(0).floor == 70);
        CHECK(s.commit() == GC_OK);
    }
    released(__LINE__, 1, 1, 0);
    // scope left without a commit: all tickets cancelled once
    reset();
    {
        Set s(0);
        for (int k = 0; k < 3; k++) CHECK(s.add(&r[k], k) == GC_OK);
    }
    released(__LINE__, 3, 0, 3);
    // a failing end in the middle: every ticket still ended exactly once, nothing cancelled, the first error returned
    reset(0, 2);
    {
        Set s(0);
        for (int k = 0; k < 3; k++) CHECK(s.add(&r[k], k) == GC_OK);
        CHECK(s.commit() == GC_ERR_HIP);
    }
    released(__LINE__, 3, 3, 0);
    CHECK(g_ends == 3);
    // more rings than the bound: refused before anything is reserved, the set keeps what it held; a ring that is in the set
    // can still lower its floor
    reset();
    {
        Set s(0);
        for (int k = 0; k < Set::MAX_RINGS; k++) CHECK(s.add(&r[k], 10 + k) == GC_OK);
        CHECK(s.add(&r[4], 0) == GC_ERR_INVALID);
        CHECK(g_begins == Set::MAX_RINGS && s.size() == Set::MAX_RINGS);
        CHECK(s.add(&r[3], 5) == GC_OK && s.ticket(3).floor == 5);
        CHECK(s.commit() == GC_OK);
    }
    released(__LINE__, Set::MAX_RINGS + 1, Set::MAX_RINGS, 1);
    std::printf("%d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
