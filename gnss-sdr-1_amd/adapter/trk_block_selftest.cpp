// trk_block_selftest -- what the tracking blocks, groups and adapters share (tracking_block_base.h, tracking_signals.h,
// tracking_adapter_base.h), without a GPU:
//   - walk_records under both policies against the four loops it replaced (veml / GLONASS, block / group; copied below), on canned
//     records: items field by field, position, state, last record, events, the slot's active flag;
//   - ring_feed_fresh and the two launch sizes against the lines they replaced;
//   - every field of every row of the signal table against the three tables it replaced (copied below), and trk_generate_replicas
//     bit for bit against the generator calls it replaced;
//   - every adapter's implementation() and item_size(), and every Dll_Pll_Conf field the veml adapters derive, under the default
//     configuration and under one that exercises the clamps, against the constructor they had (copied below);
//   - the real device-loop blocks and groups without a device: the construction status, start_tracking, standby, run().
// Creates no GPU context: run it with no device visible (tests/test_trk_block_base.py hides them).
#include "dll_pll_tracking_adapters.h"
#include "hip_glonass_tracking_group.h"
#include "hip_gps_l1_ca_dll_pll_c_aid_tracking.h"
#include "hip_tracking_group.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT(cond, ...)                                            \
    do                                                               \
        {                                                            \
            if (!(cond))                                             \
                {                                                    \
                    std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                    std::printf(__VA_ARGS__);                        \
                    std::printf("\n");                               \
                    g_fail++;                                        \
                }                                                    \
        }                                                            \
    while (0)

static bool same_synchro(const Gnss_Synchro& a, const Gnss_Synchro& b)
{
    return a.System == b.System && std::memcmp(a.Signal, b.Signal, 3) == 0 && a.PRN == b.PRN && a.Channel_ID == b.Channel_ID && a.Acq_delay_samples == b.Acq_delay_samples &&
           a.Acq_doppler_hz == b.Acq_doppler_hz && a.Acq_samplestamp_samples == b.Acq_samplestamp_samples && a.Acq_doppler_step == b.Acq_doppler_step &&
           a.Flag_valid_acquisition == b.Flag_valid_acquisition && a.fs == b.fs && a.Prompt_I == b.Prompt_I && a.Prompt_Q == b.Prompt_Q && a.CN0_dB_hz == b.CN0_dB_hz &&
           a.Carrier_Doppler_hz == b.Carrier_Doppler_hz && a.Carrier_phase_rads == b.Carrier_phase_rads && a.Code_phase_samples == b.Code_phase_samples &&
           a.Tracking_sample_counter == b.Tracking_sample_counter && a.Flag_valid_symbol_output == b.Flag_valid_symbol_output && a.correlation_length_ms == b.correlation_length_ms &&
           a.Flag_valid_word == b.Flag_valid_word && a.TOW_at_current_symbol_ms == b.TOW_at_current_symbol_ms && a.Pseudorange_m == b.Pseudorange_m && a.RX_time == b.RX_time &&
           a.Flag_valid_pseudorange == b.Flag_valid_pseudorange && a.interp_TOW_ms == b.interp_TOW_ms;
}
static bool same_items(const std::vector<Gnss_Synchro>& a, const std::vector<Gnss_Synchro>& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!same_synchro(a[i], b[i])) return false;
    return true;
}

// ---- the record walk ---------------------------------------------------------------------------------------------------------------

// what a walk leaves behind in a block (sample counter, state, last record, events, engine-slot stops) or in a group slot (position,
// active, events, stops)
struct Walked
{
    std::vector<Gnss_Synchro> items;
    uint64_t position = 0;
    int32_t d_state = 0;
    gc_loop_record d_last{};
    std::vector<int> d_events;
    char active = 1;
    int stops = 0;
};
static bool same_walked(const Walked& a, const Walked& b)
{
    return same_items(a.items, b.items) && a.position == b.position && a.d_state == b.d_state && std::memcmp(&a.d_last, &b.d_last, sizeof a.d_last) == 0 && a.d_events == b.d_events &&
           a.active == b.active && a.stops == b.stops;
}

static const gnsscorr::TrkSignalInfo& e5a() { return gnsscorr::trk_signal(gnsscorr::TrkSignal::GALILEO_E5A); }
static const bool kInterchange = true;  // the E5a pilot: every field assignment of synchro_from_record shows
static const double kFs = 4e6;

// step 3 of hip_dll_pll_veml_tracking_dev::work as it was
static void old_veml_block_walk(Walked& w, const std::vector<gc_loop_record>& d_records, int n_periods, const Gnss_Synchro& acq)
{
    uint64_t d_sample_counter = w.position;
    uint64_t position = d_sample_counter;
    for (int k = 0; k < n_periods; k++)
        {
            const gc_loop_record& r = d_records[k];
            if (r.sample_counter == position && r.valid == 0 && r.state >= 2) break;  // nothing was correlated: out of input
            position = r.sample_counter;
            w.d_state = r.state;
            w.d_last = r;
            if (r.valid)
                {
                    const Gnss_Synchro s = gnsscorr::synchro_from_record(r, acq, e5a(), kInterchange, kFs);
                    w.items.push_back(s);
                }
            if (r.state == 0)
                {
                    w.d_events.push_back(3);  // loss of lock (:868)
                    break;
                }
        }
    w.position = position;
}

// step 3 of hip_glonass_ca_dll_pll_tracking_dev::work as it was
static void old_glonass_block_walk(Walked& w, const std::vector<gc_loop_record>& d_records, int n_periods, const Gnss_Synchro& acq)
{
    uint64_t position = w.position;
    for (int k = 0; k < n_periods; k++)
        {
            const gc_loop_record& r = d_records[k];
            if (r.valid == 0) break;  // nothing was correlated: out of input
            position = r.sample_counter;
            w.d_state = r.state;
            w.d_last = r;
            w.items.push_back(gnsscorr::glonass_synchro_from_record(r, acq, static_cast<int64_t>(kFs)));
            if (r.state == 0)
                {
                    w.d_events.push_back(3);  // loss of lock (:741)
                    w.stops++;                // gc_trk_loop_stop(d_loop, 0)
                    break;
                }
        }
    w.position = position;
}

// the slot loop of hip_tracking_group::run as it was
static void old_veml_group_walk(Walked& w, const std::vector<gc_loop_record>& d_records, int n_periods, const Gnss_Synchro& acq)
{
    uint64_t position = w.position;
    for (int k = 0; k < n_periods; k++)
        {
            const gc_loop_record& r = d_records[k];
            if (r.sample_counter == position && r.valid == 0 && r.state >= 2) break;  // out of input
            position = r.sample_counter;
            if (r.valid)
                {
                    w.items.push_back(gnsscorr::synchro_from_record(r, acq, e5a(), kInterchange, kFs));
                }
            if (r.state == 0)
                {
                    w.d_events.push_back(3);  // loss of lock: the slot is free for the next acquisition
                    w.active = 0;
                    break;
                }
        }
    w.position = position;
}

// the slot loop of hip_glonass_tracking_group::run as it was
static void old_glonass_group_walk(Walked& w, const std::vector<gc_loop_record>& d_records, int n_periods, const Gnss_Synchro& acq)
{
    uint64_t position = w.position;
    for (int k = 0; k < n_periods; k++)
        {
            const gc_loop_record& r = d_records[k];
            if (r.valid == 0) break;  // out of input
            position = r.sample_counter;
            w.items.push_back(gnsscorr::glonass_synchro_from_record(r, acq, static_cast<int64_t>(kFs)));
            if (r.state == 0)
                {
                    w.d_events.push_back(3);  // loss of lock: the slot is free for the next acquisition
                    w.active = 0;
                    w.stops++;  // gc_trk_loop_stop(d_loop, ch)
                    break;
                }
        }
    w.position = position;
}

// the shared walk with what hip_device_loop_block::work / hip_loop_group_base::run do with its result
static void new_walk(Walked& w, const gnsscorr::TrkLoopPolicy& policy, bool group, const std::vector<gc_loop_record>& records, int n, const Gnss_Synchro& acq)
{
    const gnsscorr::RecordWalk r = gnsscorr::walk_records(policy, records.data(), n, w.position, [&](const gc_loop_record& rec) {
        w.items.push_back(policy.pull_in_item ? gnsscorr::glonass_synchro_from_record(rec, acq, static_cast<int64_t>(kFs)) : gnsscorr::synchro_from_record(rec, acq, e5a(), kInterchange, kFs));
    });
    if (!group && r.last)
        {
            w.d_state = r.last->state;
            w.d_last = *r.last;
        }
    if (r.lost)
        {
            w.d_events.push_back(3);
            if (group) w.active = 0;
            if (policy.stops_engine_slot) w.stops++;
        }
    w.position = r.position;
}

static gc_loop_record rec(uint64_t counter, int32_t valid, int32_t state, float seed)
{
    gc_loop_record r;
    std::memset(&r, 0, sizeof r);
    r.sample_counter = counter;
    r.valid = valid;
    r.state = state;
    r.prompt_data[0] = 100.0f + seed;
    r.prompt_data[1] = -7.0f - seed;
    r.rem_code_phase_samples = 0.25 + seed;
    r.acc_carrier_phase_rad = -1234.5 - seed;
    r.carrier_doppler_hz = 1500.0f + seed;
    r.code_freq_chips = 1.023e6f + seed;
    r.cn0_db_hz = 44.0f + seed;
    r.carrier_lock_test = 0.9f;
    return r;
}

static void test_record_walk()
{
    const uint64_t P = 1000000;  // where the channel is
    struct Case
    {
        const char* name;
        std::vector<gc_loop_record> records;
        int n;
    };
    const gc_loop_record poison = rec(777, 1, 4, 99.0f);  // behind a loss of lock: never read
    gc_loop_record standby;                                // a stopped engine slot: all zero
    std::memset(&standby, 0, sizeof standby);
    const std::vector<Case> cases = {
        {"n = 0", {rec(P + 4000, 1, 4, 1)}, 0},
        {"all valid", {rec(P + 4000, 1, 4, 1), rec(P + 8001, 1, 4, 2), rec(P + 12001, 1, 2, 3)}, 3},
        {"veml pull-in records", {rec(P + 2345, 0, 1, 1), rec(P + 2345, 0, 1, 2), rec(P + 6345, 1, 2, 3)}, 3},
        {"veml integrating record", {rec(P + 4000, 1, 4, 1), rec(P + 8000, 0, 3, 2), rec(P + 12000, 1, 4, 3)}, 3},
        {"end of input at k = 0", {rec(P, 0, 2, 1), rec(P, 0, 2, 2)}, 2},
        {"end of input at k = 0, integrating", {rec(P, 0, 3, 1)}, 1},
        {"end of input in the middle", {rec(P + 4000, 1, 4, 1), rec(P + 8000, 1, 4, 2), rec(P + 8000, 0, 4, 3), rec(P + 8000, 0, 4, 4)}, 4},
        {"loss of lock in the middle, valid 1", {rec(P + 4000, 1, 4, 1), rec(P + 8000, 1, 0, 2), poison, poison}, 4},
        {"veml loss with valid 0", {rec(P + 4000, 1, 2, 1), rec(P + 8000, 0, 0, 2), poison}, 3},
        {"loss in the last record", {rec(P + 4000, 1, 4, 1), rec(P + 8000, 1, 0, 2)}, 2},
        {"records of a stopped slot", {standby, standby}, 2},
        {"a position that did not move in pull-in", {rec(P, 0, 1, 1), rec(P + 4000, 1, 2, 2)}, 2},
    };
    Gnss_Synchro acq;
    acq.System = 'E';
    acq.Signal[0] = '5';
    acq.Signal[1] = 'X';
    acq.PRN = 11;
    acq.Channel_ID = 3;
    acq.Acq_delay_samples = 123.0;
    acq.Acq_doppler_hz = -250.0;
    acq.Acq_samplestamp_samples = 4242;
    for (const Case& c : cases)
        {
            Walked start;
            start.position = P;
            start.d_state = 1;
            start.d_last = rec(5, 1, 2, 50.0f);
            Walked a = start, b = start;
            old_veml_block_walk(a, c.records, c.n, acq);
            new_walk(b, gnsscorr::kVemlLoopPolicy, false, c.records, c.n, acq);
            EXPECT(same_walked(a, b), "record walk, veml block, %s: %zu / %zu items, position %llu / %llu, state %d / %d", c.name, a.items.size(), b.items.size(),
                (unsigned long long)a.position, (unsigned long long)b.position, a.d_state, b.d_state);
            a = b = start;
            old_glonass_block_walk(a, c.records, c.n, acq);
            new_walk(b, gnsscorr::kGlonassLoopPolicy, false, c.records, c.n, acq);
            EXPECT(same_walked(a, b), "record walk, GLONASS block, %s: %zu / %zu items, position %llu / %llu, state %d / %d", c.name, a.items.size(), b.items.size(),
                (unsigned long long)a.position, (unsigned long long)b.position, a.d_state, b.d_state);
            a = b = start;
            old_veml_group_walk(a, c.records, c.n, acq);
            new_walk(b, gnsscorr::kVemlLoopPolicy, true, c.records, c.n, acq);
            EXPECT(same_walked(a, b), "record walk, veml group, %s: %zu / %zu items, position %llu / %llu, active %d / %d", c.name, a.items.size(), b.items.size(),
                (unsigned long long)a.position, (unsigned long long)b.position, a.active, b.active);
            a = b = start;
            old_glonass_group_walk(a, c.records, c.n, acq);
            new_walk(b, gnsscorr::kGlonassLoopPolicy, true, c.records, c.n, acq);
            EXPECT(same_walked(a, b), "record walk, GLONASS group, %s: %zu / %zu items, position %llu / %llu, active %d / %d", c.name, a.items.size(), b.items.size(),
                (unsigned long long)a.position, (unsigned long long)b.position, a.active, b.active);
        }
    // the cases do what their names say (the copies above could agree on nothing happening)
    Walked w;
    w.position = P;
    new_walk(w, gnsscorr::kVemlLoopPolicy, false, cases[2].records, 3, acq);
    EXPECT(w.items.size() == 1 && w.position == P + 6345 && w.d_state == 2, "veml pull-in records: %zu items, position %llu", w.items.size(), (unsigned long long)w.position);
    w = Walked();
    w.position = P;
    new_walk(w, gnsscorr::kGlonassLoopPolicy, true, cases[7].records, 4, acq);
    EXPECT(w.items.size() == 2 && w.position == P + 8000 && w.d_events == std::vector<int>{3} && !w.active && w.stops == 1, "loss in the middle: %zu items", w.items.size());
    EXPECT(w.items[1].Prompt_I == 102.0 && w.items[1].Tracking_sample_counter == P + 8000 && w.items[1].PRN == 11, "loss in the middle: the item of the period that lost lock");
    w = Walked();
    w.position = P;
    new_walk(w, gnsscorr::kVemlLoopPolicy, true, cases[6].records, 4, acq);
    EXPECT(w.items.size() == 2 && w.position == P + 8000 && w.d_events.empty() && w.active, "end of input in the middle: %zu items", w.items.size());
    EXPECT(w.items[0].Prompt_I == -8.0 && w.items[0].Prompt_Q == 101.0 && w.items[0].correlation_length_ms == 1 && w.items[0].fs == 4000000, "veml item: I/Q interchange");
}

// ---- ring feed plan and launch sizes -----------------------------------------------------------------------------------------------

static void test_feed_and_launch()
{
    const uint32_t vector_length = 4000;
    const int d_ring_periods = 8;
    struct Feed
    {
        const char* name;
        int ninput_items;
        uint64_t d_pushed, d_sample_counter;
    };
    const Feed feeds[] = {{"ninput < have", 3000, 10000 + 5000, 10000}, {"ninput == have", 5000, 10000 + 5000, 10000}, {"fresh > room", 40000, 10000 + 5000, 10000},
        {"room == 0", 40000, 10000 + 32000, 10000}, {"have == 0", 7000, 10000, 10000}, {"ninput == 0", 0, 10000 + 100, 10000}, {"fresh == room", 32000, 10000 + 4000, 10000},
        {"a piece shorter than a period", 1234, 10000, 10000}};
    for (const Feed& f : feeds)
        {
            // step 1 of work() as it was
            const uint64_t have = f.d_pushed - f.d_sample_counter;  // already pushed, not yet consumed
            uint64_t fresh = static_cast<uint64_t>(f.ninput_items) > have ? static_cast<uint64_t>(f.ninput_items) - have : 0;
            const uint64_t room = static_cast<uint64_t>(vector_length) * d_ring_periods - have;
            fresh = std::min(fresh, room);
            const uint64_t got = gnsscorr::ring_feed_fresh(f.ninput_items, have, static_cast<uint64_t>(vector_length) * d_ring_periods);
            EXPECT(got == fresh, "ring feed plan, %s: %llu, was %llu", f.name, (unsigned long long)got, (unsigned long long)fresh);
        }
    EXPECT(gnsscorr::ring_feed_fresh(40000, 5000, 32000) == 27000 && gnsscorr::ring_feed_fresh(40000, 32000, 32000) == 0 && gnsscorr::ring_feed_fresh(3000, 5000, 32000) == 0,
        "ring feed plan: values");

    struct Launch
    {
        const char* name;
        int max_out, produced;
        uint64_t d_pushed, d_sample_counter;
    };
    std::vector<gc_loop_record> d_records(d_ring_periods + 2);
    const Launch launches[] = {{"all periods fit", 80, 0, 10000 + 13000, 10000}, {"max_out smaller than the periods available", 2, 0, 10000 + 13000, 10000},
        {"the record buffer is the limit", 80, 0, 10000 + 48000, 10000}, {"max_out == 1 with a pending pull-in item", 1, 1, 10000 + 13000, 10000},
        {"max_out == 0", 0, 0, 10000 + 13000, 10000}, {"less than a period", 80, 0, 10000 + 1234, 10000}, {"nothing pushed", 80, 1, 10000, 10000}};
    for (const Launch& l : launches)
        {
            const int* produced = &l.produced;
            // step 2 of work() as it was (the GLONASS block's; the veml block's is the same line with *produced == 0)
            const int n_periods = std::min<int>(std::min<int>(l.max_out - *produced, static_cast<int>(d_records.size())),
                static_cast<int>((l.d_pushed - l.d_sample_counter) / vector_length) + 1);
            const int got = gnsscorr::block_launch_periods(l.max_out - l.produced, d_records.size(), l.d_pushed, l.d_sample_counter, vector_length);
            EXPECT(got == n_periods, "block launch size, %s: %d, was %d", l.name, got, n_periods);
        }
    EXPECT(gnsscorr::block_launch_periods(1 - 1, 10, 23000, 10000, 4000) == 0, "block launch size: max_out 1 and a pull-in item leave no period");
    EXPECT(gnsscorr::block_launch_periods(2, 10, 23000, 10000, 4000) == 2 && gnsscorr::block_launch_periods(80, 10, 23000, 10000, 4000) == 4, "block launch size: values");

    struct Group
    {
        const char* name;
        uint64_t head;
        std::vector<char> d_active;
        std::vector<uint64_t> d_position;
        std::vector<uint32_t> vlen;
        int expect;
    };
    const Group groups[] = {{"no active slot", 100000, {0, 0, 0}, {0, 0, 0}, {4000, 4000, 4000}, 0}, {"head <= position", 100000, {1, 1, 0}, {100000, 120000, 0}, {4000, 4000, 4000}, 0},
        {"one signal", 100000, {1, 0, 1}, {90000, 0, 60000}, {4000, 4000, 4000}, 11}, {"an inactive slot far behind", 100000, {1, 0}, {99000, 0}, {4000, 4000}, 1},
        {"two vector lengths", 100000, {1, 1}, {36000, 52000}, {16000, 4000}, 13}, {"two vector lengths, the long one behind", 100000, {1, 1}, {4000, 96000}, {16000, 4000}, 7}};
    for (const Group& g : groups)
        {
            // the launch-size loop of hip_tracking_group::run as it was
            const int d_n = static_cast<int>(g.d_active.size());
            const uint64_t head = g.head;
            int n_periods = 0;
            bool any = false;
            for (int ch = 0; ch < d_n; ch++)
                if (g.d_active[ch])
                    {
                        any = true;
                        // each slot's own code period: a mixed group sizes the launch for its shortest one
                        const uint32_t vlen = g.vlen[ch];
                        if (head > g.d_position[ch]) n_periods = std::max<int>(n_periods, static_cast<int>((head - g.d_position[ch]) / vlen) + 1);
                    }
            if (!any) n_periods = 0;
            const int got = gnsscorr::group_launch_periods(g.head, g.d_active, g.d_position, [&](int ch) { return g.vlen[ch]; });
            EXPECT(got == n_periods && got == g.expect, "group launch size, %s: %d, was %d, expected %d", g.name, got, n_periods, g.expect);
        }
}

// ---- the signal table --------------------------------------------------------------------------------------------------------------

// the three tables tracking_signals.h replaced, as they were
struct OldTrkSignalConstants
{
    double carrier_freq_hz, code_period_s, code_chip_rate_hz;
    uint32_t code_length_chips, code_samples_per_chip;
    bool veml, has_pilot, interchange_iq_with_pilot;
    int32_t correlation_length_ms;
};
static bool old_trk_signal_constants(char system, const std::string& signal, OldTrkSignalConstants* c)
{
    if (system == 'G' && signal == "1C") *c = {1575.42e6, 0.001, 1.023e6, 1023, 1, false, false, false, 1};
    else if (system == 'G' && signal == "2S") *c = {1.22760e9, 0.02, 0.5115e6, 10230, 1, false, false, false, 20};
    else if (system == 'G' && signal == "L5") *c = {1.17645e9, 0.001, 10.23e6, 10230, 1, false, true, true, 1};
    else if (system == 'E' && signal == "1B") *c = {1575.42e6, 0.004, 1.023e6, 4092, 2, true, true, false, 4};
    else if (system == 'E' && signal == "5X") *c = {1.17645e9, 0.001, 1.023e7, 10230, 1, false, true, true, 1};
    else if (system == 'C' && signal == "B1") *c = {1.561098e9, 0.001, 2.046e6, 2046, 1, false, false, false, 1};
    else if (system == 'C' && signal == "B3") *c = {1.268520e9, 0.001, 10.23e6, 10230, 1, false, false, false, 1};
    else return false;
    return true;
}

struct OldTrkSignalTraits
{
    const char* implementation;
    char system;
    const char* signal;
    double code_rate_hz, code_length_chips;
    float pll_bw_hz, dll_bw_hz, pll_bw_narrow_hz, dll_bw_narrow_hz;
    float early_late_space_chips, early_late_space_narrow_chips;
    bool veml;
    int cn0_min;
    double carrier_lock_th;
    bool has_pilot;
    int max_extension_data;
};
static const OldTrkSignalTraits& old_trk_traits(gnsscorr::TrkSignal s)
{
    static const OldTrkSignalTraits t[] = {
        {"GPS_L1_CA_DLL_PLL_Tracking_HIP", 'G', "1C", 1.023e6, 1023.0, 50.0f, 2.0f, 20.0f, 2.0f, 0.5f, 0.5f, false, 30, 0.80, false, 20},
        {"Galileo_E1_DLL_PLL_VEML_Tracking_HIP", 'E', "1B", 1.023e6, 4092.0, 5.0f, 0.5f, 2.0f, 0.25f, 0.15f, 0.15f, true, 25, 0.85, true, 0},
        {"BEIDOU_B1I_DLL_PLL_Tracking_HIP", 'C', "B1", 2.046e6, 2046.0, 50.0f, 2.0f, 20.0f, 2.0f, 0.5f, 0.5f, false, 25, 0.85, false, 20},
        {"GPS_L2_M_DLL_PLL_Tracking_HIP", 'G', "2S", 0.5115e6, 10230.0, 2.0f, 0.75f, 2.0f, 0.75f, 0.5f, 0.5f, false, 25, 0.85, false, 1},
        {"GPS_L5_DLL_PLL_Tracking_HIP", 'G', "L5", 10.23e6, 10230.0, 50.0f, 2.0f, 2.0f, 0.25f, 0.5f, 0.15f, false, 25, 0.75, true, 10},
        {"Galileo_E5a_DLL_PLL_Tracking_HIP", 'E', "5X", 10.23e6, 10230.0, 20.0f, 20.0f, 5.0f, 2.0f, 0.5f, 0.15f, false, 25, 0.85, true, 20},
        {"BEIDOU_B3I_DLL_PLL_Tracking_HIP", 'C', "B3", 10.23e6, 10230.0, 50.0f, 2.0f, 20.0f, 2.0f, 0.5f, 0.5f, false, 25, 0.85, false, 20}};
    return t[static_cast<int>(s)];
}

// what the constructor of hip_dll_pll_veml_tracking set per signal, as it was (without the symbol-synchronisation set-up, which stays there)
struct OldBlockConstants
{
    double d_signal_carrier_freq = 0.0, d_code_period = 0.0, d_code_chip_rate = 0.0;
    uint32_t d_code_length_chips = 0, d_code_samples_per_chip = 0;
    int32_t d_correlation_length_ms = 1;
    bool d_veml = false, interchange_iq = false, track_pilot = false;
};
static OldBlockConstants old_block_constants(char system, const std::string& signal_type, bool track_pilot_in)
{
    OldBlockConstants b;
    struct
    {
        char system;
        bool track_pilot;
    } trk_parameters = {system, track_pilot_in};
    double& d_signal_carrier_freq = b.d_signal_carrier_freq;
    double& d_code_period = b.d_code_period;
    double& d_code_chip_rate = b.d_code_chip_rate;
    uint32_t& d_code_length_chips = b.d_code_length_chips;
    uint32_t& d_code_samples_per_chip = b.d_code_samples_per_chip;
    int32_t& d_correlation_length_ms = b.d_correlation_length_ms;
    bool& d_veml = b.d_veml;
    bool& interchange_iq = b.interchange_iq;
    if (trk_parameters.system == 'G' && signal_type == "1C")
        {
            d_signal_carrier_freq = 1575.42e6;  // GPS_L1_FREQ_HZ
            d_code_period = 0.001;
            d_code_chip_rate = 1.023e6;
            d_correlation_length_ms = 1;
            d_code_samples_per_chip = 1;
            d_code_length_chips = 1023;
            trk_parameters.track_pilot = false;  // no pilot component, no secondary code
        }
    else if (trk_parameters.system == 'E' && signal_type == "1B")
        {
            d_signal_carrier_freq = 1575.42e6;  // Galileo_E1_FREQ_HZ
            d_code_period = 0.004;
            d_code_chip_rate = 1.023e6;
            d_code_length_chips = 4092;
            d_correlation_length_ms = 4;
            d_code_samples_per_chip = 2;  // sinBOC(1,1) replica, 2 samples per chip
            d_veml = true;
        }
    else if (trk_parameters.system == 'C' && signal_type == "B1")
        {
            d_signal_carrier_freq = 1.561098e9;  // BEIDOU_B1I_FREQ_HZ
            d_code_period = 0.001;
            d_code_chip_rate = 2.046e6;
            d_code_length_chips = 2046;
            d_correlation_length_ms = 1;
            d_code_samples_per_chip = 1;
            trk_parameters.track_pilot = false;
        }
    else if (trk_parameters.system == 'G' && signal_type == "2S")
        {
            d_signal_carrier_freq = 1.22760e9;  // GPS_L2_FREQ_HZ
            d_code_period = 0.02;               // GPS_L2_M_PERIOD
            d_code_chip_rate = 0.5115e6;
            d_code_length_chips = 10230;
            d_correlation_length_ms = 20;
            d_code_samples_per_chip = 1;
            trk_parameters.track_pilot = false;  // no pilot component, no secondary code
        }
    else if (trk_parameters.system == 'G' && signal_type == "L5")
        {
            d_signal_carrier_freq = 1.17645e9;  // GPS_L5_FREQ_HZ
            d_code_period = 0.001;
            d_code_chip_rate = 10.23e6;
            d_correlation_length_ms = 1;
            d_code_samples_per_chip = 1;
            d_code_length_chips = 10230;
            interchange_iq = trk_parameters.track_pilot;
        }
    else if (trk_parameters.system == 'E' && signal_type == "5X")
        {
            d_signal_carrier_freq = 1.17645e9;  // GALILEO_E5A_FREQ_HZ
            d_code_period = 0.001;
            d_code_chip_rate = 1.023e7;
            d_correlation_length_ms = 1;
            d_code_samples_per_chip = 1;
            d_code_length_chips = 10230;
            interchange_iq = trk_parameters.track_pilot;
        }
    else if (trk_parameters.system == 'C' && signal_type == "B3")
        {
            d_signal_carrier_freq = 1.268520e9;  // BEIDOU_B3I_FREQ_HZ
            d_code_period = 0.001;
            d_code_chip_rate = 10.23e6;
            d_code_length_chips = 10230;
            d_correlation_length_ms = 1;
            d_code_samples_per_chip = 1;
            trk_parameters.track_pilot = false;
        }
    b.track_pilot = trk_parameters.track_pilot;
    return b;
}

static const gnsscorr::TrkSignal kAllSignals[] = {gnsscorr::TrkSignal::GPS_L1_CA, gnsscorr::TrkSignal::GALILEO_E1, gnsscorr::TrkSignal::BEIDOU_B1I, gnsscorr::TrkSignal::GPS_L2_M,
    gnsscorr::TrkSignal::GPS_L5, gnsscorr::TrkSignal::GALILEO_E5A, gnsscorr::TrkSignal::BEIDOU_B3I};

static void test_signal_table()
{
    for (gnsscorr::TrkSignal s : kAllSignals)
        {
            const gnsscorr::TrkSignalInfo& n = gnsscorr::trk_signal(s);
            const OldTrkSignalTraits& t = old_trk_traits(s);
            EXPECT(n.system == t.system && std::string(n.signal) == t.signal, "signal table: row %d is %c %s", static_cast<int>(s), n.system, n.signal);
            EXPECT(gnsscorr::trk_signal_find(t.system, t.signal) == &n, "signal table: look-up of %c %s", t.system, t.signal);
            EXPECT(std::string(n.implementation) == t.implementation && n.code_chip_rate_hz == t.code_rate_hz && static_cast<double>(n.code_length_chips) == t.code_length_chips &&
                       n.pll_bw_hz == t.pll_bw_hz && n.dll_bw_hz == t.dll_bw_hz && n.pll_bw_narrow_hz == t.pll_bw_narrow_hz && n.dll_bw_narrow_hz == t.dll_bw_narrow_hz &&
                       n.early_late_space_chips == t.early_late_space_chips && n.early_late_space_narrow_chips == t.early_late_space_narrow_chips && n.veml == t.veml &&
                       n.cn0_min == t.cn0_min && n.carrier_lock_th == t.carrier_lock_th && n.has_pilot == t.has_pilot && n.max_extension_data == t.max_extension_data,
                "signal table: %c %s differs from the adapters' traits", t.system, t.signal);
            OldTrkSignalConstants c;
            const bool known = old_trk_signal_constants(t.system, t.signal, &c);
            EXPECT(known && n.carrier_freq_hz == c.carrier_freq_hz && n.code_period_s == c.code_period_s && n.code_chip_rate_hz == c.code_chip_rate_hz &&
                       n.code_length_chips == c.code_length_chips && n.code_samples_per_chip == c.code_samples_per_chip && n.veml == c.veml && n.has_pilot == c.has_pilot &&
                       n.interchange_iq_with_pilot == c.interchange_iq_with_pilot && n.correlation_length_ms == c.correlation_length_ms,
                "signal table: %c %s differs from the device block's constants", t.system, t.signal);
            for (bool pilot : {false, true})
                {
                    const OldBlockConstants b = old_block_constants(t.system, t.signal, pilot);
                    const bool track_pilot = pilot && n.has_pilot;  // what the constructor does with the row
                    EXPECT(n.carrier_freq_hz == b.d_signal_carrier_freq && n.code_period_s == b.d_code_period && n.code_chip_rate_hz == b.d_code_chip_rate &&
                               n.code_length_chips == b.d_code_length_chips && n.code_samples_per_chip == b.d_code_samples_per_chip && n.correlation_length_ms == b.d_correlation_length_ms &&
                               n.veml == b.d_veml && track_pilot == b.track_pilot && (track_pilot && n.interchange_iq_with_pilot) == b.interchange_iq,
                        "signal table: %c %s (pilot %d) differs from the host block's constructor", t.system, t.signal, pilot);
                }
        }
    EXPECT(gnsscorr::trk_signal_find('R', "1G") == nullptr && gnsscorr::trk_signal_find('G', "1B") == nullptr && gnsscorr::trk_signal_find('E', "1C") == nullptr, "signal table: unknown signals");
    OldTrkSignalConstants c;
    EXPECT(!old_trk_signal_constants('R', "1G", &c), "signal table: the old look-up");
    // GPS L1 and GLONASS constants of the carrier-aided and GLONASS blocks, as they were written there
    const CAidSignal g = CAidSignal::gps_l1(), r1 = CAidSignal::glonass(1), r2 = CAidSignal::glonass(2);
    EXPECT(!g.is_glonass && g.system == 'G' && g.code_rate_hz == 1.023e6 && g.code_length_chips == 1023.0 && g.carrier_freq_hz == 1575.42e6 && g.channel_spacing_hz == 0.0, "C-aid: GPS L1");
    EXPECT(r1.is_glonass && r1.system == 'R' && r1.code_rate_hz == 0.511e6 && r1.code_length_chips == 511.0 && r1.carrier_freq_hz == 1.602e9 && r1.channel_spacing_hz == 0.5625e6, "C-aid: GLONASS L1");
    EXPECT(r2.is_glonass && r2.system == 'R' && r2.code_rate_hz == 0.511e6 && r2.code_length_chips == 511.0 && r2.carrier_freq_hz == 1.246e9 && r2.channel_spacing_hz == 0.4375e6, "C-aid: GLONASS L2");
    EXPECT(gnsscorr::glonass_band(1).freq_hz == 1.602e9 && gnsscorr::glonass_band(1).dfreq_hz == 0.5625e6 && gnsscorr::glonass_band(2).freq_hz == 1.246e9 && gnsscorr::glonass_band(2).dfreq_hz == 0.4375e6,
        "GLONASS bands");
}

// the generator calls of loop_start_channel as they were (the host block made the same calls without looking at the status)
static gc_status old_replicas(char system, const std::string& signal, uint32_t prn, bool pilot, std::vector<float>& code, std::vector<float>& data_code)
{
    const int code_len = static_cast<int>(code.size());
    gc_status st = GC_OK;
    if (system == 'G' && signal == "1C") st = gc_gps_l1_ca_code_gen_float(code.data(), static_cast<int32_t>(prn), 0);
    else if (system == 'G' && signal == "2S") st = gc_gps_l2c_m_code_gen_float(code.data(), prn);
    else if (system == 'G' && signal == "L5")
        {
            st = pilot ? gc_gps_l5q_code_gen_float(code.data(), prn) : gc_gps_l5i_code_gen_float(code.data(), prn);
            if (pilot && st == GC_OK) st = gc_gps_l5i_code_gen_float(data_code.data(), prn);
        }
    else if (system == 'E' && signal == "1B")
        {
            st = gc_galileo_e1_code_gen_sinboc11_float(code.data(), pilot ? "1C" : "1B", prn);
            if (pilot && st == GC_OK) st = gc_galileo_e1_code_gen_sinboc11_float(data_code.data(), "1B", prn);
        }
    else if (system == 'E' && signal == "5X")
        {
            std::vector<float> aux(2 * code_len);
            st = gc_galileo_e5_a_code_gen_complex_primary(aux.data(), static_cast<int32_t>(prn), "5X");
            for (int i = 0; i < code_len; i++)
                {
                    code[i] = pilot ? aux[2 * i + 1] : aux[2 * i];
                    data_code[i] = aux[2 * i];
                }
        }
    else if (system == 'C' && signal == "B1") st = gc_beidou_b1i_code_gen_float(code.data(), static_cast<int32_t>(prn), 0);
    else st = gc_beidou_b3i_code_gen_float(code.data(), static_cast<int32_t>(prn), 0);
    return st;
}

static void test_replicas()
{
    const uint32_t prns[] = {7, 19, 8, 12, 3, 24, 30};  // one per row of the table
    const float untouched = 12345.0f;
    for (gnsscorr::TrkSignal s : kAllSignals)
        {
            const gnsscorr::TrkSignalInfo& n = gnsscorr::trk_signal(s);
            const uint32_t prn = prns[static_cast<int>(s)];
            const size_t len = static_cast<size_t>(n.code_length_chips) * n.code_samples_per_chip;
            for (bool pilot : {false, true})
                {
                    if (pilot && !n.has_pilot) continue;
                    std::vector<float> code(len, untouched), data(len, untouched), old_code(len, untouched), old_data(len, untouched);
                    const gc_status st = gnsscorr::trk_generate_replicas(n.system, n.signal, prn, pilot, code.data(), data.data());
                    const gc_status old_st = old_replicas(n.system, n.signal, prn, pilot, old_code, old_data);
                    EXPECT(st == GC_OK && old_st == GC_OK, "replicas %c %s PRN %u pilot %d: status %d, was %d (%s)", n.system, n.signal, prn, pilot, st, old_st, gc_last_error());
                    EXPECT(std::memcmp(code.data(), old_code.data(), len * sizeof(float)) == 0, "replicas %c %s pilot %d: the code differs", n.system, n.signal, pilot);
                    size_t chips = 0;
                    for (float v : code) chips += (v == 1.0f || v == -1.0f) ? 1 : 0;
                    EXPECT(chips == len, "replicas %c %s pilot %d: %zu of %zu samples are chips", n.system, n.signal, pilot, chips, len);
                    if (pilot)
                        {
                            EXPECT(std::memcmp(data.data(), old_data.data(), len * sizeof(float)) == 0, "replicas %c %s: the data component's code differs", n.system, n.signal);
                            EXPECT(std::memcmp(data.data(), code.data(), len * sizeof(float)) != 0, "replicas %c %s: pilot and data replica are the same", n.system, n.signal);
                            // a NULL data_code with pilot: the code alone
                            std::vector<float> alone(len, untouched);
                            EXPECT(gnsscorr::trk_generate_replicas(n.system, n.signal, prn, true, alone.data(), nullptr) == GC_OK && alone == code, "replicas %c %s: pilot without data_code", n.system, n.signal);
                        }
                    else
                        {
                            size_t touched = 0;
                            for (float v : data) touched += v != untouched ? 1 : 0;
                            EXPECT(touched == 0, "replicas %c %s: data_code written without pilot (%zu values)", n.system, n.signal, touched);
                        }
                }
            // a PRN the signal does not have: the generator's status
            std::vector<float> code(len), data(len), old_code(len), old_data(len);
            const gc_status st = gnsscorr::trk_generate_replicas(n.system, n.signal, 99, n.has_pilot, code.data(), data.data());
            const gc_status old_st = old_replicas(n.system, n.signal, 99, n.has_pilot, old_code, old_data);
            EXPECT(st != GC_OK && st == old_st, "replicas %c %s PRN 99: status %d, was %d", n.system, n.signal, st, old_st);
        }
    std::vector<float> code(10230, untouched);
    EXPECT(gnsscorr::trk_generate_replicas('R', "1G", 1, false, code.data(), nullptr) == GC_ERR_INVALID && code[0] == untouched, "replicas: a signal that is not in the table");
}

// ---- adapters ----------------------------------------------------------------------------------------------------------------------

// the constructor of DllPllTrackingHip as it was, up to the Dll_Pll_Conf it hands to the block
static Dll_Pll_Conf old_adapter_conf(gnsscorr::TrkSignal SIG, ConfigurationInterface* configuration, const std::string& role)
{
    const OldTrkSignalTraits& t = old_trk_traits(SIG);
    Dll_Pll_Conf trk_param = Dll_Pll_Conf();
    int fs_in_deprecated = configuration->property("GNSS-SDR.internal_fs_hz", 2048000);
    int fs_in = configuration->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
    trk_param.fs_in = fs_in;
    trk_param.high_dyn = configuration->property(role + ".high_dyn", false);
    trk_param.dump = configuration->property(role + ".dump", false);
    trk_param.dump_filename = configuration->property(role + ".dump_filename", std::string("./track_ch"));
    trk_param.dump_mat = configuration->property(role + ".dump_mat", true);
    trk_param.smoother_length = std::max(1, configuration->property(role + ".smoother_length", 10));
    trk_param.pll_bw_hz = configuration->property(role + ".pll_bw_hz", t.pll_bw_hz);
    trk_param.pll_bw_narrow_hz = configuration->property(role + ".pll_bw_narrow_hz", t.pll_bw_narrow_hz);
    trk_param.dll_bw_narrow_hz = configuration->property(role + ".dll_bw_narrow_hz", t.dll_bw_narrow_hz);
    trk_param.dll_bw_hz = configuration->property(role + ".dll_bw_hz", t.dll_bw_hz);
    trk_param.dll_filter_order = std::min(3, std::max(1, configuration->property(role + ".dll_filter_order", 2)));
    trk_param.pll_filter_order = std::min(3, std::max(2, configuration->property(role + ".pll_filter_order", 3)));
    trk_param.fll_filter_order = (trk_param.pll_filter_order == 2) ? 1 : 2;
    trk_param.enable_fll_pull_in = configuration->property(role + ".enable_fll_pull_in", false);
    trk_param.fll_bw_hz = configuration->property(role + ".fll_bw_hz", 35.0f);
    trk_param.pull_in_time_s = static_cast<unsigned int>(configuration->property(role + ".pull_in_time_s", 2.0f));
    trk_param.early_late_space_chips = configuration->property(role + ".early_late_space_chips", t.early_late_space_chips);
    trk_param.early_late_space_narrow_chips = configuration->property(role + ".early_late_space_narrow_chips", t.early_late_space_narrow_chips);
    int extend_correlation_symbols = configuration->property(role + ".extend_correlation_symbols", 1);
    bool track_pilot = configuration->property(role + ".track_pilot", false);
    if (!t.has_pilot) track_pilot = false;
    if (extend_correlation_symbols < 1) extend_correlation_symbols = 1;
    if (!track_pilot)
        {
            const int longest = std::max(1, t.max_extension_data);
            if (extend_correlation_symbols > longest) extend_correlation_symbols = longest;
        }
    trk_param.extend_correlation_symbols = extend_correlation_symbols;
    if (t.veml)
        {
            trk_param.very_early_late_space_chips = configuration->property(role + ".very_early_late_space_chips", 0.6f);
            trk_param.very_early_late_space_narrow_chips = configuration->property(role + ".very_early_late_space_narrow_chips", 0.6f);
        }
    else
        {
            trk_param.very_early_late_space_chips = 0.0;
            trk_param.very_early_late_space_narrow_chips = 0.0;
        }
    trk_param.vector_length = std::round(static_cast<double>(fs_in) / (t.code_rate_hz / t.code_length_chips));
    trk_param.system = t.system;
    std::memcpy(trk_param.signal, t.signal, 3);
    trk_param.track_pilot = track_pilot;
    trk_param.cn0_samples = configuration->property(role + ".cn0_samples", 20);
    trk_param.cn0_min = configuration->property(role + ".cn0_min", t.cn0_min);
    trk_param.max_lock_fail = configuration->property(role + ".max_lock_fail", 50);
    trk_param.carrier_lock_th = configuration->property(role + ".carrier_lock_th", t.carrier_lock_th);
    return trk_param;
}

static bool same_conf(const Dll_Pll_Conf& a, const Dll_Pll_Conf& b)
{
    return a.fll_filter_order == b.fll_filter_order && a.enable_fll_pull_in == b.enable_fll_pull_in && a.enable_fll_steady_state == b.enable_fll_steady_state &&
           a.pull_in_time_s == b.pull_in_time_s && a.pll_filter_order == b.pll_filter_order && a.dll_filter_order == b.dll_filter_order && a.fs_in == b.fs_in &&
           a.vector_length == b.vector_length && a.dump == b.dump && a.dump_mat == b.dump_mat && a.dump_filename == b.dump_filename && a.pll_pull_in_bw_hz == b.pll_pull_in_bw_hz &&
           a.dll_pull_in_bw_hz == b.dll_pull_in_bw_hz && a.fll_bw_hz == b.fll_bw_hz && a.pll_bw_hz == b.pll_bw_hz && a.dll_bw_hz == b.dll_bw_hz && a.pll_bw_narrow_hz == b.pll_bw_narrow_hz &&
           a.dll_bw_narrow_hz == b.dll_bw_narrow_hz && a.early_late_space_chips == b.early_late_space_chips && a.very_early_late_space_chips == b.very_early_late_space_chips &&
           a.early_late_space_narrow_chips == b.early_late_space_narrow_chips && a.very_early_late_space_narrow_chips == b.very_early_late_space_narrow_chips &&
           a.extend_correlation_symbols == b.extend_correlation_symbols && a.high_dyn == b.high_dyn && a.cn0_samples == b.cn0_samples &&
           a.carrier_lock_det_mav_samples == b.carrier_lock_det_mav_samples && a.cn0_min == b.cn0_min && a.max_lock_fail == b.max_lock_fail && a.smoother_length == b.smoother_length &&
           a.carrier_lock_th == b.carrier_lock_th && a.track_pilot == b.track_pilot && a.system == b.system && std::memcmp(a.signal, b.signal, 3) == 0;
}

template <gnsscorr::TrkSignal SIG, class Block>
static void check_veml_adapter(ConfigurationInterface* config, const char* config_name, const char* suffix)
{
    const std::string role = "Tracking";
    DllPllTrackingHip<SIG, Block> trk(config, role, 1, 1);
    const OldTrkSignalTraits& t = old_trk_traits(SIG);
    EXPECT(trk.implementation() == std::string(t.implementation) + suffix, "adapter %s%s: implementation %s", t.implementation, suffix, trk.implementation().c_str());
    EXPECT(trk.item_size() == sizeof(gr_complex) && trk.role() == role && trk.block() != nullptr, "adapter %s%s: item size, role, block", t.implementation, suffix);
    EXPECT(same_conf(trk.conf(), old_adapter_conf(SIG, config, role)), "adapter %s%s, %s configuration: the Dll_Pll_Conf differs", t.implementation, suffix, config_name);
    Gnss_Synchro syn;
    trk.set_channel(3);
    trk.set_gnss_synchro(&syn);
    trk.stop_tracking();
    EXPECT(trk.block()->state() == 0, "adapter %s%s: state after stop_tracking", t.implementation, suffix);
}

template <gnsscorr::TrkSignal SIG>
static void check_veml_adapters(ConfigurationInterface* config, const char* config_name)
{
    check_veml_adapter<SIG, hip_dll_pll_veml_tracking>(config, config_name, "");
    check_veml_adapter<SIG, hip_dll_pll_veml_tracking_dev>(config, config_name, "_DEV");
}

template <class Adapter>
static void check_glonass_adapter(ConfigurationInterface* config, const char* name)
{
    Adapter trk(config, "Tracking", 1, 1);
    EXPECT(trk.implementation() == name && trk.item_size() == sizeof(gr_complex) && trk.role() == "Tracking" && trk.block() != nullptr, "adapter %s: implementation %s", name,
        trk.implementation().c_str());
    EXPECT(trk.vector_length() == 6625 && trk.block()->required_input_items() == 2 * 6625, "adapter %s: vector length %u", name, trk.vector_length());
    trk.stop_tracking();
    EXPECT(!trk.block()->tracking_enabled(), "adapter %s: enabled after stop_tracking", name);
}

template <int BAND>
static void check_c_aid_adapter(const char* name, unsigned int vector_length)
{
    for (const char* item_type : {"gr_complex", "cshort"})
        {
            InMemoryConfiguration config;
            config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
            config.set_property("Tracking.item_type", item_type);
            DllPllCAidTrackingHip<BAND> trk(&config, "Tracking", 1, 1);
            const bool cshort = std::string(item_type) == "cshort";
            EXPECT(trk.implementation() == name && trk.role() == "Tracking" && trk.item_type() == item_type, "adapter %s (%s): implementation %s", name, item_type, trk.implementation().c_str());
            EXPECT(trk.item_size() == (cshort ? sizeof(std::complex<int16_t>) : sizeof(gr_complex)), "adapter %s (%s): item size %zu", name, item_type, trk.item_size());
            EXPECT((trk.block_cshort() != nullptr) == cshort && (trk.block_gr_complex() != nullptr) == !cshort && trk.vector_length() == vector_length, "adapter %s (%s): block, vector length %u", name,
                item_type, trk.vector_length());
            trk.set_channel(2);
            trk.stop_tracking();
        }
}

static void test_adapters()
{
    InMemoryConfiguration defaults;
    // the clamps: an extension above the data limit, a pilot the signal may not have, filter orders out of range, the deprecated rate key
    InMemoryConfiguration clamps;
    clamps.set_property("GNSS-SDR.internal_fs_hz", "5000000");
    clamps.set_property("Tracking.extend_correlation_symbols", "50");
    clamps.set_property("Tracking.track_pilot", "true");
    clamps.set_property("Tracking.dll_filter_order", "0");
    clamps.set_property("Tracking.pll_filter_order", "9");
    clamps.set_property("Tracking.smoother_length", "0");
    clamps.set_property("Tracking.cn0_min", "31");
    clamps.set_property("Tracking.very_early_late_space_chips", "0.7");
    // the data limit without the pilot, and the orders clamped from the other side
    InMemoryConfiguration data_limit;
    data_limit.set_property("GNSS-SDR.internal_fs_hz", "5000000");
    data_limit.set_property("GNSS-SDR.internal_fs_sps", "12500000");
    data_limit.set_property("Tracking.extend_correlation_symbols", "50");
    data_limit.set_property("Tracking.dll_filter_order", "7");
    data_limit.set_property("Tracking.pll_filter_order", "1");
    struct
    {
        InMemoryConfiguration* config;
        const char* name;
    } configs[] = {{&defaults, "default"}, {&clamps, "clamping"}, {&data_limit, "data-limit"}};
    for (const auto& c : configs)
        {
            check_veml_adapters<gnsscorr::TrkSignal::GPS_L1_CA>(c.config, c.name);
            check_veml_adapters<gnsscorr::TrkSignal::GALILEO_E1>(c.config, c.name);
            check_veml_adapters<gnsscorr::TrkSignal::BEIDOU_B1I>(c.config, c.name);
            check_veml_adapters<gnsscorr::TrkSignal::GPS_L2_M>(c.config, c.name);
            check_veml_adapters<gnsscorr::TrkSignal::GPS_L5>(c.config, c.name);
            check_veml_adapters<gnsscorr::TrkSignal::GALILEO_E5A>(c.config, c.name);
            check_veml_adapters<gnsscorr::TrkSignal::BEIDOU_B3I>(c.config, c.name);
        }
    // what the clamps give, in numbers (old_adapter_conf could be as wrong as the adapter)
    {
        GpsL1CaDllPllTrackingHipDev l1(&clamps, "Tracking", 1, 1);
        EXPECT(l1.conf().extend_correlation_symbols == 20 && !l1.conf().track_pilot && l1.conf().dll_filter_order == 1 && l1.conf().pll_filter_order == 3 && l1.conf().fll_filter_order == 2 &&
                   l1.conf().fs_in == 5e6 && l1.conf().vector_length == 5000 && l1.conf().smoother_length == 1 && l1.conf().cn0_min == 31 && l1.conf().very_early_late_space_chips == 0.0f,
            "GPS L1 adapter under the clamping configuration");
        GalileoE1DllPllVemlTrackingHip e1(&clamps, "Tracking", 1, 1);
        EXPECT(e1.conf().extend_correlation_symbols == 50 && e1.conf().track_pilot && e1.conf().vector_length == 20000 && e1.conf().very_early_late_space_chips == 0.7f &&
                   e1.conf().very_early_late_space_narrow_chips == 0.6f,
            "Galileo E1 adapter under the clamping configuration");
        GalileoE1DllPllVemlTrackingHip e1d(&data_limit, "Tracking", 1, 1);
        EXPECT(e1d.conf().extend_correlation_symbols == 1 && e1d.conf().dll_filter_order == 3 && e1d.conf().pll_filter_order == 2 && e1d.conf().fll_filter_order == 1 && e1d.conf().fs_in == 12.5e6,
            "Galileo E1 adapter under the data-limit configuration");
        GpsL5DllPllTrackingHip l5(&data_limit, "Tracking", 1, 1);
        EXPECT(l5.conf().extend_correlation_symbols == 10 && l5.conf().carrier_lock_th == 0.75 && l5.conf().vector_length == 12500, "GPS L5 adapter under the data-limit configuration");
        GpsL1CaDllPllTrackingHip d(&defaults, "Tracking", 1, 1);
        EXPECT(d.conf().fs_in == 2048000.0 && d.conf().vector_length == 2048 && d.conf().pll_bw_hz == 50.0f && d.conf().cn0_min == 30 && d.conf().carrier_lock_th == 0.80, "GPS L1 adapter defaults");
    }
    InMemoryConfiguration glonass;
    glonass.set_property("GNSS-SDR.internal_fs_sps", "6625000");
    check_glonass_adapter<GlonassL1CaDllPllTrackingHip>(&glonass, "GLONASS_L1_CA_DLL_PLL_Tracking_HIP");
    check_glonass_adapter<GlonassL2CaDllPllTrackingHip>(&glonass, "GLONASS_L2_CA_DLL_PLL_Tracking_HIP");
    check_glonass_adapter<GlonassL1CaDllPllTrackingDevHip>(&glonass, "GLONASS_L1_CA_DLL_PLL_Tracking_Dev_HIP");
    check_glonass_adapter<GlonassL2CaDllPllTrackingDevHip>(&glonass, "GLONASS_L2_CA_DLL_PLL_Tracking_Dev_HIP");
    check_c_aid_adapter<0>("GPS_L1_CA_DLL_PLL_C_Aid_Tracking_HIP", 4000);
    check_c_aid_adapter<1>("GLONASS_L1_CA_DLL_PLL_C_Aid_Tracking_HIP", 4000);
    check_c_aid_adapter<2>("GLONASS_L2_CA_DLL_PLL_C_Aid_Tracking_HIP", 4000);
}

// ---- the real blocks and groups without a device -----------------------------------------------------------------------------------

template <class Block>
static void check_block_without_device(Block& blk, const char* name, gc_status expect_status)
{
    const gc_status st = blk.last_status();
    EXPECT(st != GC_OK && (expect_status == GC_OK || st == expect_status), "%s without a device: construction status %d", name, st);
    Gnss_Synchro syn;
    syn.System = 'G';
    syn.PRN = 1;
    blk.set_channel(1);
    blk.set_gnss_synchro(&syn);
    blk.start_tracking();
    EXPECT(blk.last_status() == st && blk.state() == 0 && !blk.tracking_enabled() && blk.events().empty(), "%s without a device: start_tracking changed status %d or state %d", name,
        blk.last_status(), blk.state());
    std::vector<gr_complex> in(9000, gr_complex(1.0f, -1.0f));
    Gnss_Synchro out[4];
    uint64_t counter = 0;
    for (int n : {9000, 0, 1234})
        {
            int produced = -1;
            const int consumed = blk.work(in.data(), n, out, 4, &produced);
            counter += static_cast<uint64_t>(n);
            EXPECT(consumed == n && produced == 0 && blk.sample_counter() == counter, "%s in standby: %d of %d items consumed, %d produced, counter %llu", name, consumed, n, produced,
                (unsigned long long)blk.sample_counter());
        }
    blk.stop_tracking();
    EXPECT(blk.last_status() == st && blk.state() == 0 && blk.events().empty(), "%s without a device: stop_tracking", name);
}

template <class Group>
static void check_group_without_context(Group& group, const char* name, int n_channels)
{
    const gc_status st = group.last_status();
    EXPECT(st != GC_OK, "%s with a null context: construction status %d", name, st);
    EXPECT(group.n_channels() == n_channels, "%s with a null context: %d channels", name, group.n_channels());
    Gnss_Synchro acq;
    acq.System = 'G';
    acq.PRN = 1;
    EXPECT(group.start_tracking(0, acq, 0) == st && group.start_tracking(-1, acq, 0) == st, "%s with a null context: start_tracking does not return the construction status", name);
    std::vector<std::vector<Gnss_Synchro>> out;
    EXPECT(group.run(out) == -1 && out.empty() && group.last_status() == st, "%s with a null context: run()", name);
}

static void test_blocks_without_device()
{
    Dll_Pll_Conf conf;
    conf.fs_in = 4e6;
    conf.vector_length = 4000;
    {
        hip_dll_pll_veml_tracking_dev blk(conf, 0, 8);
        check_block_without_device(blk, "veml device-loop block", GC_OK);
        EXPECT(blk.required_input_items() == 8000, "veml device-loop block: forecast");
    }
    {
        Dll_Pll_Conf unknown = conf;
        unknown.system = 'R';
        std::memcpy(unknown.signal, "1G", 3);
        hip_dll_pll_veml_tracking_dev blk(unknown, 0, 8);
        check_block_without_device(blk, "veml device-loop block with a signal it does not have", GC_ERR_INVALID);
    }
    gnsscorr::GlonassTrkConf g;
    g.band = 2;
    g.fs_in = 6625000;
    g.vector_length = 6625;
    {
        hip_glonass_ca_dll_pll_tracking_dev blk(g, 0, 8);
        check_block_without_device(blk, "GLONASS device-loop block", GC_OK);
        EXPECT(blk.required_input_items() == 13250, "GLONASS device-loop block: forecast");
        hip_glonass_ca_dll_pll_tracking_dev positional(2, 6625000, 6625, 50.0f, 2.0f, 0.5f);
        check_block_without_device(positional, "GLONASS device-loop block, positional constructor", blk.last_status());
        EXPECT(positional.required_input_items() == 13250, "GLONASS device-loop block, positional constructor: forecast");
    }
    {
        hip_tracking_group group(nullptr, nullptr, conf, 3);
        check_group_without_context(group, "veml group", 3);
        Dll_Pll_Conf e1 = conf;
        e1.system = 'E';
        std::memcpy(e1.signal, "1B", 3);
        e1.vector_length = 16000;
        hip_tracking_group mixed(nullptr, nullptr, std::vector<std::pair<Dll_Pll_Conf, int>>{{conf, 2}, {e1, 1}});
        check_group_without_context(mixed, "mixed veml group", 3);
        EXPECT(mixed.signal_of(0) == 0 && mixed.signal_of(1) == 0 && mixed.signal_of(2) == 1, "mixed veml group: signal_of");
        Dll_Pll_Conf unknown = conf;
        unknown.system = 'R';
        hip_tracking_group refused(nullptr, nullptr, unknown, 2);
        EXPECT(refused.last_status() == GC_ERR_INVALID && refused.n_channels() == 0, "veml group with a signal it does not have: status %d", refused.last_status());
        hip_tracking_group empty(nullptr, nullptr, conf, 0);
        EXPECT(empty.last_status() == GC_ERR_INVALID, "veml group without slots: status %d", empty.last_status());
    }
    {
        hip_glonass_tracking_group group(nullptr, nullptr, g, 3);
        check_group_without_context(group, "GLONASS group", 3);
        hip_glonass_tracking_group empty(nullptr, nullptr, g, 0);
        EXPECT(empty.last_status() == GC_ERR_INVALID, "GLONASS group without slots: status %d", empty.last_status());
    }
}

int main()
{
    test_record_walk();
    test_feed_and_launch();
    test_signal_table();
    test_replicas();
    test_adapters();
    test_blocks_without_device();
    if (g_fail)
        {
            std::printf("%d check(s) FAILED\n", g_fail);
            return 1;
        }
    std::printf("trk block self-test passed\n");
    return 0;
}
