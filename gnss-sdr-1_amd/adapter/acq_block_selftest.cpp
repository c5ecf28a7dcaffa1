// acq_block_selftest -- what the acquisition block images share (acquisition_block_base.h, acquisition_adapter_base.h), without a GPU:
//   - hip_acquisition_item_block driven through scripted blocks whose search step returns canned outcomes instead of calling an
//     engine, once per state numbering and policy of the four item blocks (Tong, QuickSync, paired, E5a CAF): reset and find, reset and
//     fail at max_dwells, engine error, set_state(1) from outside, two searches in a row, 0 / 1 / 3 items in the idle and terminal
//     states.  After every call: items consumed, sample counter, state, events, the synchro fields a restart clears, and d_active as a
//     further idle call shows it;
//   - inclusive_doppler_bins against the values of the loops it replaced;
//   - exponential_quantile_threshold, bit for bit, against the calculate_threshold it replaced (copied below), and the step-0 case;
//   - the real blocks without a device: init() gives GC_ERR_NO_DEVICE and one item in state 1 takes each block's own error path.
// Creates no GPU context: run it with no device visible (tests/test_acq_block_base.py hides them).
#include "hip_e5a_noncoherent_iq_acquisition_caf.h"
#include "hip_pcps_quicksync_acquisition.h"
#include "hip_pcps_tong_acquisition.h"
#include "pcps_acquisition_adapters.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static int g_fail = 0;
#define EXPECT(cond, ...)                                       \
    do                                                          \
        {                                                       \
            if (!(cond))                                        \
                {                                               \
                    std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                    std::printf(__VA_ARGS__);                   \
                    std::printf("\n");                          \
                    g_fail++;                                   \
                }                                               \
        }                                                       \
    while (0)

// ---- scripted blocks -------------------------------------------------------------------------------------------------------------

// one call of the search step: the items it consumes (and counts), the dwells it counts, the state it leaves
struct Step
{
    int32_t next_state;
    int consumed;
    uint32_t dwells;
};

struct Kind
{
    const char* name;
    hip_acquisition_item_block::Policy policy;
    uint32_t fft_size, item_length;
    bool needs_items;  // Tong and CAF return 0 from the search state without items; QuickSync and paired run their dwell whatever n says
    // what one item does when the engine fails, with max_dwells = 2 (the table of the block headers)
    std::vector<Step> on_error;
};

static std::vector<Kind> kinds()
{
    return {
        {"tong", {1, 1, 2, 3, false}, 8, 8, true, {{3, 1, 1}}},                    // one item consumed, dwell_count++, state 3
        {"quicksync", {1, 1, 2, 3, true}, 5, 12, false, {{1, 1, 1}, {3, 1, 1}}},   // the decision rule on a statistic of 0
        {"paired", {1, 1, 2, 3, false}, 6, 6, false, {{1, 1, 1}, {3, 1, 1}}},      // stays in 1 until the dwell count is max_dwells
        {"caf", {1, 2, 3, 4, false}, 10, 10, true, {{4, 1, 1}}},                   // state 4 at once
    };
}

class ScriptedBlock : public hip_acquisition_item_block
{
public:
    explicit ScriptedBlock(const Kind& k) : hip_acquisition_item_block(k.policy, 1, 2, 5000, 4000000, 4000, 4000, false, "", k.fft_size, k.item_length), d_needs_items(k.needs_items) {}

    void push(const std::vector<Step>& steps) { d_script.insert(d_script.end(), steps.begin(), steps.end()); }
    size_t steps_left() const { return d_script.size() - d_pos; }
    int restarts = 0, engines = 0, codes = 0;
    bool have_code = false;

private:
    gc_status create_engine() override
    {
        engines++;
        d_have_code = have_code;
        return GC_OK;
    }
    gc_status load_code() override
    {
        codes++;
        return GC_ERR_STATE;
    }
    void on_restart() override { restarts++; }
    int search(const gr_complex*, gc_stream*, uint64_t, int n_items) override
    {
        if (d_needs_items && n_items <= 0) return 0;
        if (d_pos >= d_script.size())
            {
                EXPECT(false, "search step called with an empty script");
                return 0;
            }
        const Step s = d_script[d_pos++];
        count_items(s.consumed);
        d_dwell_count += s.dwells;
        // a winner, so that the next restart has something to clear
        d_gnss_synchro->Acq_delay_samples = 123.0;
        d_gnss_synchro->Acq_doppler_hz = -250.0;
        d_gnss_synchro->Acq_samplestamp_samples = d_sample_counter;
        d_gnss_synchro->Acq_doppler_step = 250U;
        d_mag = 2.0f;
        d_input_power = 3.0f;
        d_test_statistics = 4.0f;
        d_state = s.next_state;
        return s.consumed;
    }

    bool d_needs_items;
    std::vector<Step> d_script;
    size_t d_pos = 0;
};

static void dirty(Gnss_Synchro& g)
{
    g.Acq_delay_samples = 9.0;
    g.Acq_doppler_hz = 9.0;
    g.Acq_samplestamp_samples = 9ULL;
    g.Acq_doppler_step = 9U;
}

static bool restart_cleared(const Gnss_Synchro& g) { return g.Acq_delay_samples == 0.0 && g.Acq_doppler_hz == 0.0 && g.Acq_samplestamp_samples == 0ULL && g.Acq_doppler_step == 0U; }

// the running expectation of one block
struct Driver
{
    const Kind& k;
    ScriptedBlock b;
    Gnss_Synchro g;
    uint64_t counter = 0;
    std::vector<int> events;
    std::vector<gr_complex> in;

    explicit Driver(const Kind& kind) : k(kind), b(kind), in(static_cast<size_t>(kind.item_length) * 3)
    {
        b.set_gnss_synchro(&g);
    }

    // one work() call: `consumed` items are expected back and counted, `state` is expected afterwards, `event` (0: none) is published
    void call(const char* what, int n_items, int consumed, int32_t state, int event = 0)
    {
        const int got = b.work(in.data(), n_items);
        counter += static_cast<uint64_t>(k.item_length) * static_cast<uint64_t>(consumed);
        if (event != 0) events.push_back(event);
        EXPECT(got == consumed, "%s, %s: consumed %d of %d, expected %d", k.name, what, got, n_items, consumed);
        EXPECT(b.sample_counter() == counter, "%s, %s: sample counter %llu, expected %llu", k.name, what, static_cast<unsigned long long>(b.sample_counter()),
            static_cast<unsigned long long>(counter));
        EXPECT(b.state() == state, "%s, %s: state %d, expected %d", k.name, what, b.state(), state);
        EXPECT(b.events() == events, "%s, %s: %zu events, expected %zu", k.name, what, b.events().size(), events.size());
    }

    // state 0 with d_active set: restart, go to the search state, consume everything
    void start(const char* what, int n_items)
    {
        const int before = b.restarts;
        dirty(g);
        call(what, n_items, n_items, k.policy.search_first);
        EXPECT(restart_cleared(g) && b.restarts == before + 1, "%s, %s: restart did not clear the synchro fields", k.name, what);
        EXPECT(b.dwell_count() == 0 && b.mag() == 0 && b.input_power() == 0.0f && b.test_statistics() == 0.0f, "%s, %s: restart left a count or a statistic", k.name, what);
    }

    // a further call in state 0 shows d_active: cleared, the block stays idle and restarts nothing
    void idle(const char* what, int n_items)
    {
        const int before = b.restarts;
        dirty(g);
        call(what, n_items, n_items, 0);
        EXPECT(!restart_cleared(g) && b.restarts == before, "%s, %s: an idle block restarted", k.name, what);
    }
};

static void drive(const Kind& k)
{
    const auto& p = k.policy;
    Driver d(k);
    // init(): clears all eight synchro fields, creates the engine, loads a code only if there is one
    d.g.Flag_valid_acquisition = d.g.Flag_valid_symbol_output = d.g.Flag_valid_pseudorange = d.g.Flag_valid_word = true;
    dirty(d.g);
    d.b.init();
    EXPECT(!d.g.Flag_valid_acquisition && !d.g.Flag_valid_symbol_output && !d.g.Flag_valid_pseudorange && !d.g.Flag_valid_word && restart_cleared(d.g), "%s: init() left a synchro field",
        k.name);
    EXPECT(d.b.engines == 1 && d.b.codes == 0 && d.b.last_status() == GC_OK && d.b.restarts == 0, "%s: init() without a code", k.name);
    d.b.have_code = true;
    d.b.init();
    EXPECT(d.b.engines == 2 && d.b.codes == 1 && d.b.last_status() == GC_ERR_STATE, "%s: init() re-installs the code and reports its status", k.name);
    EXPECT(d.b.fft_size() == k.fft_size && d.b.item_length() == k.item_length && d.b.state() == 0, "%s: sizes", k.name);

    // idle and not active: items are counted and consumed
    for (int n : {0, 1, 3}) d.idle("idle", n);

    // reset and find
    d.b.set_active(true);
    d.start("find: state 0", 3);
    d.b.push({{p.positive, 1, 1}});
    d.call("find: dwell", 2, 1, p.positive);
    EXPECT(d.b.dwell_count() == 1 && d.g.Acq_samplestamp_samples == d.counter, "%s, find: dwell count %u", k.name, d.b.dwell_count());
    d.call("find: positive state", 3, 3, 0, 1);
    d.idle("find: afterwards", 1);

    // reset and fail at max_dwells = 2; the block is started without items and the verdict published without items
    d.b.set_active(true);
    d.start("fail: state 0", 0);
    if (k.needs_items)
        d.call("fail: search state without items", 0, 0, p.search_first);
    d.b.push({{p.search_last, 1, 1}, {p.negative, 1, 1}});
    d.call("fail: dwell 1", 1, 1, p.search_last);  // CAF: state 2 is a search state too
    d.call("fail: dwell 2", 3, 1, p.negative);
    EXPECT(d.b.dwell_count() == 2, "%s, fail: dwell count %u", k.name, d.b.dwell_count());
    d.call("fail: negative state", 0, 0, 0, 2);
    d.idle("fail: afterwards", 3);

    // two searches in a row: the second starts from zeroed counts; Tong-like steps that ran several dwells in one call
    d.b.set_active(true);
    d.start("second search: state 0", 1);
    d.b.push({{p.positive, 2, 2}});
    d.call("second search: two dwells in one call", 3, 2, p.positive);
    EXPECT(d.b.dwell_count() == 2, "%s, second search: dwell count %u", k.name, d.b.dwell_count());
    d.call("second search: positive state", 1, 1, 0, 1);
    d.idle("second search: afterwards", 0);

    // engine error: the block's own path to the negative state
    d.b.set_active(true);
    d.start("error: state 0", 1);
    d.b.push(k.on_error);
    for (size_t i = 0; i < k.on_error.size(); i++) d.call("error: item", 1, 1, k.on_error[i].next_state);
    EXPECT(d.b.dwell_count() == k.on_error.size() && d.b.state() == p.negative, "%s, error: %u dwells", k.name, d.b.dwell_count());
    d.call("error: negative state", 1, 1, 0, 2);
    d.idle("error: afterwards", 1);

    // set_state(1) from outside restarts; only the QuickSync kind also sets d_active, which state 0 then shows
    {
        const int before = d.b.restarts;
        dirty(d.g);
        d.b.set_state(1);
        EXPECT(d.b.state() == 1 && restart_cleared(d.g) && d.b.restarts == before + 1, "%s: set_state(1) did not restart", k.name);
        d.b.push({{p.negative, 1, 1}});
        d.call("set_state(1): dwell", 1, 1, p.negative);
        d.b.set_state(0);  // back to idle without the terminal state's clearing of d_active
        EXPECT(d.b.restarts == before + 1, "%s: set_state(0) restarted", k.name);
        if (p.set_state_activates)
            {
                d.start("set_state(1) had activated", 1);
                d.b.set_state(p.negative);
                d.call("set_state(1): negative state", 1, 1, 0, 2);
            }
        d.idle("set_state(1): afterwards", 1);
    }

    // terminal states entered from outside, with 0, 1 and 3 items; a state outside the numbering consumes nothing
    for (int n : {0, 1, 3})
        {
            d.b.set_state(p.positive);
            d.call("positive state", n, n, 0, 1);
            d.b.set_state(p.negative);
            d.call("negative state", n, n, 0, 2);
            d.idle("after a terminal state", n);
        }
    d.b.set_state(p.negative + 1);
    d.call("unknown state", 3, 0, p.negative + 1);
    d.b.set_state(0);
    EXPECT(d.b.steps_left() == 0, "%s: %zu scripted steps were not run", k.name, d.b.steps_left());
    d.b.clear_events();
    EXPECT(d.b.events().empty(), "%s: clear_events", k.name);
}

// ---- Doppler bins and the threshold rule -----------------------------------------------------------------------------------------

// calculate_threshold as PcpsAcquisitionHip and GalileoE1PairedAcquisitionHip had it, members turned into parameters
static float old_calculate_threshold(float pfa, unsigned int vector_length_, unsigned int doppler_max_, unsigned int doppler_step_)
{
    unsigned int frequency_bins = 0;
    for (int doppler = static_cast<int>(-doppler_max_); doppler <= static_cast<int>(doppler_max_); doppler += doppler_step_) frequency_bins++;
    unsigned int ncells = vector_length_ * frequency_bins;
    double exponent = 1 / static_cast<double>(ncells);
    double val = std::pow(1.0 - pfa, exponent);
    auto lambda = double(vector_length_);
    return static_cast<float>(-std::log(1.0 - val) / lambda);
}

static void helper_tests()
{
    using gnsscorr::inclusive_doppler_bins;
    // the five loops agreed on these: -5000 .. 5000 by 250; the one bin at 0; -10000 .. 9980 by 333
    EXPECT(inclusive_doppler_bins(5000, 250) == 41, "5000 / 250: %u", inclusive_doppler_bins(5000, 250));
    EXPECT(inclusive_doppler_bins(0, 250) == 1, "0 / 250: %u", inclusive_doppler_bins(0, 250));
    EXPECT(inclusive_doppler_bins(10000, 333) == 61, "10000 / 333: %u", inclusive_doppler_bins(10000, 333));
    // a step of 0: the CAF copy gave 0 bins, the Tong and QuickSync copies made it 250 first (their wrappers still do), the paired copy
    // and the adapters' rule did not end
    EXPECT(inclusive_doppler_bins(5000, 0) == 0, "5000 / 0: %u", inclusive_doppler_bins(5000, 0));
    uint32_t step = 0;
    EXPECT(gnsscorr::tong_doppler_bins(5000, 0) == 41 && gnsscorr::quicksync_doppler_bins(5000, step) == 41 && step == 250, "the wrappers' 0 means 250");
    // doppler_max + doppler_step past 2^31: -1.5e9, -0.5e9, 0.5e9, 1.5e9 are 4 bins, which the int64_t copies (Tong, CAF) counted.  The
    // int32_t copies wrapped at the fifth value and went on counting; the shared function follows the 64-bit copies, whose count is
    // the number of values in the range
    EXPECT(inclusive_doppler_bins(1500000000U, 1000000000U) == 4, "1.5e9 / 1e9: %u", inclusive_doppler_bins(1500000000U, 1000000000U));

    struct
    {
        float pfa;
        unsigned int length, max, step;
    } const cases[] = {{0.001f, 4000, 5000, 250}, {0.01f, 16000, 10000, 250}, {1e-6f, 32000, 10000, 125}, {0.1f, 2048, 5000, 500}, {0.001f, 8000, 0, 250}, {0.5f, 1, 1000, 300},
        {0.001f, 32000, 10000, 333}};
    for (const auto& c : cases)
        {
            const float want = old_calculate_threshold(c.pfa, c.length, c.max, c.step);
            const float got = gnsscorr::exponential_quantile_threshold(c.pfa, c.length, c.max, c.step);
            EXPECT(std::memcmp(&want, &got, sizeof want) == 0 && want > 0.0f, "threshold(%g, %u, %u, %u): %a, calculate_threshold gave %a", c.pfa, c.length, c.max, c.step, got, want);
        }

    // a Pfa with a step of 0 (set_threshold before set_doppler_step): the given threshold stays installed
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1C.pfa", "0.001");
    GpsL1CaPcpsAcquisitionHip acq(&config, "Acquisition_1C", 1, 0);
    acq.set_threshold(0.37f);
    EXPECT(acq.threshold() == 0.37f, "PcpsAcquisitionHip, step 0: threshold %g", acq.threshold());
    acq.set_doppler_step(250);
    acq.set_threshold(0.37f);
    const float want = old_calculate_threshold(0.001f, 4000, 5000, 250);
    EXPECT(acq.threshold() == want && acq.vector_length() == 4000, "PcpsAcquisitionHip, step 250: threshold %g, expected %g", acq.threshold(), want);
    config.set_property("Acquisition_1B.pfa", "0.001");
    config.set_property("Acquisition_1B.coherent_integration_time_ms", "8");
    GalileoE1Pcps8msAmbiguousAcquisitionHip e8(&config, "Acquisition_1B", 1, 0);
    e8.set_threshold(0.21f);
    EXPECT(e8.threshold() == 0.21f, "8 ms adapter, step 0: threshold %g", e8.threshold());

    // tile_code: reps copies, nothing behind them
    std::vector<gr_complex> one = {{1.0f, 2.0f}, {3.0f, 4.0f}, {5.0f, 6.0f}}, tiled(8, gr_complex(-1.0f, -1.0f));
    gnsscorr::tile_code(one.data(), 3, 2, tiled.data());
    EXPECT(tiled[0] == one[0] && tiled[2] == one[2] && tiled[3] == one[0] && tiled[5] == one[2] && tiled[6] == gr_complex(-1.0f, -1.0f), "tile_code");
}

// ---- the real blocks without a device --------------------------------------------------------------------------------------------

static void no_device_tests()
{
    EXPECT(gnsscorr::shared_context() == nullptr, "a device is visible: this program is meant to run without one");
    if (gnsscorr::shared_context() != nullptr) return;
    std::vector<gr_complex> item(32000, gr_complex(0.0f, 0.0f));
    {
        Gnss_Synchro g;
        hip_pcps_tong_acquisition b(1, 5000, 4000000, 4000, 4000, 1, 2, 3, false, "");
        b.set_gnss_synchro(&g);
        b.init();
        EXPECT(b.last_status() == GC_ERR_NO_DEVICE && b.engine() == nullptr && b.num_doppler_bins() == 41, "tong: init status %d, %u bins (a step of 0 means 250)", b.last_status(),
            b.num_doppler_bins());
        b.set_state(1);
        // one item consumed, dwell_count++, state 3
        EXPECT(b.work(item.data(), 2) == 1 && b.state() == 3 && b.dwell_count() == 1 && b.sample_counter() == 4000 && b.last_status() == GC_ERR_STATE, "tong: error path, state %d",
            b.state());
        EXPECT(b.work_ring(nullptr, 0, 1) == 1 && b.state() == 0 && b.events() == std::vector<int>{2}, "tong: ACQ_FAIL");
    }
    {
        Gnss_Synchro g;
        hip_pcps_quicksync_acquisition b(2, 4, 2, 5000, 4000000, 4000, 4000, false, false, "");
        b.set_gnss_synchro(&g);
        b.init();
        EXPECT(b.last_status() == GC_ERR_NO_DEVICE && b.num_doppler_bins() == 41 && b.fft_size() == 2000 && b.item_length() == 16000, "quicksync: init status %d", b.last_status());
        b.set_state(1);
        // the decision rule on a statistic of 0: dwell 1 of 2 stays in state 1, dwell 2 is negative; the counter moves before the dwell
        EXPECT(b.work(item.data(), 1) == 1 && b.state() == 1 && b.dwell_count() == 1 && b.sample_counter() == 16000 && b.last_status() == GC_ERR_STATE, "quicksync: dwell 1, state %d",
            b.state());
        EXPECT(b.work(item.data(), 1) == 1 && b.state() == 3 && b.dwell_count() == 2 && b.sample_counter() == 32000, "quicksync: dwell 2, state %d", b.state());
        EXPECT(b.work(item.data(), 1) == 1 && b.state() == 0 && b.events() == std::vector<int>{2}, "quicksync: ACQ_FAIL");
        // set_state(1) had set d_active, the negative state cleared it
        EXPECT(b.work(item.data(), 1) == 1 && b.state() == 0, "quicksync: idle afterwards");
    }
    for (auto kind : {hip_pcps_paired_acquisition::CCCWSR, hip_pcps_paired_acquisition::E1_8MS})
        {
            Gnss_Synchro g;
            hip_pcps_paired_acquisition b(kind, 4, 2, 10000, 4000000, 4000, 16000, false, "");
            b.set_gnss_synchro(&g);
            b.init();
            EXPECT(b.last_status() == GC_ERR_INVALID && b.num_doppler_bins() == 0, "paired: a step of 0 is refused, status %d", b.last_status());
            b.set_doppler_step(250);
            b.init();
            EXPECT(b.last_status() == GC_ERR_NO_DEVICE && b.num_doppler_bins() == 81 && b.fft_size() == 16000, "paired: init status %d, %u bins", b.last_status(), b.num_doppler_bins());
            b.set_state(1);
            // stays in state 1 until the dwell count is max_dwells, then 3
            EXPECT(b.work(item.data(), 1) == 1 && b.state() == 1 && b.dwell_count() == 1 && b.last_status() == GC_ERR_STATE, "paired: dwell 1, state %d", b.state());
            EXPECT(b.work(item.data(), 1) == 1 && b.state() == 3 && b.dwell_count() == 2 && b.sample_counter() == 32000, "paired: dwell 2, state %d", b.state());
            EXPECT(b.work(item.data(), 1) == 1 && b.state() == 0 && b.events() == std::vector<int>{2}, "paired: ACQ_FAIL");
        }
    {
        Gnss_Synchro g;
        hip_e5a_noncoherent_iq_acquisition_caf b(1, 2, 5000, 2000000, 2000, 2000, false, false, "", true, 0, 0);
        b.set_gnss_synchro(&g);
        b.init();
        EXPECT(b.last_status() == GC_ERR_NO_DEVICE && b.num_doppler_bins() == 41, "caf: init status %d, %u bins (the step starts at 250)", b.last_status(), b.num_doppler_bins());
        b.set_state(1);
        // state 4 at once; the earlier error status is kept when there is no engine
        EXPECT(b.work(item.data(), 1) == 1 && b.state() == 4 && b.well_count() == 1 && b.sample_counter() == 2000 && b.last_status() == GC_ERR_NO_DEVICE, "caf: error path, state %d",
            b.state());
        EXPECT(b.work_ring(nullptr, 0, 1) == 1 && b.state() == 0 && b.events() == std::vector<int>{2}, "caf: ACQ_FAIL");
    }
    {
        Gnss_Synchro g;
        hip_pcps_acquisition_fine_doppler b(1, 5000, 4000000, 4000, false, false, "");
        b.set_gnss_synchro(&g);
        b.set_doppler_step(250);
        b.init();
        EXPECT(b.last_status() == GC_ERR_NO_DEVICE && b.engine() == nullptr && b.fine_engine() == nullptr && b.num_doppler_bins() == 40, "fine Doppler: init status %d", b.last_status());
        b.set_state(1);
        EXPECT(b.work(item.data(), 4000) == 4000 && b.state() == 5 && b.last_status() == GC_ERR_STATE, "fine Doppler: error path, state %d", b.state());
        EXPECT(b.work(item.data(), 100) == 100 && b.state() == 0 && b.events() == std::vector<int>{2}, "fine Doppler: ACQ_FAIL");
    }
    {
        InMemoryConfiguration config;
        config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
        Gnss_Synchro g;
        GpsL1CaPcpsAcquisitionHip acq(&config, "Acquisition_1C", 1, 0);
        acq.set_gnss_synchro(&g);
        acq.set_doppler_step(250);
        acq.init();
        EXPECT(acq.block()->last_status() == GC_ERR_NO_DEVICE, "pcps: init status %d", acq.block()->last_status());
    }
}

int main()
{
    for (const Kind& k : kinds()) drive(k);
    helper_tests();
    no_device_tests();
    if (g_fail == 0) std::printf("acq block self-test passed\n");
    return g_fail == 0 ? 0 : 1;
}
