// glonass_loop_selftest.cpp -- the GLONASS C/A tracking block on the device loop against the host-loop block, on the GPU:
//   1. hip_glonass_ca_dll_pll_tracking_dev (items pushed in uneven pieces) against hip_glonass_ca_dll_pll_tracking (one level-1
//      correlator launch per period) on the same samples, item by item, the pull-in item included: Tracking_sample_counter equal,
//      prompt within 3e-3 of |prompt|, Doppler within 0.05 Hz, C/N0 within 0.05 dB (the gates of the device loop's GPU tests);
//   2. hip_glonass_tracking_group with 4 slots of different frequency channels on one ring against 4 single device blocks.
// The scenarios are checked for soundness on the way: every period's block length is at least 1e-3 sample away from a rounding
// boundary (|Code_phase_samples| <= 0.499), so that a last-bit difference in a correlator sum cannot move a block.
// Usage: glonass_loop_selftest (needs a GPU).
#include "hip_glonass_tracking_group.h"
#include <cmath>
#include <cstdio>
#include <random>
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

static const double FS = 6.625e6, BAND_HZ = 1.602e9, DFRQ_HZ = 0.5625e6;
static const uint32_t VL = 6625;
static const int PERIODS = 64;

struct Sat
{
    uint32_t prn;
    double doppler_hz, delay_samples;
};

// unit-variance complex noise plus one C/A signal per satellite on its own frequency channel, each with a small carrier phase at
// the sample its tracking starts on (the block's second-order loop is lightly damped: a phase step at hand-over rings for tens of periods)
static std::vector<gr_complex> synth(const std::vector<Sat>& sats, size_t n, double cn0_dbhz, unsigned seed)
{
    std::vector<float> code(511);
    gc_glonass_l1_ca_code_gen_float(code.data(), 0);
    std::mt19937 gen(seed);
    std::normal_distribution<float> nd(0.0f, std::sqrt(0.5f));
    std::vector<gr_complex> x(n);
    for (auto& v : x) v = gr_complex(nd(gen), nd(gen));
    const double amp = std::sqrt(std::pow(10.0, cn0_dbhz / 10.0) / FS);
    for (const Sat& s : sats)
        {
            const double f_channel = DFRQ_HZ * gnsscorr::glonass_default_channels().at(s.prn);
            const double rate = 0.511e6 * (1.0 + s.doppler_hz / (BAND_HZ + f_channel)) / FS;
            const double tau0 = 511.0 - s.delay_samples * 0.511e6 / FS;
            const double first = s.delay_samples + VL;  // about where the pull-in puts the first tracked sample
            for (size_t i = 0; i < n; i++)
                {
                    const double ph = 2.0 * M_PI * std::fmod((f_channel + s.doppler_hz) * (static_cast<double>(i) - first) / FS, 1.0) + 0.05;
                    const size_t chip = static_cast<size_t>(std::floor(tau0 + static_cast<double>(i) * rate)) % 511;
                    x[i] += gr_complex(static_cast<float>(amp * code[chip] * std::cos(ph)), static_cast<float>(amp * code[chip] * std::sin(ph)));
                }
        }
    return x;
}

static Gnss_Synchro acquisition(const Sat& s)
{
    Gnss_Synchro syn;
    syn.System = 'R';
    syn.Signal[0] = '1';
    syn.Signal[1] = 'G';
    syn.PRN = s.prn;
    syn.Acq_delay_samples = s.delay_samples;
    syn.Acq_doppler_hz = s.doppler_hz + 0.5;
    syn.Acq_samplestamp_samples = 0;
    return syn;
}

// items of the host-loop block: one per work() call
static std::vector<Gnss_Synchro> run_host_block(const std::vector<gr_complex>& x, Gnss_Synchro syn, int max_items)
{
    hip_glonass_ca_dll_pll_tracking blk(1, static_cast<int64_t>(FS), VL, 35.0f, 2.0f, 0.5f, 10, 25, 50, 0.85);
    blk.set_gnss_synchro(&syn);
    blk.start_tracking();
    std::vector<Gnss_Synchro> items;
    size_t pos = 0;
    while (pos + blk.required_input_items() <= x.size() && static_cast<int>(items.size()) < max_items)
        {
            Gnss_Synchro out;
            int produced = 0;
            pos += blk.work(x.data() + pos, static_cast<int>(x.size() - pos), &out, &produced);
            items.push_back(out);
        }
    EXPECT(blk.last_status() == GC_OK && blk.tracking_enabled(), "host block: status %d (%s)", blk.last_status(), gc_last_error());
    return items;
}

// items of the device-loop block, its input arriving in uneven pieces
static std::vector<Gnss_Synchro> run_dev_block(const std::vector<gr_complex>& x, Gnss_Synchro syn)
{
    hip_glonass_ca_dll_pll_tracking_dev blk(1, static_cast<int64_t>(FS), VL, 35.0f, 2.0f, 0.5f, 10, 25, 50, 0.85);
    blk.set_gnss_synchro(&syn);
    blk.start_tracking();
    std::vector<Gnss_Synchro> items, out(80);
    const size_t pieces[] = {3000, 9000, 500, 13250, 6625, 100, 20000, 1, 6624, 7000};
    size_t consumed = 0, available = 0, k = 0;
    while (available < x.size())
        {
            available = std::min(x.size(), available + pieces[k++ % 10]);
            int produced = 0;
            consumed += blk.work(x.data() + consumed, static_cast<int>(available - consumed), out.data(), static_cast<int>(out.size()), &produced);
            items.insert(items.end(), out.begin(), out.begin() + produced);
            if (blk.last_status() != GC_OK) break;
        }
    EXPECT(blk.last_status() == GC_OK && blk.tracking_enabled() && blk.events().empty(), "device block: status %d (%s), state %d", blk.last_status(), gc_last_error(),
        blk.state());
    return items;
}

// the gates of the device loop's GPU tests on two item lists; returns the number of items compared
static size_t compare(const char* what, const std::vector<Gnss_Synchro>& a, const std::vector<Gnss_Synchro>& b)
{
    const size_t n = std::min(a.size(), b.size());
    double worst_prompt = 0.0, worst_doppler = 0.0, worst_cn0 = 0.0;
    for (size_t k = 0; k < n; k++)
        {
            const Gnss_Synchro &p = a[k], &q = b[k];
            EXPECT(p.Tracking_sample_counter == q.Tracking_sample_counter, "%s item %zu: Tracking_sample_counter %llu / %llu", what, k,
                (unsigned long long)p.Tracking_sample_counter, (unsigned long long)q.Tracking_sample_counter);
            EXPECT(p.Flag_valid_symbol_output == q.Flag_valid_symbol_output && p.Flag_valid_symbol_output == (k > 0), "%s item %zu: valid flags %d / %d", what, k,
                p.Flag_valid_symbol_output, q.Flag_valid_symbol_output);
            EXPECT(p.PRN == q.PRN && p.fs == q.fs && p.correlation_length_ms == 1 && q.correlation_length_ms == 1, "%s item %zu: header fields", what, k);
            const double scale = std::hypot(p.Prompt_I, p.Prompt_Q) + 1e-9;
            const double dp = std::hypot(p.Prompt_I - q.Prompt_I, p.Prompt_Q - q.Prompt_Q) / scale;
            if (k > 0) worst_prompt = std::max(worst_prompt, dp);
            worst_doppler = std::max(worst_doppler, std::fabs(p.Carrier_Doppler_hz - q.Carrier_Doppler_hz));
            worst_cn0 = std::max(worst_cn0, std::fabs(p.CN0_dB_hz - q.CN0_dB_hz));
            EXPECT(k == 0 || dp <= 3e-3, "%s item %zu: prompt differs by %.3g of |prompt|", what, k, dp);
            EXPECT(std::fabs(p.Carrier_Doppler_hz - q.Carrier_Doppler_hz) < 0.05, "%s item %zu: Doppler %.4f / %.4f", what, k, p.Carrier_Doppler_hz, q.Carrier_Doppler_hz);
            EXPECT(std::fabs(p.CN0_dB_hz - q.CN0_dB_hz) < 0.05, "%s item %zu: C/N0 %.3f / %.3f", what, k, p.CN0_dB_hz, q.CN0_dB_hz);
            EXPECT(std::fabs(p.Code_phase_samples - q.Code_phase_samples) < 1e-3, "%s item %zu: code phase %.5f / %.5f", what, k, p.Code_phase_samples, q.Code_phase_samples);
            EXPECT(std::fabs(p.Carrier_phase_rads - q.Carrier_phase_rads) < 0.05, "%s item %zu: carrier phase %.4f / %.4f", what, k, p.Carrier_phase_rads, q.Carrier_phase_rads);
            EXPECT(std::fabs(p.Code_phase_samples) <= 0.499, "%s item %zu: the scenario's block length is within 1e-3 sample of a rounding boundary", what, k);
        }
    std::printf("%s: %zu items, worst prompt %.2e of |prompt|, Doppler %.2e Hz, C/N0 %.2e dB\n", what, n, worst_prompt, worst_doppler, worst_cn0);
    return n;
}

static void test_device_block_against_host_block()
{
    const Sat sat = {22, 700.0, 1343.1};  // slot 22: frequency channel -3
    const auto x = synth({sat}, static_cast<size_t>(VL) * (PERIODS + 3), 74.0, 51);
    const auto host = run_host_block(x, acquisition(sat), PERIODS);
    const auto dev = run_dev_block(x, acquisition(sat));
    EXPECT(host.size() >= 60 && dev.size() >= 60, "items: host %zu, device %zu", host.size(), dev.size());
    const size_t n = compare("device block / host block", host, dev);
    EXPECT(n >= 60, "only %zu items compared", n);
    if (n > 0) EXPECT(std::fabs(dev[n - 1].Carrier_Doppler_hz - sat.doppler_hz) < 3.0 && dev[n - 1].CN0_dB_hz > 60.0, "device block: Doppler %.2f, C/N0 %.1f", dev[n - 1].Carrier_Doppler_hz, dev[n - 1].CN0_dB_hz);
}

static void test_group_against_single_blocks()
{
    // slots 1, 2, 3, 12: frequency channels +1, -4, +5, -1
    const std::vector<Sat> sats = {{1, -800.0, 4410.1}, {2, 650.0, 127.9}, {3, 1000.0, 2222.1}, {12, -420.0, 5801.2}};
    const auto x = synth(sats, static_cast<size_t>(VL) * (PERIODS + 3), 74.0, 61);
    gc_ctx* ctx = nullptr;
    gc_stream* ring = nullptr;
    EXPECT(gc_ctx_create(0, &ctx) == GC_OK, "gc_ctx_create: %s", gc_last_error());
    EXPECT(gc_stream_create(ctx, GC_IQ_F32, static_cast<uint64_t>(VL) * 80, 2 * VL, &ring) == GC_OK, "gc_stream_create: %s", gc_last_error());
    std::vector<std::vector<Gnss_Synchro>> items;
    {
        gnsscorr::GlonassTrkConf conf;
        conf.band = 1;
        conf.fs_in = static_cast<int64_t>(FS);
        conf.vector_length = VL;
        conf.pll_bw_hz = 35.0f;
        conf.dll_bw_hz = 2.0f;
        conf.early_late_space_chips = 0.5f;
        conf.cn0_samples = 10;
        hip_glonass_tracking_group group(ctx, ring, conf, 5);  // slot 4 stays free
        EXPECT(group.last_status() == GC_OK, "group: %s", gc_last_error());
        for (int ch = 0; ch < 4; ch++) EXPECT(group.start_tracking(ch, acquisition(sats[ch]), 0) == GC_OK, "group start %d: %s", ch, gc_last_error());
        const size_t pieces[] = {7000, 300, 26500, 6625, 1, 13249};
        size_t pushed = 0, k = 0;
        while (pushed < x.size())
            {
                const size_t n = std::min(x.size() - pushed, pieces[k++ % 6]);
                EXPECT(gc_stream_push(ring, x.data() + pushed, n, nullptr) == GC_OK, "push: %s", gc_last_error());
                pushed += n;
                EXPECT(group.run(items) >= 0, "group run: %s", gc_last_error());
            }
        for (int ch = 0; ch < 4; ch++) EXPECT(group.active(ch) && group.events(ch).empty(), "group slot %d lost lock", ch);
        EXPECT(items.size() == 5 && items[4].empty(), "the free slot produced items");
    }
    for (int ch = 0; ch < 4; ch++)
        {
            const auto single = run_dev_block(x, acquisition(sats[ch]));
            char what[64];
            std::snprintf(what, sizeof what, "group slot %d / single block", ch);
            const size_t n = compare(what, single, items[ch]);
            EXPECT(n >= 60 && single.size() == items[ch].size(), "%s: %zu / %zu items", what, single.size(), items[ch].size());
            if (n > 0) EXPECT(std::fabs(items[ch][n - 1].Carrier_Doppler_hz - sats[ch].doppler_hz) < 3.0, "group slot %d: Doppler %.2f", ch, items[ch][n - 1].Carrier_Doppler_hz);
        }
    gc_stream_destroy(ring);
    gc_ctx_destroy(ctx);
}

int main()
{
    test_device_block_against_host_block();
    test_group_against_single_blocks();
    if (g_fail)
        {
            std::printf("glonass_loop_selftest: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("glonass_loop_selftest: ok\n");
    return 0;
}
