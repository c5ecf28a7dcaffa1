// fine_doppler_selftest -- GpsL1CaPcpsAcquisitionFineDopplerHip over hip_pcps_acquisition_fine_doppler (the image of
// pcps_acquisition_fine_doppler_cc), and the fine_doppler flag of hip_acquisition_bank.
//   fine_doppler_selftest --host   the pieces that need no GPU: the bin count (+doppler_max excluded), the adapter's keys and
//                                  defaults, compute_CAF with its wrap cases, refusals of the library that need no device.  Creates
//                                  no GPU context.
//   fine_doppler_selftest          on synthetic GPS L1 C/A at 4 Msps: a satellite at -1762.5 Hz searched with a 500 Hz step is declared
//                                  and its Doppler reported within one fine bin (12.5 Hz), with the block's counters and stamps; a
//                                  noise-only search is negative; a bank with fine_doppler refines three satellites of five PRNs, the
//                                  other two stay absent, and the same search with the flag off is what it is without the parameter.
//                                  Needs a GPU (run by pytest -m gpu).
#include "hip_acquisition_bank.h"
#include "pcps_acquisition_adapters.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
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

// ---- host side -------------------------------------------------------------------------------------------------------------------

static void host_tests()
{
    using namespace gnsscorr;
    EXPECT(fine_doppler_bins(5000, 500) == 20 && fine_doppler_bins(5000, 250) == 40, "+doppler_max is not searched");
    EXPECT(fine_doppler_bins(5000, 300) == 33 && fine_doppler_bins(1000, 300) == 6 && fine_doppler_bins(5000, 0) == 0, "floor(2 * doppler_max / doppler_step)");
    EXPECT(fine_doppler_samples_per_chip(4000000) == 4 && fine_doppler_samples_per_chip(2048000) == 3, "samples per chip");
    {
        InMemoryConfiguration none;
        GpsL1CaPcpsAcquisitionFineDopplerHip d(&none, "Acquisition_1C", 1, 0);
        EXPECT(d.vector_length() == 2048 && d.block()->fft_size() == 2048 && d.block()->item_length() == 2048, "default rate: %u", d.vector_length());
        EXPECT(d.doppler_max() == 5000 && d.sampled_ms() == 1 && d.max_dwells() == 1 && !d.dump() && !d.blocking_on_standby() && d.dump_filename() == "./acquisition.mat",
            "defaults");
        EXPECT(d.implementation() == "GPS_L1_CA_PCPS_Acquisition_Fine_Doppler_HIP" && d.item_size() == sizeof(gr_complex), "implementation name");
        InMemoryConfiguration config;
        config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
        config.set_property("Acquisition_1C.doppler_max", "6000");
        config.set_property("Acquisition_1C.coherent_integration_time_ms", "3");
        config.set_property("Acquisition_1C.max_dwells", "2");
        config.set_property("Acquisition_1C.dump", "true");
        config.set_property("Acquisition_1C.dump_filename", "./x.mat");
        config.set_property("Acquisition_1C.blocking_on_standby", "true");
        GpsL1CaPcpsAcquisitionFineDopplerHip b(&config, "Acquisition_1C", 1, 0);
        // the transform is one millisecond whatever coherent_integration_time_ms says
        EXPECT(b.vector_length() == 4000 && b.block()->fft_size() == 4000 && b.sampled_ms() == 3, "keys: %u %u", b.vector_length(), b.block()->fft_size());
        EXPECT(b.doppler_max() == 6000 && b.max_dwells() == 2 && b.dump() && b.blocking_on_standby() && b.dump_filename() == "./x.mat", "keys");
        b.set_doppler_step(500);
        EXPECT(b.block()->num_doppler_bins() == 24, "6000 / 500: %u bins", b.block()->num_doppler_bins());
        b.set_doppler_max(5000);
        b.set_doppler_step(500);
        b.set_threshold(2.5f);
        EXPECT(b.block()->num_doppler_bins() == 20 && b.threshold() == 2.5f && b.block()->threshold() == 2.5f, "5000 / 500: %u bins", b.block()->num_doppler_bins());
        // blocking_on_standby: state 0 consumes nothing; no engine before init(): a dwell fails the search instead of hanging the channel
        Gnss_Synchro g;
        b.set_gnss_synchro(&g);
        std::vector<gr_complex> item(4000);
        EXPECT(b.block()->work(item.data(), 4000) == 0 && b.block()->sample_counter() == 0 && b.block()->state() == 0, "standby blocks");
        b.set_state(1);
        EXPECT(b.block()->work(item.data(), 4000) == 4000 && b.block()->state() == 5 && b.block()->last_status() == GC_ERR_STATE, "no engine: state %d", b.block()->state());
        EXPECT(b.block()->work(item.data(), 4000) == 0 && b.block()->events().size() == 1 && b.block()->events()[0] == 2 && b.block()->sample_counter() == 4000 &&
                b.block()->state() == 0, "ACQ_FAIL published");
    }
    {
        // compute_CAF on a 3 x 16 grid, 2 samples per chip: the first maximum with the bins ascending, the range [t - 2, t + 2) zeroed
        const uint32_t n = 16;
        std::vector<float> grid(3 * n, 1.0f);
        grid[1 * n + 8] = 10.0f;
        grid[2 * n + 3] = 10.0f;  // a later bin does not win a tie
        grid[1 * n + 6] = 7.0f;   // inside the range
        grid[1 * n + 10] = 6.0f;  // index 2 itself is NOT zeroed
        grid[1 * n + 12] = 5.0f;
        std::vector<float> g = grid;
        FineDopplerCaf r = fine_doppler_caf(g.data(), 3, n, 2);
        EXPECT(r.index_doppler == 1 && r.index_time == 8 && r.first_peak == 10.0f && r.second_peak == 6.0f && r.test_statistics == 10.0f / 6.0f, "CAF: bin %d, time %u, %g / %g",
            r.index_doppler, r.index_time, r.first_peak, r.second_peak);
        EXPECT(g[n + 6] == 0.0f && g[n + 7] == 0.0f && g[n + 8] == 0.0f && g[n + 9] == 0.0f && g[n + 10] == 6.0f && g[n + 5] == 1.0f, "CAF: the range is [6, 10)");
        EXPECT(g[2 * n + 3] == 10.0f && g[3] == 1.0f, "CAF: other rows stay");
        // the peak at index 1: index 1 of the range wraps to 15, index 2 stays 3
        g.assign(3 * n, 1.0f);
        g[1] = 9.0f;
        g[15] = 8.0f;
        g[3] = 4.0f;
        g[14] = 3.0f;
        r = fine_doppler_caf(g.data(), 3, n, 2);
        EXPECT(r.index_doppler == 0 && r.index_time == 1 && r.second_peak == 4.0f && g[15] == 0.0f && g[0] == 0.0f && g[2] == 0.0f && g[3] == 4.0f && g[14] == 3.0f,
            "CAF, low wrap: second %g", r.second_peak);
        // the peak at index 15: index 2 of the range wraps to 1 (17 - 16), index 1 stays 13
        g.assign(3 * n, 1.0f);
        g[2 * n + 15] = 9.0f;
        g[2 * n + 0] = 8.0f;
        g[2 * n + 1] = 5.0f;
        g[2 * n + 13] = 7.0f;
        g[2 * n + 12] = 2.0f;
        r = fine_doppler_caf(g.data(), 3, n, 2);
        EXPECT(r.index_doppler == 2 && r.index_time == 15 && r.second_peak == 5.0f && g[2 * n + 13] == 0.0f && g[2 * n + 0] == 0.0f && g[2 * n + 1] == 5.0f,
            "CAF, high wrap: second %g", r.second_peak);
        // the peak at index 14: index 2 is 16 - 16 = 0
        g.assign(3 * n, 1.0f);
        g[14] = 9.0f;
        g[0] = 6.0f;
        g[15] = 8.0f;
        r = fine_doppler_caf(g.data(), 3, n, 2);
        EXPECT(r.index_time == 14 && r.second_peak == 6.0f && g[15] == 0.0f && g[12] == 0.0f && g[0] == 6.0f, "CAF, range that ends at the array's end: second %g", r.second_peak);
        // an all-zero grid: bin 0, time 0, 0 / 0
        g.assign(3 * n, 0.0f);
        r = fine_doppler_caf(g.data(), 3, n, 2);
        EXPECT(r.index_doppler == 0 && r.index_time == 0 && r.first_peak == 0.0f && std::isnan(r.test_statistics), "CAF of zeros");
    }
    gc_fine_doppler* h = nullptr;
    gc_fine_doppler_conf c;
    std::memset(&c, 0, sizeof c);
    c.fs_in = 4000000;
    c.samples_per_code = 4000;
    c.prn_replicas = 10;
    c.zero_padding_factor = 8;
    c.window_hz = 1000.0f;
    EXPECT(gc_fine_doppler_create(nullptr, &c, 1, &h) == GC_ERR_INVALID && h == nullptr, "NULL context");
    c.prn_replicas = 51;
    EXPECT(gc_fine_doppler_create(nullptr, &c, 1, &h) == GC_ERR_INVALID && std::strstr(gc_last_error(), "prn_replicas") != nullptr, "P = 51: %s", gc_last_error());
    uint32_t first = 0, bins = 0;
    EXPECT(gc_fine_doppler_window(4000000, 320000, -1762.5, 1000.0, &first, &bins) == GC_OK && first == 320000 - 141 - 79 && bins == 159, "window %u %u", first, bins);
    EXPECT(gc_fine_doppler_estimate(nullptr, nullptr, nullptr, 1, nullptr) == GC_ERR_INVALID && gc_fine_doppler_destroy(nullptr) == GC_ERR_INVALID, "NULL handle");
}

// ---- GPU -------------------------------------------------------------------------------------------------------------------------

static const double kFs = 4e6;

// n samples: satellites prns[k] at dopplers[k] Hz whose code period starts at sample delays[k] (mod 4000), cn0 dB-Hz each, in noise of unit power
static std::vector<gr_complex> synth(size_t n, const std::vector<int>& prns, const std::vector<double>& dopplers, const std::vector<double>& delays, double cn0_db_hz,
    unsigned seed)
{
    std::vector<double> re(n, 0.0), im(n, 0.0);
    for (size_t k = 0; k < prns.size(); k++)
        {
            std::vector<float> code(1023);
            gc_gps_l1_ca_code_gen_float(code.data(), prns[k], 0);
            const double amp = std::sqrt(std::pow(10.0, cn0_db_hz / 10.0) / kFs);
            const double rate = 1.023e6 * (1.0 + dopplers[k] / 1575.42e6) / kFs;
            const double tau0 = 1023.0 - delays[k] * 1.023e6 / kFs;
            for (size_t i = 0; i < n; i++)
                {
                    const double ph = 2.0 * M_PI * std::fmod(dopplers[k] / kFs * static_cast<double>(i), 1.0) + 0.7 + static_cast<double>(k);
                    const size_t chip = static_cast<size_t>(std::floor(tau0 + static_cast<double>(i) * rate)) % 1023;
                    re[i] += amp * code[chip] * std::cos(ph);
                    im[i] += amp * code[chip] * std::sin(ph);
                }
        }
    std::mt19937 gen(seed);
    std::normal_distribution<double> nd(0.0, std::sqrt(0.5));
    std::vector<gr_complex> x(n);
    for (size_t i = 0; i < n; i++) x[i] = gr_complex(static_cast<float>(re[i] + nd(gen)), static_cast<float>(im[i] + nd(gen)));
    return x;
}

// the scheduler: hands the block one forecast's worth of samples per call until it has published an event
static size_t run_block(GpsL1CaPcpsAcquisitionFineDopplerHip& acq, const std::vector<gr_complex>& x)
{
    auto blk = acq.block();
    const size_t item = blk->item_length();
    size_t pos = 0;
    int guard = 0;
    while (blk->events().empty() && guard++ < 1000 && x.size() - pos >= item) pos += static_cast<size_t>(blk->work(x.data() + pos, static_cast<int>(item)));
    return pos;
}

static void setup(GpsL1CaPcpsAcquisitionFineDopplerHip& acq, Gnss_Synchro& g, uint32_t prn, float threshold)
{
    g.System = 'G';
    g.Signal[0] = '1';
    g.Signal[1] = 'C';
    g.PRN = prn;
    acq.set_channel(0);
    acq.set_gnss_synchro(&g);
    acq.set_doppler_max(5000);
    acq.set_doppler_step(500);
    acq.set_threshold(threshold);
    acq.init();
    acq.set_local_code();
    acq.set_state(1);
}

static void test_block()
{
    // first peak / second peak of the winner's row: about 1.1 - 1.5 in noise, above 10 for 50 dB-Hz after two 1 ms dwells
    const float kThreshold = 3.0f;
    const double kDoppler = -1762.5, kDelay = 1234.0;
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1C.max_dwells", "2");
    const auto x = synth(48000, {5}, {kDoppler}, {kDelay}, 50.0, 17);
    {
        Gnss_Synchro g;
        GpsL1CaPcpsAcquisitionFineDopplerHip acq(&config, "Acquisition_1C", 1, 0);
        setup(acq, g, 5, kThreshold);
        auto blk = acq.block();
        EXPECT(blk->last_status() == GC_OK, "engines: %s", gc_last_error());
        EXPECT(blk->fft_size() == 4000 && blk->num_doppler_bins() == 20, "sizes %u %u", blk->fft_size(), blk->num_doppler_bins());
        const size_t used = run_block(acq, x);
        EXPECT(blk->events().size() == 1 && blk->events()[0] == 1 && blk->positive_acq() == 1, "expected ACQ SUCCESS (statistic %g, %s)", blk->test_statistics(), gc_last_error());
        // two dwells, 32000 more samples for the 10 ms, one item for the event
        EXPECT(blk->well_count() == 2 && g.Acq_samplestamp_samples == 8000 && blk->sample_counter() == 44000 && used == 44000 && g.Acq_doppler_step == 500,
            "dwells %u, stamp %llu, counter %llu, used %zu", blk->well_count(), static_cast<unsigned long long>(g.Acq_samplestamp_samples),
            static_cast<unsigned long long>(blk->sample_counter()), used);
        EXPECT(std::abs(g.Acq_delay_samples - kDelay) <= 2.0, "delay %g", g.Acq_delay_samples);
        const double coarse = blk->caf().index_doppler * 500.0 - 5000.0;
        EXPECT(coarse == -2000.0 || coarse == -1500.0, "coarse Doppler %g", coarse);
        const gc_fine_doppler_result& f = blk->fine_result();
        EXPECT(f.status == GC_FINE_REFINED && f.window_bins == 159 && g.Acq_doppler_hz == f.doppler_hz, "fine stage: status %d, %u bins, %g Hz", f.status, f.window_bins, f.doppler_hz);
        EXPECT(std::abs(g.Acq_doppler_hz - kDoppler) <= 12.5 && g.Acq_doppler_hz != coarse, "Doppler %g Hz, expected %g within one fine bin", g.Acq_doppler_hz, kDoppler);
        EXPECT(f.peak > 100.0f * f.mean, "fine peak %g against mean %g", f.peak, f.mean);
        std::printf("fine Doppler acquisition: delay %g samples, coarse %g Hz, fine %g Hz, statistic %g, peak / mean %g\n", g.Acq_delay_samples, coarse, g.Acq_doppler_hz,
            blk->test_statistics(), f.peak / f.mean);
        // reset() + state 0 starts the next search (the channel's way)
        acq.reset();
        EXPECT(blk->work(x.data(), 4000) == 4000 && blk->state() == 1 && blk->well_count() == 0, "restart: state %d", blk->state());
    }
    {
        // noise only
        const auto noise = synth(48000, {}, {}, {}, 0.0, 18);
        Gnss_Synchro g;
        GpsL1CaPcpsAcquisitionFineDopplerHip acq(&config, "Acquisition_1C", 1, 0);
        setup(acq, g, 5, kThreshold);
        auto blk = acq.block();
        const size_t used = run_block(acq, noise);
        EXPECT(blk->events().size() == 1 && blk->events()[0] == 2 && blk->positive_acq() == 0, "noise: expected ACQ FAIL (statistic %g)", blk->test_statistics());
        EXPECT(blk->test_statistics() > 1.0f && blk->test_statistics() < kThreshold && used == 12000 && blk->fine_result().status == 0, "noise: statistic %g, used %zu",
            blk->test_statistics(), used);
        std::printf("fine Doppler acquisition, noise only: statistic %g\n", blk->test_statistics());
    }
}

static bool same(const Gnss_Synchro& a, const Gnss_Synchro& b)
{
    return a.PRN == b.PRN && a.System == b.System && a.Signal[0] == b.Signal[0] && a.Signal[1] == b.Signal[1] &&
           std::memcmp(&a.Acq_delay_samples, &b.Acq_delay_samples, sizeof(double)) == 0 && std::memcmp(&a.Acq_doppler_hz, &b.Acq_doppler_hz, sizeof(double)) == 0 &&
           a.Acq_samplestamp_samples == b.Acq_samplestamp_samples && a.Flag_valid_acquisition == b.Flag_valid_acquisition;
}

static void test_bank()
{
    const std::vector<uint32_t> prns = {3, 9, 14, 22, 30};
    const std::vector<int> present = {9, 22, 30};
    const std::vector<double> dopplers = {-1762.5, 2330.0, 412.5}, delays = {1234.0, 77.0, 3999.0};
    const size_t n = 4000 * 12;
    const auto x = synth(n + 1001, present, dopplers, delays, 50.0, 23);
    gc_ctx* ctx = gnsscorr::shared_context();
    gc_stream* ring = nullptr;
    EXPECT(ctx && gc_stream_create(ctx, GC_IQ_F32, 4000 * 16, 4000, &ring) == GC_OK, "ring: %s", gc_last_error());
    if (!ring) return;
    uint64_t first = 0;
    EXPECT(gc_stream_push(ring, x.data(), x.size(), &first) == GC_OK && first == 0, "push: %s", gc_last_error());
    {
        // statistic = peak / N^4 / input power: noise cells average 1 / N; 50 dB-Hz gives about 100 / N
        const float thr = 30.0f / 4000.0f;
        hip_acquisition_bank today(ctx, ring, 'G', "1C", prns, 4000000, 5000, 500, thr);
        hip_acquisition_bank off(ctx, ring, 'G', "1C", prns, 4000000, 5000, 500, thr, 1, true, GC_IQ_F32, false, false, false);
        hip_acquisition_bank fine(ctx, ring, 'G', "1C", prns, 4000000, 5000, 500, thr, 1, true, GC_IQ_F32, false, false, true);
        EXPECT(today.last_status() == GC_OK && off.last_status() == GC_OK && fine.last_status() == GC_OK, "banks: %d %d %d (%s)", today.last_status(), off.last_status(),
            fine.last_status(), gc_last_error());
        const uint64_t at = 1001;  // an odd index: the code periods start at delays[k] - 1001 (mod 4000)
        const auto a = today.search(at), b = off.search(at), c = fine.search(at);
        EXPECT(a.size() == 3 && b.size() == 3 && c.size() == 3, "detections %zu %zu %zu (%s)", a.size(), b.size(), c.size(), gc_last_error());
        EXPECT(fine.last_status() == GC_OK, "fine bank: %s", gc_last_error());
        for (size_t i = 0; i < a.size() && i < b.size() && i < c.size(); i++)
            {
                EXPECT(same(a[i], b[i]), "flag off: detection %zu differs from the bank without the parameter", i);
                EXPECT(a[i].PRN == c[i].PRN && a[i].Acq_delay_samples == c[i].Acq_delay_samples && a[i].Acq_samplestamp_samples == c[i].Acq_samplestamp_samples,
                    "flag on: detection %zu: PRN %u / %u, delay %g / %g", i, a[i].PRN, c[i].PRN, a[i].Acq_delay_samples, c[i].Acq_delay_samples);
                size_t k = 0;
                while (k < present.size() && static_cast<uint32_t>(present[k]) != c[i].PRN) k++;
                EXPECT(k < present.size(), "PRN %u is not in the signal", c[i].PRN);
                if (k == present.size()) continue;
                EXPECT(std::fmod(a[i].Acq_doppler_hz, 500.0) == 0.0 && std::abs(a[i].Acq_doppler_hz - dopplers[k]) <= 250.0, "PRN %u: coarse %g", a[i].PRN, a[i].Acq_doppler_hz);
                EXPECT(std::abs(c[i].Acq_doppler_hz - dopplers[k]) <= 12.5, "PRN %u: fine %g Hz, expected %g within one fine bin", c[i].PRN, c[i].Acq_doppler_hz, dopplers[k]);
                size_t slot = 0;
                while (prns[slot] != c[i].PRN) slot++;
                const gc_fine_doppler_result& f = fine.fine_result(slot);
                EXPECT(f.status == GC_FINE_REFINED && f.doppler_hz == c[i].Acq_doppler_hz && f.window_bins == 159, "PRN %u: stage status %d", c[i].PRN, f.status);
                std::printf("bank: PRN %u coarse %g Hz, fine %g Hz (true %g)\n", c[i].PRN, a[i].Acq_doppler_hz, c[i].Acq_doppler_hz, dopplers[k]);
            }
        // the two PRNs that are not in the signal were not refined
        EXPECT(fine.fine_result(0).status == 0 && fine.fine_result(2).status == 0 && fine.statistic(0) < thr && fine.statistic(2) < thr, "absent PRNs: %d %d",
            fine.fine_result(0).status, fine.fine_result(2).status);
        // a ring that does not hold the ten code periods yet: the detections keep the coarse Doppler, the status says why
        const auto late = fine.search(n + 1001 - 4000 * 3);
        EXPECT(late.size() == 3 && fine.last_status() == GC_ERR_INVALID, "late search: %zu detections, status %d", late.size(), fine.last_status());
        for (const auto& d : late) EXPECT(std::fmod(d.Acq_doppler_hz, 500.0) == 0.0, "late search: PRN %u keeps its coarse Doppler (%g)", d.PRN, d.Acq_doppler_hz);
        const auto again = fine.search(at);
        EXPECT(again.size() == c.size() && fine.last_status() == GC_OK, "a failed refinement is not sticky");
        for (size_t i = 0; i < again.size() && i < c.size(); i++) EXPECT(same(again[i], c[i]), "search %zu repeats", i);
    }
    gc_stream_destroy(ring);
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "--host")
        {
            host_tests();
            if (g_fail == 0) std::printf("fine doppler host self-test passed\n");
            return g_fail == 0 ? 0 : 1;
        }
    if (gc_device_count() == 0)
        {
            std::printf("no GPU: libgnsscorr has no CPU fallback\n");
            return 3;
        }
    test_block();
    test_bank();
    if (g_fail == 0) std::printf("fine doppler self-test passed\n");
    return g_fail == 0 ? 0 : 1;
}
