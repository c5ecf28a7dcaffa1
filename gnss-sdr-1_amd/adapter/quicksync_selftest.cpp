// quicksync_selftest -- the QuickSync adapters (hip_pcps_quicksync_acquisition.h: GpsL1CaPcpsQuickSyncAcquisitionHip and
// GalileoE1PcpsQuickSyncAmbiguousAcquisitionHip over hip_pcps_quicksync_acquisition).
//   quicksync_selftest --host               the pieces that need no GPU: inclusive bin count, rounding of
//                                           coherent_integration_time_ms, default folding factors, bit_transition_flag forcing two
//                                           dwells, the Pfa threshold rule, the decision machine of
//                                           pcps_quicksync_acquisition_cc.cc:503-527.  Creates no GPU context.
//   quicksync_selftest <tests/golden dir>   on the GPS L1 C/A (4 Msps, 2 ms, PRN 1) and Galileo E1 (4 Msps, 8 ms, PRN 1) captures,
//                                           f = 2: both are declared inside the gates of kat_expected.json; an absent PRN ends
//                                           negative at max_dwells; with bit_transition_flag the decision waits for the second
//                                           dwell.  Needs a GPU (run by pytest -m gpu).
#include "hip_pcps_quicksync_acquisition.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
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

static std::vector<gr_complex> read_iq(const std::string& path)
{
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    std::vector<gr_complex> v;
    if (!f) return v;
    size_t bytes = static_cast<size_t>(f.tellg());
    v.resize(bytes / sizeof(gr_complex));
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(gr_complex)));
    return v;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------

static void host_tests()
{
    using namespace gnsscorr;
    uint32_t step = 500;
    EXPECT(quicksync_doppler_bins(5000, step) == 21 && step == 500, "5000 / 500: both ends count");
    step = 250;
    EXPECT(quicksync_doppler_bins(5000, step) == 41, "5000 / 250");
    step = 0;
    EXPECT(quicksync_doppler_bins(5000, step) == 41 && step == 250, "a step of 0 means 250");
    step = 300;
    EXPECT(quicksync_doppler_bins(1000, step) == 7, "1000 / 300: -1000 .. 800");

    // gps :71-87 (multiple = f), galileo :79-96 (multiple = 4 f)
    EXPECT(quicksync_coherent_ms(4, 4) == 4 && quicksync_coherent_ms(6, 4) == 4 && quicksync_coherent_ms(2, 4) == 4 && quicksync_coherent_ms(9, 2) == 8, "GPS rounding");
    EXPECT(quicksync_coherent_ms(8, 8) == 8 && quicksync_coherent_ms(12, 8) == 8 && quicksync_coherent_ms(4, 8) == 8 && quicksync_coherent_ms(17, 8) == 16, "Galileo rounding");

    // :503-527
    EXPECT(quicksync_decide(2.0f, 1.0f, 1, 3, false) == 2, "positive at once");
    EXPECT(quicksync_decide(0.5f, 1.0f, 1, 3, false) == 1 && quicksync_decide(0.5f, 1.0f, 2, 3, false) == 1, "goes on below the threshold");
    EXPECT(quicksync_decide(0.5f, 1.0f, 3, 3, false) == 3, "negative at max_dwells");
    EXPECT(quicksync_decide(1.0f, 1.0f, 1, 1, false) == 3, "the threshold itself is not exceeded");
    EXPECT(quicksync_decide(2.0f, 1.0f, 1, 2, true) == 1, "bit transition: no decision at the first dwell");
    EXPECT(quicksync_decide(2.0f, 1.0f, 2, 2, true) == 2 && quicksync_decide(0.5f, 1.0f, 2, 2, true) == 3, "bit transition: decision at the second dwell");

    // adapters: no engine exists before init()
    {
        InMemoryConfiguration config;
        config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
        GpsL1CaPcpsQuickSyncAcquisitionHip acq(&config, "Acquisition_1C", 1, 0);
        EXPECT(acq.code_length() == 4000 && acq.folding_factor() == 4 && acq.sampled_ms() == 4 && acq.vector_length() == 16000 && acq.max_dwells() == 1,
            "GPS defaults: %u %u %u %u %u", acq.code_length(), acq.folding_factor(), acq.sampled_ms(), acq.vector_length(), acq.max_dwells());
        EXPECT(acq.block()->fft_size() == 1000 && acq.block()->item_length() == 16000, "GPS block: %u %u", acq.block()->fft_size(), acq.block()->item_length());
        EXPECT(acq.implementation() == "GPS_L1_CA_PCPS_QuickSync_Acquisition_HIP", "implementation name");
        config.set_property("Acquisition_1C.folding_factor", "2");
        config.set_property("Acquisition_1C.coherent_integration_time_ms", "5");
        config.set_property("Acquisition_1C.max_dwells", "3");
        GpsL1CaPcpsQuickSyncAcquisitionHip b(&config, "Acquisition_1C", 1, 0);
        EXPECT(b.folding_factor() == 2 && b.sampled_ms() == 4 && b.vector_length() == 16000 && b.max_dwells() == 3 && b.block()->fft_size() == 2000, "GPS keys");
        config.set_property("Acquisition_1C.bit_transition_flag", "true");
        GpsL1CaPcpsQuickSyncAcquisitionHip c(&config, "Acquisition_1C", 1, 0);
        EXPECT(c.max_dwells() == 2 && c.block()->max_dwells() == 2, "bit_transition_flag forces two dwells");
        // default GNSS-SDR.internal_fs_hz of the GPS adapter: 2048000 -> 2048 samples per code
        InMemoryConfiguration none;
        GpsL1CaPcpsQuickSyncAcquisitionHip d(&none, "Acquisition_1C", 1, 0);
        EXPECT(d.code_length() == 2048 && d.folding_factor() == 4, "GPS at the default rate: %u %u", d.code_length(), d.folding_factor());
        // Pfa rule
        config.set_property("Acquisition_1C.pfa", "0.001");
        b.set_doppler_max(5000);
        b.set_doppler_step(250);
        b.set_threshold(0.5f);
        const double val = std::pow(1.0 - static_cast<double>(0.001f), 1.0 / (2000.0 * 41.0));
        const float want = static_cast<float>(-std::log(1.0 - val) / 2000.0);
        EXPECT(std::abs(b.threshold() - want) <= 1e-5f * want, "Pfa threshold %g, expected %g", b.threshold(), want);
        InMemoryConfiguration plain;
        plain.set_property("GNSS-SDR.internal_fs_sps", "4000000");
        GpsL1CaPcpsQuickSyncAcquisitionHip e(&plain, "Acquisition_1C", 1, 0);
        e.set_threshold(0.5f);
        EXPECT(e.threshold() == 0.5f, "without pfa the given threshold is installed");
    }
    {
        InMemoryConfiguration config;
        GalileoE1PcpsQuickSyncAmbiguousAcquisitionHip acq(&config, "Acquisition_1B", 1, 0);
        EXPECT(acq.code_length() == 16000 && acq.folding_factor() == 2 && acq.sampled_ms() == 8 && acq.vector_length() == 32000, "Galileo defaults: %u %u %u %u",
            acq.code_length(), acq.folding_factor(), acq.sampled_ms(), acq.vector_length());
        EXPECT(acq.block()->fft_size() == 8000 && acq.block()->item_length() == 32000, "Galileo block");
        config.set_property("Acquisition_1B.coherent_integration_time_ms", "20");
        GalileoE1PcpsQuickSyncAmbiguousAcquisitionHip b(&config, "Acquisition_1B", 1, 0);
        EXPECT(b.sampled_ms() == 16 && b.vector_length() == 64000, "Galileo rounding to 4 f ms: %u", b.sampled_ms());
        EXPECT(b.implementation() == "Galileo_E1_PCPS_QuickSync_Ambiguous_Acquisition_HIP", "implementation name");
    }
    // the library's helpers and refusals that need no device
    uint32_t f = 0;
    EXPECT(gc_quicksync_default_folding_factor(4000, &f) == GC_OK && f == 4, "default folding factor of 4000");
    EXPECT(gc_quicksync_default_folding_factor(4000, nullptr) == GC_ERR_INVALID, "NULL out");
    gc_acq* h = nullptr;
    gc_acq_conf c;
    std::memset(&c, 0, sizeof c);
    EXPECT(gc_acq_create_quicksync(nullptr, &c, 1, 2, &h) == GC_ERR_INVALID && h == nullptr, "NULL context");
    EXPECT(gc_acq_quicksync_candidates(nullptr, 0, nullptr, nullptr) == GC_ERR_INVALID, "NULL handle");
}

// ---- GPU -------------------------------------------------------------------------------------------------------------------------

// stream_to_vector + scheduler: hands the block whole items until it has published an event (one more call publishes it)
template <class Adapter>
static void run_items(Adapter& acq, const std::vector<gr_complex>& x)
{
    auto blk = acq.block();
    const size_t item = acq.vector_length();
    size_t pos = 0;
    int guard = 0;
    while (blk->events().empty() && guard++ < 1000)
        {
            const int avail = static_cast<int>((x.size() - pos) / item);
            if (avail == 0 && blk->state() < 2) break;  // source exhausted in the middle of a search
            pos += static_cast<size_t>(blk->work(x.data() + pos, avail)) * item;
        }
}

template <class Adapter>
static void setup(Adapter& acq, Gnss_Synchro& g, char system, char sig1, uint32_t prn, float threshold, unsigned doppler_max, unsigned doppler_step)
{
    g.System = system;
    g.Signal[0] = '1';
    g.Signal[1] = sig1;
    g.PRN = prn;
    acq.set_channel(0);
    acq.set_gnss_synchro(&g);
    acq.set_threshold(threshold);
    acq.set_doppler_max(doppler_max);
    acq.set_doppler_step(doppler_step);
    acq.init();
    acq.set_local_code();
    acq.set_state(1);
}

// Thresholds.  statistic = max |.|^2 / M^4 / input_power.  A signal that fills the block gives f^4 times its share of the input power
// (the fold adds f^2 pieces coherently, the folded code f); both captures are strong: 16.1 (GPS, all of the power) and 1.2 (Galileo:
// E1-B is half of the power, and one data bit boundary falls into the 8 ms) in the numpy restatement.  Noise cells average f^3 / M:
// 0.004 (GPS, M = 2000) and 0.001 (Galileo, M = 8000), and the largest of n_bins * M of them about ln(n_bins M) = 11 to 13 times
// that.  A C/A code at the capture's strength adds its cross-correlation, at most -21.6 dB of 16, twice (two folded pieces): 0.22.
static const float kGpsThreshold = 1.0f, kGalileoThreshold = 0.2f;

static void test_gps(const std::vector<gr_complex>& x)
{
    // gates of kat_expected.json "gps_l1_ca"
    const double kDelay = 524.0, kDoppler = 1680.0, kMaxDelayErrorChips = 0.5, kMaxDopplerErrorHz = 666.0;
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1C.coherent_integration_time_ms", "2");
    config.set_property("Acquisition_1C.folding_factor", "2");
    config.set_property("Acquisition_1C.doppler_max", "5000");
    config.set_property("Acquisition_1C.max_dwells", "1");
    {
        Gnss_Synchro g;
        GpsL1CaPcpsQuickSyncAcquisitionHip acq(&config, "Acquisition_1C", 1, 0);
        EXPECT(acq.vector_length() == 8000, "vector length %u", acq.vector_length());
        setup(acq, g, 'G', 'C', 1, kGpsThreshold, 5000, 250);
        auto blk = acq.block();
        EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
        EXPECT(blk->fft_size() == 2000 && blk->num_doppler_bins() == 41, "sizes %u %u (both ends of the Doppler range count)", blk->fft_size(), blk->num_doppler_bins());
        run_items(acq, x);
        EXPECT(blk->events().size() == 1 && blk->events()[0] == 1, "GPS: expected ACQ SUCCESS (statistic %g)", blk->test_statistics());
        EXPECT(blk->dwell_count() == 1 && g.Acq_samplestamp_samples == 8000 && g.Acq_doppler_step == 250, "GPS: dwell %u, stamp %llu, step %u", blk->dwell_count(),
            static_cast<unsigned long long>(g.Acq_samplestamp_samples), g.Acq_doppler_step);
        EXPECT(std::abs(kDelay - g.Acq_delay_samples) * 1023 / 4000 < kMaxDelayErrorChips, "GPS: delay %g", g.Acq_delay_samples);
        EXPECT(std::abs(kDoppler - g.Acq_doppler_hz) <= kMaxDopplerErrorHz, "GPS: Doppler %g", g.Acq_doppler_hz);
        const gc_acq_result& r = blk->last_result();
        const float want = r.mag / (2000.0f * 2000.0f * 2000.0f * 2000.0f) / r.input_power;
        EXPECT(std::abs(blk->test_statistics() - want) <= 2e-4f * want, "GPS: statistic %g, mag / M^4 / input power %g", blk->test_statistics(), want);
        EXPECT(blk->possible_delay().size() == 2 && blk->possible_delay()[0] == r.indext && blk->possible_delay()[1] == r.indext + 2000, "GPS: candidate delays");
        EXPECT(blk->corr_output_f()[0] > 50.0f * blk->corr_output_f()[1], "GPS: candidates %g %g", blk->corr_output_f()[0], blk->corr_output_f()[1]);
        std::printf("GPS QuickSync acquisition: delay %g samples, Doppler %g Hz, statistic %g, candidates %g / %g\n", g.Acq_delay_samples, g.Acq_doppler_hz,
            blk->test_statistics(), blk->corr_output_f()[0], blk->corr_output_f()[1]);
    }
    // an absent PRN on 1 ms code periods with f = 1: the 2 ms hold two items, both dwells run, then ACQ_FAIL
    {
        InMemoryConfiguration c1;
        c1.set_property("GNSS-SDR.internal_fs_sps", "4000000");
        c1.set_property("Acquisition_1C.coherent_integration_time_ms", "1");
        c1.set_property("Acquisition_1C.folding_factor", "1");
        c1.set_property("Acquisition_1C.max_dwells", "2");
        Gnss_Synchro g;
        GpsL1CaPcpsQuickSyncAcquisitionHip absent(&c1, "Acquisition_1C", 1, 0);
        EXPECT(absent.vector_length() == 4000, "vector length %u", absent.vector_length());
        setup(absent, g, 'G', 'C', 19, kGpsThreshold / 16.0f, 5000, 250);  // f = 1: f^4 is 1
        run_items(absent, x);
        auto blk = absent.block();
        EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
        EXPECT(blk->events().size() == 1 && blk->events()[0] == 2, "absent PRN: expected ACQ FAIL (statistic %g)", blk->test_statistics());
        EXPECT(blk->dwell_count() == 2 && blk->test_statistics() > 0.0f && blk->sample_counter() == 8000, "absent PRN: %u dwells, statistic %g, %llu samples", blk->dwell_count(),
            blk->test_statistics(), static_cast<unsigned long long>(blk->sample_counter()));
        std::printf("GPS QuickSync, absent PRN 19: statistic %g after %u dwells\n", blk->test_statistics(), blk->dwell_count());
        // the present PRN with bit_transition_flag: above the threshold at the first dwell already, declared at the second only
        c1.set_property("Acquisition_1C.bit_transition_flag", "true");
        c1.set_property("Acquisition_1C.max_dwells", "5");
        Gnss_Synchro g2;
        GpsL1CaPcpsQuickSyncAcquisitionHip bt(&c1, "Acquisition_1C", 1, 0);
        setup(bt, g2, 'G', 'C', 1, kGpsThreshold / 16.0f, 5000, 250);
        auto blk2 = bt.block();
        EXPECT(blk2->work(x.data(), 2) == 1 && blk2->state() == 1 && blk2->test_statistics() > kGpsThreshold / 16.0f, "bit transition: first dwell decides nothing (state %d, statistic %g)",
            blk2->state(), blk2->test_statistics());
        EXPECT(blk2->work(x.data() + 4000, 1) == 1 && blk2->state() == 2 && blk2->dwell_count() == 2, "bit transition: positive at the second dwell (state %d)", blk2->state());
        (void)blk2->work(x.data(), 0);
        EXPECT(blk2->events().size() == 1 && blk2->events()[0] == 1, "bit transition: expected ACQ SUCCESS");
        EXPECT(g2.Acq_samplestamp_samples == 8000, "bit transition: stamp %llu", static_cast<unsigned long long>(g2.Acq_samplestamp_samples));
    }
}

static void test_galileo(const std::vector<gr_complex>& x)
{
    // gates of kat_expected.json "galileo_e1"
    const double kDelay = 2920.0, kDoppler = -632.0, kMaxDelayErrorChips = 0.175, kMaxDopplerErrorHz = 166.0;
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1B.doppler_max", "10000");
    Gnss_Synchro g;
    GalileoE1PcpsQuickSyncAmbiguousAcquisitionHip acq(&config, "Acquisition_1B", 1, 0);  // defaults: 8 ms, f = 2
    EXPECT(acq.vector_length() == 32000, "vector length %u", acq.vector_length());
    setup(acq, g, 'E', 'B', 1, kGalileoThreshold, 10000, 250);
    auto blk = acq.block();
    EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
    EXPECT(blk->fft_size() == 8000 && blk->num_doppler_bins() == 81, "sizes %u %u", blk->fft_size(), blk->num_doppler_bins());
    run_items(acq, x);
    EXPECT(blk->events().size() == 1 && blk->events()[0] == 1, "Galileo: expected ACQ SUCCESS (statistic %g)", blk->test_statistics());
    EXPECT(std::abs(kDelay - g.Acq_delay_samples) * 1023 / 4000 < kMaxDelayErrorChips, "Galileo: delay %g", g.Acq_delay_samples);
    EXPECT(std::abs(kDoppler - g.Acq_doppler_hz) <= kMaxDopplerErrorHz, "Galileo: Doppler %g", g.Acq_doppler_hz);
    std::printf("Galileo QuickSync acquisition: delay %g samples, Doppler %g Hz, statistic %g, candidates %g / %g\n", g.Acq_delay_samples, g.Acq_doppler_hz,
        blk->test_statistics(), blk->corr_output_f()[0], blk->corr_output_f()[1]);

    Gnss_Synchro g2;
    GalileoE1PcpsQuickSyncAmbiguousAcquisitionHip absent(&config, "Acquisition_1B", 1, 0);
    setup(absent, g2, 'E', 'B', 20, kGalileoThreshold, 10000, 250);
    run_items(absent, x);
    auto blk2 = absent.block();
    EXPECT(blk2->events().size() == 1 && blk2->events()[0] == 2 && blk2->dwell_count() == 1, "absent E20: expected ACQ FAIL after one dwell (statistic %g)", blk2->test_statistics());
    std::printf("Galileo QuickSync, absent PRN 20: statistic %g\n", blk2->test_statistics());
}

int main(int argc, char** argv)
{
    if (argc < 2)
        {
            std::printf("usage: %s --host | <golden dir>\n", argv[0]);
            return 2;
        }
    if (std::string(argv[1]) == "--host")
        {
            host_tests();
            if (g_fail == 0) std::printf("quicksync host self-test passed\n");
            return g_fail == 0 ? 0 : 1;
        }
    const auto gps = read_iq(std::string(argv[1]) + "/kat_gps_l1_ca_id1_fs4msps_2ms.dat");
    const auto gal = read_iq(std::string(argv[1]) + "/kat_galileo_e1_id1_fs4msps_8ms.dat");
    EXPECT(gps.size() == 8000 && gal.size() == 32000, "capture sizes %zu %zu", gps.size(), gal.size());
    if (g_fail) return 1;
    test_gps(gps);
    test_galileo(gal);
    if (g_fail == 0) std::printf("quicksync self-test passed\n");
    return g_fail == 0 ? 0 : 1;
}
