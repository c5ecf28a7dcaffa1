// tong_selftest -- the Tong adapters (hip_pcps_tong_acquisition.h: GpsL1CaPcpsTongAcquisitionHip and
// GalileoE1PcpsTongAmbiguousAcquisitionHip over hip_pcps_tong_acquisition).
//   tong_selftest --host               the pieces that need no GPU: inclusive bin count, the adapters' keys and defaults, the Galileo
//                                      rounding of coherent_integration_time_ms, the Pfa threshold rule, refusals of the library
//                                      that need no device.  Creates no GPU context.
//   tong_selftest <tests/golden dir>   on the GPS L1 C/A (4 Msps, 2 ms, PRN 1) and Galileo E1 (4 Msps, 8 ms, PRN 1) captures, two items
//                                      each: the present PRN is declared inside the gates of kat_expected.json, from host items and
//                                      from a ring (one call for all dwells), with the stamp at the end of the deciding block; an
//                                      absent PRN ends negative.  Needs a GPU (run by pytest -m gpu).
#include "hip_pcps_tong_acquisition.h"
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
    EXPECT(tong_doppler_bins(5000, 250) == 41 && tong_doppler_bins(5000, 500) == 21, "both ends count");
    EXPECT(tong_doppler_bins(1000, 300) == 7 && tong_doppler_bins(5000, 0) == 41, "1000 / 300: -1000 .. 800; a step of 0 means 250");
    {
        InMemoryConfiguration none;
        GpsL1CaPcpsTongAcquisitionHip d(&none, "Acquisition_1C", 1, 0);
        EXPECT(d.code_length() == 2048 && d.vector_length() == 2048 && d.sampled_ms() == 1, "GPS at the default rate: %u %u", d.code_length(), d.vector_length());
        EXPECT(d.tong_init_val() == 1 && d.tong_max_val() == 2 && d.tong_max_dwells() == 3, "Tong defaults %u %u %u", d.tong_init_val(), d.tong_max_val(), d.tong_max_dwells());
        EXPECT(d.implementation() == "GPS_L1_CA_PCPS_Tong_Acquisition_HIP", "implementation name");
        InMemoryConfiguration config;
        config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
        config.set_property("Acquisition_1C.coherent_integration_time_ms", "2");
        config.set_property("Acquisition_1C.tong_init_val", "2");
        config.set_property("Acquisition_1C.tong_max_val", "5");
        GpsL1CaPcpsTongAcquisitionHip b(&config, "Acquisition_1C", 1, 0);
        EXPECT(b.code_length() == 4000 && b.vector_length() == 8000 && b.block()->fft_size() == 8000 && b.block()->item_length() == 8000, "GPS keys: %u %u", b.code_length(),
            b.vector_length());
        EXPECT(b.tong_init_val() == 2 && b.tong_max_val() == 5 && b.tong_max_dwells() == 6, "tong_max_dwells defaults to tong_max_val + 1: %u", b.tong_max_dwells());
        config.set_property("Acquisition_1C.tong_max_dwells", "9");
        GpsL1CaPcpsTongAcquisitionHip c(&config, "Acquisition_1C", 1, 0);
        EXPECT(c.tong_max_dwells() == 9, "tong_max_dwells key");
        // Pfa rule: ncells = vector_length * bins, lambda = vector_length
        config.set_property("Acquisition_1C.pfa", "0.001");
        b.set_doppler_max(5000);
        b.set_doppler_step(250);
        b.set_threshold(0.5f);
        const double val = std::pow(1.0 - static_cast<double>(0.001f), 1.0 / (8000.0 * 41.0));
        const float want = static_cast<float>(-std::log(1.0 - val) / 8000.0);
        EXPECT(std::abs(b.threshold() - want) <= 1e-5f * want && b.block()->threshold() == b.threshold(), "Pfa threshold %g, expected %g", b.threshold(), want);
        InMemoryConfiguration plain;
        plain.set_property("GNSS-SDR.internal_fs_sps", "4000000");
        GpsL1CaPcpsTongAcquisitionHip e(&plain, "Acquisition_1C", 1, 0);
        e.set_threshold(0.5f);
        EXPECT(e.threshold() == 0.5f, "without pfa the given threshold is installed");
        // no engine before init(): a dwell fails the search instead of hanging the channel
        Gnss_Synchro g;
        e.set_gnss_synchro(&g);
        e.set_state(1);
        std::vector<gr_complex> item(4000);
        EXPECT(e.block()->work(item.data(), 1) == 1 && e.block()->state() == 3 && e.block()->last_status() == GC_ERR_STATE, "no engine: state %d", e.block()->state());
        EXPECT(e.block()->work(item.data(), 2) == 2 && e.block()->events().size() == 1 && e.block()->events()[0] == 2 && e.block()->sample_counter() == 12000, "ACQ_FAIL published");
    }
    {
        InMemoryConfiguration config;
        GalileoE1PcpsTongAmbiguousAcquisitionHip acq(&config, "Acquisition_1B", 1, 0);
        EXPECT(acq.code_length() == 16000 && acq.sampled_ms() == 4 && acq.vector_length() == 16000 && acq.block()->fft_size() == 16000, "Galileo defaults: %u %u %u", acq.code_length(),
            acq.sampled_ms(), acq.vector_length());
        config.set_property("Acquisition_1B.coherent_integration_time_ms", "10");
        GalileoE1PcpsTongAmbiguousAcquisitionHip b(&config, "Acquisition_1B", 1, 0);
        EXPECT(b.sampled_ms() == 8 && b.vector_length() == 32000 && b.block()->fft_size() == 32000, "Galileo rounding down to 4 ms: %u", b.sampled_ms());
        EXPECT(b.implementation() == "Galileo_E1_PCPS_Tong_Ambiguous_Acquisition_HIP", "implementation name");
    }
    float t = 0.0f;
    EXPECT(gc_tong_threshold(0.01f, 4000, 5000, 250, &t) == GC_OK && t > 0.0f, "threshold");
    EXPECT(gc_tong_threshold(0.01f, 4000, 5000, 250, nullptr) == GC_ERR_INVALID, "NULL out");
    gc_acq* h = nullptr;
    gc_acq_conf c;
    std::memset(&c, 0, sizeof c);
    EXPECT(gc_acq_create_tong(nullptr, &c, 1, 1, 2, 3, &h) == GC_ERR_INVALID && h == nullptr, "NULL context");
    EXPECT(gc_acq_tong_status(nullptr, nullptr) == GC_ERR_INVALID && gc_acq_tong_set_threshold(nullptr, 1.0f) == GC_ERR_INVALID, "NULL handle");
}

// ---- GPU -------------------------------------------------------------------------------------------------------------------------

// stream_to_vector + scheduler: hands the block whole host items until it has published an event (one more call publishes it)
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
    acq.set_doppler_max(doppler_max);
    acq.set_doppler_step(doppler_step);
    acq.set_threshold(threshold);
    acq.init();
    acq.set_local_code();
    acq.set_state(1);
}

// Thresholds, per dwell (the block multiplies by the dwell count).  A signal that fills the block adds its share of the input power
// per dwell; the numpy restatement gives 0.86 and 0.92 per dwell for G01, 0.18 and 0.17 for E01 (E1-B is half of the power), against
// 0.011 / 0.009 for the absent G19 (cross-correlation of a strong C/A code) and 0.0022 / 0.0017 for E20 (the largest of 1.3 million noise cells)
static const float kGpsThreshold = 0.1f, kGalileoThreshold = 0.02f;

static void test_gps(const std::vector<gr_complex>& x)
{
    // gates of kat_expected.json "gps_l1_ca"
    const double kDelay = 524.0, kDoppler = 1680.0, kMaxDelayErrorChips = 0.5, kMaxDopplerErrorHz = 666.0;
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    {
        // defaults (1, 2, 3): one hit declares
        Gnss_Synchro g;
        GpsL1CaPcpsTongAcquisitionHip acq(&config, "Acquisition_1C", 1, 0);
        setup(acq, g, 'G', 'C', 1, kGpsThreshold, 5000, 250);
        auto blk = acq.block();
        EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
        EXPECT(blk->fft_size() == 4000 && blk->num_doppler_bins() == 41, "sizes %u %u (both ends of the Doppler range count)", blk->fft_size(), blk->num_doppler_bins());
        run_items(acq, x);
        EXPECT(blk->events().size() == 1 && blk->events()[0] == 1, "GPS: expected ACQ SUCCESS (statistic %g)", blk->test_statistics());
        EXPECT(blk->dwell_count() == 1 && blk->tong_count() == 2 && g.Acq_samplestamp_samples == 4000 && g.Acq_doppler_step == 250, "GPS: dwell %u, count %u, stamp %llu",
            blk->dwell_count(), blk->tong_count(), static_cast<unsigned long long>(g.Acq_samplestamp_samples));
        EXPECT(std::abs(kDelay - g.Acq_delay_samples) * 1023 / 4000 < kMaxDelayErrorChips, "GPS: delay %g", g.Acq_delay_samples);
        EXPECT(std::abs(kDoppler - g.Acq_doppler_hz) <= kMaxDopplerErrorHz, "GPS: Doppler %g", g.Acq_doppler_hz);
        EXPECT(std::abs(blk->test_statistics() - 0.8584f) <= 2e-3f && blk->sample_counter() == 8000, "GPS: statistic %g, %llu samples", blk->test_statistics(),
            static_cast<unsigned long long>(blk->sample_counter()));
        std::printf("GPS Tong acquisition: delay %g samples, Doppler %g Hz, statistic %g after %u dwell(s)\n", g.Acq_delay_samples, g.Acq_doppler_hz, blk->test_statistics(),
            blk->dwell_count());
    }
    gc_ctx* ctx = gnsscorr::shared_context();
    gc_stream* ring = nullptr;
    EXPECT(ctx && gc_stream_create(ctx, GC_IQ_F32, 16000, 4000, &ring) == GC_OK, "ring: %s", gc_last_error());
    if (!ring) return;
    uint64_t first = 0;
    EXPECT(gc_stream_push(ring, x.data(), x.size(), &first) == GC_OK && first == 0, "push: %s", gc_last_error());
    {
        // (1, 3, 4) from the ring: both items in ONE call, two hits, positive at the second dwell, stamp at its end
        config.set_property("Acquisition_1C.tong_max_val", "3");
        Gnss_Synchro g;
        GpsL1CaPcpsTongAcquisitionHip acq(&config, "Acquisition_1C", 1, 0);
        setup(acq, g, 'G', 'C', 1, kGpsThreshold, 5000, 250);
        auto blk = acq.block();
        EXPECT(blk->work_ring(ring, 0, 2) == 2 && blk->state() == 2 && blk->dwell_count() == 2 && blk->tong_count() == 3, "ring: state %d, dwell %u, count %u (%s)", blk->state(),
            blk->dwell_count(), blk->tong_count(), gc_last_error());
        EXPECT(g.Acq_samplestamp_samples == 8000 && g.Acq_delay_samples == 524.0 && g.Acq_doppler_hz == 1750.0, "ring: stamp %llu, delay %g, Doppler %g",
            static_cast<unsigned long long>(g.Acq_samplestamp_samples), g.Acq_delay_samples, g.Acq_doppler_hz);
        EXPECT(std::abs(blk->test_statistics() - 1.8423f) <= 4e-3f, "ring: accumulated statistic %g", blk->test_statistics());
        EXPECT(blk->work_ring(ring, 8000, 0) == 0 && blk->events().size() == 1 && blk->events()[0] == 1 && blk->state() == 0, "ring: ACQ SUCCESS published");
        config.set_property("Acquisition_1C.tong_max_val", "2");
    }
    {
        // defaults from the ring, both items offered: the first dwell decides, the second moves nothing and is not consumed
        Gnss_Synchro g;
        GpsL1CaPcpsTongAcquisitionHip acq(&config, "Acquisition_1C", 1, 0);
        setup(acq, g, 'G', 'C', 1, kGpsThreshold, 5000, 250);
        auto blk = acq.block();
        EXPECT(blk->work_ring(ring, 0, 2) == 1 && blk->state() == 2 && blk->dwell_count() == 1 && g.Acq_samplestamp_samples == 4000, "ring, early decision: state %d, dwell %u, stamp %llu",
            blk->state(), blk->dwell_count(), static_cast<unsigned long long>(g.Acq_samplestamp_samples));
        EXPECT(std::abs(blk->test_statistics() - 0.8584f) <= 2e-3f, "ring, early decision: the deciding dwell's statistic stays (%g)", blk->test_statistics());
        // an absent PRN: one miss from init 1 is a negative
        Gnss_Synchro g2;
        GpsL1CaPcpsTongAcquisitionHip absent(&config, "Acquisition_1C", 1, 0);
        setup(absent, g2, 'G', 'C', 19, kGpsThreshold, 5000, 250);
        run_items(absent, x);
        auto b2 = absent.block();
        EXPECT(b2->events().size() == 1 && b2->events()[0] == 2 && b2->dwell_count() == 1 && b2->tong_count() == 0, "absent PRN: expected ACQ FAIL after one dwell (statistic %g)",
            b2->test_statistics());
        EXPECT(b2->test_statistics() > 0.0f && b2->test_statistics() < kGpsThreshold, "absent PRN: statistic %g", b2->test_statistics());
        std::printf("GPS Tong, absent PRN 19: statistic %g\n", b2->test_statistics());
        // set_active + state 0 restarts a search (the channel's reset()): the same result again
        (void)blk->work_ring(ring, 0, 0);  // state 2 -> event -> state 0, d_active cleared
        acq.reset();
        EXPECT(blk->work_ring(ring, 0, 0) == 0 && blk->state() == 1 && blk->dwell_count() == 0, "restart: state %d", blk->state());
        EXPECT(blk->work_ring(ring, 4000, 1) == 1 && blk->state() == 2 && blk->dwell_count() == 1, "restart: second search on the second item, state %d", blk->state());
    }
    gc_stream_destroy(ring);
}

static void test_galileo(const std::vector<gr_complex>& x)
{
    // gates of kat_expected.json "galileo_e1"
    const double kDelay = 2920.0, kDoppler = -632.0, kMaxDelayErrorChips = 0.175, kMaxDopplerErrorHz = 166.0;
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1B.doppler_max", "10000");
    Gnss_Synchro g;
    GalileoE1PcpsTongAmbiguousAcquisitionHip acq(&config, "Acquisition_1B", 1, 0);  // defaults: 4 ms, (1, 2, 3)
    EXPECT(acq.vector_length() == 16000, "vector length %u", acq.vector_length());
    setup(acq, g, 'E', 'B', 1, kGalileoThreshold, 10000, 250);
    auto blk = acq.block();
    EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
    EXPECT(blk->fft_size() == 16000 && blk->num_doppler_bins() == 81, "sizes %u %u", blk->fft_size(), blk->num_doppler_bins());
    run_items(acq, x);
    EXPECT(blk->events().size() == 1 && blk->events()[0] == 1 && blk->dwell_count() == 1, "Galileo: expected ACQ SUCCESS (statistic %g)", blk->test_statistics());
    EXPECT(std::abs(kDelay - g.Acq_delay_samples) * 1023 / 4000 < kMaxDelayErrorChips, "Galileo: delay %g", g.Acq_delay_samples);
    EXPECT(std::abs(kDoppler - g.Acq_doppler_hz) <= kMaxDopplerErrorHz, "Galileo: Doppler %g", g.Acq_doppler_hz);
    EXPECT(g.Acq_samplestamp_samples == 16000, "Galileo: stamp %llu", static_cast<unsigned long long>(g.Acq_samplestamp_samples));
    std::printf("Galileo Tong acquisition: delay %g samples, Doppler %g Hz, statistic %g\n", g.Acq_delay_samples, g.Acq_doppler_hz, blk->test_statistics());

    Gnss_Synchro g2;
    GalileoE1PcpsTongAmbiguousAcquisitionHip absent(&config, "Acquisition_1B", 1, 0);
    setup(absent, g2, 'E', 'B', 20, kGalileoThreshold, 10000, 250);
    run_items(absent, x);
    auto blk2 = absent.block();
    EXPECT(blk2->events().size() == 1 && blk2->events()[0] == 2 && blk2->dwell_count() == 1, "absent E20: expected ACQ FAIL after one dwell (statistic %g)", blk2->test_statistics());
    std::printf("Galileo Tong, absent PRN 20: statistic %g\n", blk2->test_statistics());
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
            if (g_fail == 0) std::printf("tong host self-test passed\n");
            return g_fail == 0 ? 0 : 1;
        }
    const auto gps = read_iq(std::string(argv[1]) + "/kat_gps_l1_ca_id1_fs4msps_2ms.dat");
    const auto gal = read_iq(std::string(argv[1]) + "/kat_galileo_e1_id1_fs4msps_8ms.dat");
    EXPECT(gps.size() == 8000 && gal.size() == 32000, "capture sizes %zu %zu", gps.size(), gal.size());
    if (g_fail) return 1;
    test_gps(gps);
    test_galileo(gal);
    if (g_fail == 0) std::printf("tong self-test passed\n");
    return g_fail == 0 ? 0 : 1;
}
