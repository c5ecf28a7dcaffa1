// paired_acquisition_selftest -- the two-hypothesis Galileo E1 adapters (pcps_acquisition_adapters.h: CCCWSR and 8 ms, both over
// hip_pcps_paired_acquisition) and hip_acquisition_bank's CCCWSR option on the Galileo E1 capture of tests/golden (4 Msps, 8 ms,
// PRN 1; gates of GalileoE1PcpsAmbiguousAcquisitionTest.ValidationOfResults, galileo_e1_pcps_ambiguous_acquisition_test.cc:293-358):
//   - CCCWSR on 4 ms blocks and the 8 ms block on the one 8 ms block both declare PRN 1 inside the gates;
//   - an absent PRN ends negative after max_dwells dwells;
//   - CCCWSR on data + pilot gives a larger statistic than the one-replica adapter on E1-B for the same block;
//   - the bank with CCCWSR combining finds the PRN the one-replica bank finds.
// Usage: paired_acquisition_selftest <tests/golden directory>.  Needs a GPU (run by pytest -m gpu).
//        paired_acquisition_selftest --host: the bin count and what a Doppler step of 0 does in the block's init() and in the 8 ms
//        adapter's Pfa rule.  Creates no GPU context.
#include "hip_acquisition_bank.h"
#include "pcps_acquisition_adapters.h"
#include <cmath>
#include <cstdio>
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

// the gates of kat_expected.json "galileo_e1"
static const double kDelay = 2920.0, kDoppler = -632.0, kMaxDelayErrorChips = 0.175, kMaxDopplerErrorHz = 166.0;
// statistic = peak / N^4 / input power: noise cells average 1 / N and the largest of 81 x 16000 x 2 hypotheses stays below 20 / N =
// 1.3e-3; the capture's PRN 1 gives about 0.18 on 4 ms (kat_expected.json)
static const float kThreshold = 0.02f;

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
static void setup(Adapter& acq, Gnss_Synchro& g, uint32_t prn, unsigned doppler_step)
{
    g.System = 'E';
    g.Signal[0] = '1';
    g.Signal[1] = 'B';
    g.PRN = prn;
    acq.set_channel(0);
    acq.set_gnss_synchro(&g);
    acq.set_threshold(kThreshold);
    acq.set_doppler_max(10000);
    acq.set_doppler_step(doppler_step);
    acq.init();
    acq.set_local_code();
    acq.set_state(1);
}

static void expect_prn1(const char* what, const Gnss_Synchro& g)
{
    const double delay_error_chips = std::abs(kDelay - g.Acq_delay_samples) * 1023 / 4000;
    EXPECT(delay_error_chips < kMaxDelayErrorChips, "%s: delay %g", what, g.Acq_delay_samples);
    EXPECT(std::abs(kDoppler - g.Acq_doppler_hz) <= kMaxDopplerErrorHz, "%s: Doppler %g", what, g.Acq_doppler_hz);
}

static float test_cccwsr(const std::vector<gr_complex>& x)
{
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1B.coherent_integration_time_ms", "6");  // not a multiple of 4: 4 ms are used
    config.set_property("Acquisition_1B.doppler_max", "10000");
    config.set_property("Acquisition_1B.max_dwells", "2");
    Gnss_Synchro g;
    GalileoE1PcpsCccwsrAmbiguousAcquisitionHip acq(&config, "Acquisition_1B", 1, 0);
    EXPECT(acq.vector_length() == 16000, "vector length %u", acq.vector_length());
    setup(acq, g, 1, 250);
    auto blk = acq.block();
    EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
    EXPECT(blk->fft_size() == 16000 && blk->num_doppler_bins() == 81, "sizes %u %u (both ends of the Doppler range count)", blk->fft_size(), blk->num_doppler_bins());
    run_items(acq, x);
    EXPECT(blk->events().size() == 1 && blk->events()[0] == 1, "CCCWSR: expected ACQ SUCCESS");
    EXPECT(blk->dwell_count() == 1 && g.Acq_samplestamp_samples == 16000 && g.Acq_doppler_step == 250, "CCCWSR: dwell %u, stamp %llu, step %u", blk->dwell_count(),
        static_cast<unsigned long long>(g.Acq_samplestamp_samples), g.Acq_doppler_step);
    expect_prn1("CCCWSR", g);
    const float stat = blk->test_statistics();
    const gc_acq_result& r = blk->last_result();
    const float want = r.mag / (16000.0f * 16000.0f * 16000.0f * 16000.0f) / r.input_power;
    EXPECT(std::abs(stat - want) <= 2e-4f * want, "CCCWSR: statistic %g, mag / N^4 / input power %g", stat, want);
    std::printf("CCCWSR acquisition: delay %g samples, Doppler %g Hz, statistic %g\n", g.Acq_delay_samples, g.Acq_doppler_hz, stat);

    // an absent PRN: two dwells, then ACQ_FAIL; d_mag is the better of the two dwells (kept across the dwells of a search)
    Gnss_Synchro g2;
    GalileoE1PcpsCccwsrAmbiguousAcquisitionHip absent(&config, "Acquisition_1B", 1, 0);
    setup(absent, g2, 20, 250);
    run_items(absent, x);
    auto blk2 = absent.block();
    EXPECT(blk2->events().size() == 1 && blk2->events()[0] == 2, "absent PRN: expected ACQ FAIL");
    EXPECT(blk2->dwell_count() == 2 && blk2->test_statistics() < kThreshold && blk2->test_statistics() > 0.0f, "absent PRN: %u dwells, statistic %g", blk2->dwell_count(),
        blk2->test_statistics());
    std::printf("CCCWSR, absent PRN 20: statistic %g after %u dwells\n", blk2->test_statistics(), blk2->dwell_count());
    return stat;
}

static void test_8ms(const std::vector<gr_complex>& x)
{
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1B.coherent_integration_time_ms", "8");
    config.set_property("Acquisition_1B.doppler_max", "10000");
    Gnss_Synchro g;
    GalileoE1Pcps8msAmbiguousAcquisitionHip acq(&config, "Acquisition_1B", 1, 0);
    EXPECT(acq.vector_length() == 32000, "vector length %u", acq.vector_length());
    setup(acq, g, 1, 125);  // 8 ms coherent: bins 125 Hz apart
    auto blk = acq.block();
    EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
    EXPECT(blk->fft_size() == 32000 && blk->num_doppler_bins() == 161, "sizes %u %u", blk->fft_size(), blk->num_doppler_bins());
    run_items(acq, x);
    EXPECT(blk->events().size() == 1 && blk->events()[0] == 1, "8 ms: expected ACQ SUCCESS");
    expect_prn1("8 ms", g);
    std::printf("8 ms acquisition: delay %g samples, Doppler %g Hz, statistic %g\n", g.Acq_delay_samples, g.Acq_doppler_hz, blk->test_statistics());
    // the Pfa rule of the adapter: quantile of an exponential distribution of rate vector_length at (1 - pfa)^(1 / cells)
    config.set_property("Acquisition_1B.pfa", "0.001");
    acq.set_threshold(0.0f);
    const double val = std::pow(1.0 - 0.001, 1.0 / (32000.0 * 161.0));
    const float want = static_cast<float>(-std::log(1.0 - val) / 32000.0);
    EXPECT(std::abs(acq.threshold() - want) <= 1e-5f * want, "Pfa threshold %g, expected %g", acq.threshold(), want);
}

// the one-replica adapter on E1-B alone, first 4 ms block
static float plain_statistic(const std::vector<gr_complex>& x)
{
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1B.coherent_integration_time_ms", "4");
    config.set_property("Acquisition_1B.doppler_max", "10000");
    Gnss_Synchro g;
    GalileoE1PcpsAmbiguousAcquisitionHip acq(&config, "Acquisition_1B", 1, 0);
    setup(acq, g, 1, 250);
    auto blk = acq.block();
    size_t pos = 0;
    int guard = 0;
    while (blk->events().empty() && guard++ < 100000 && pos < x.size())
        pos += static_cast<size_t>(blk->work(x.data() + pos, static_cast<int>(std::min<size_t>(2048, x.size() - pos))));
    EXPECT(blk->events().size() == 1 && blk->events()[0] == 1, "one-replica adapter: expected ACQ SUCCESS");
    expect_prn1("one replica", g);
    return blk->test_statistics();
}

static void test_bank(const std::vector<gr_complex>& x)
{
    gc_ctx* ctx = nullptr;
    EXPECT(gc_ctx_create(0, &ctx) == GC_OK, "context (%s)", gc_last_error());
    gc_stream* ring = nullptr;
    EXPECT(gc_stream_create(ctx, GC_IQ_F32, 64000, 16000, &ring) == GC_OK, "ring (%s)", gc_last_error());
    if (ctx && ring)
        {
            EXPECT(gc_stream_push(ring, x.data(), x.size(), nullptr) == GC_OK, "push (%s)", gc_last_error());
            const std::vector<uint32_t> prns = {5, 1, 20};
            hip_acquisition_bank plain(ctx, ring, 'E', "1B", prns, 4000000, 10000, 250, kThreshold);
            hip_acquisition_bank both(ctx, ring, 'E', "1B", prns, 4000000, 10000, 250, kThreshold, 1, true, GC_IQ_F32, false, true);
            EXPECT(plain.last_status() == GC_OK && both.last_status() == GC_OK, "banks: status %d / %d (%s)", plain.last_status(), both.last_status(), gc_last_error());
            const auto f0 = plain.search(0);
            const auto f1 = both.search(0);
            EXPECT(f0.size() == 1 && f0[0].PRN == 1, "one-replica bank: %zu detections", f0.size());
            EXPECT(f1.size() == 1 && f1[0].PRN == 1, "CCCWSR bank: %zu detections", f1.size());
            if (f0.size() == 1 && f1.size() == 1)
                {
                    expect_prn1("CCCWSR bank", f1[0]);
                    EXPECT(f1[0].Acq_delay_samples == f0[0].Acq_delay_samples && f1[0].Acq_doppler_hz == f0[0].Acq_doppler_hz, "banks disagree: %g / %g samples, %g / %g Hz",
                        f0[0].Acq_delay_samples, f1[0].Acq_delay_samples, f0[0].Acq_doppler_hz, f1[0].Acq_doppler_hz);
                    EXPECT(both.statistic(1) > plain.statistic(1), "CCCWSR bank statistic %g, one-replica %g", both.statistic(1), plain.statistic(1));
                }
            std::printf("bank: PRN 1 statistic %g with CCCWSR combining, %g on E1-B alone\n", both.statistic(1), plain.statistic(1));
        }
    if (ring) gc_stream_destroy(ring);
    if (ctx) gc_ctx_destroy(ctx);
}

// the pieces that need no GPU: the bin count and what a Doppler step of 0 does.  Creates no GPU context
static void host_tests()
{
    EXPECT(gnsscorr::inclusive_doppler_bins(10000, 250) == 81 && gnsscorr::inclusive_doppler_bins(10000, 125) == 161, "both ends of the Doppler range count");
    // init() before set_doppler_step: no bins, no engine, GC_ERR_INVALID; the search fails through the "no engine" path after max_dwells items
    Gnss_Synchro g;
    hip_pcps_paired_acquisition blk(hip_pcps_paired_acquisition::CCCWSR, 4, 2, 10000, 4000000, 4000, 16000, false, "");
    blk.set_gnss_synchro(&g);
    blk.init();
    EXPECT(blk.last_status() == GC_ERR_INVALID && blk.num_doppler_bins() == 0, "step 0: status %d, %u bins", blk.last_status(), blk.num_doppler_bins());
    blk.set_state(1);
    std::vector<gr_complex> item(16000);
    EXPECT(blk.work(item.data(), 1) == 1 && blk.state() == 1 && blk.work(item.data(), 1) == 1 && blk.state() == 3 && blk.dwell_count() == 2, "step 0: state %d after %u dwells",
        blk.state(), blk.dwell_count());
    EXPECT(blk.work(item.data(), 1) == 1 && blk.events().size() == 1 && blk.events()[0] == 2 && blk.sample_counter() == 48000, "step 0: ACQ_FAIL published");
    // a Pfa before set_doppler_step: the 8 ms adapter leaves the given threshold installed; with a step it applies its rule
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Acquisition_1B.coherent_integration_time_ms", "8");
    config.set_property("Acquisition_1B.pfa", "0.001");
    GalileoE1Pcps8msAmbiguousAcquisitionHip acq(&config, "Acquisition_1B", 1, 0);
    acq.set_doppler_max(10000);
    acq.set_threshold(0.25f);
    EXPECT(acq.threshold() == 0.25f && acq.block()->threshold() == 0.25f, "Pfa with a step of 0: threshold %g", acq.threshold());
    acq.set_doppler_step(125);
    acq.set_threshold(0.25f);
    const double val = std::pow(1.0 - 0.001, 1.0 / (32000.0 * 161.0));
    const float want = static_cast<float>(-std::log(1.0 - val) / 32000.0);
    EXPECT(std::abs(acq.threshold() - want) <= 1e-5f * want, "Pfa threshold %g, expected %g", acq.threshold(), want);
    // the CCCWSR adapter installs what it is given, Pfa or not
    GalileoE1PcpsCccwsrAmbiguousAcquisitionHip cccwsr(&config, "Acquisition_1B", 1, 0);
    cccwsr.set_doppler_step(250);
    cccwsr.set_threshold(0.25f);
    EXPECT(cccwsr.threshold() == 0.25f, "CCCWSR threshold %g", cccwsr.threshold());
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
            if (g_fail == 0) std::printf("paired acquisition host self-test passed\n");
            return g_fail == 0 ? 0 : 1;
        }
    const auto x = read_iq(std::string(argv[1]) + "/kat_galileo_e1_id1_fs4msps_8ms.dat");
    EXPECT(x.size() == 32000, "capture size %zu", x.size());
    if (x.size() != 32000) return 1;
    const float both = test_cccwsr(x);
    const float one = plain_statistic(x);
    EXPECT(both > one, "CCCWSR statistic %g is not above the one-replica statistic %g of the same block", both, one);
    std::printf("first 4 ms block: statistic %g on data + pilot, %g on E1-B alone\n", both, one);
    test_8ms(x);
    test_bank(x);
    if (g_fail == 0) std::printf("paired acquisition self-test passed\n");
    return g_fail == 0 ? 0 : 1;
}
