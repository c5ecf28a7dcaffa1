// caf_selftest -- the E5a CAF adapter (hip_e5a_noncoherent_iq_acquisition_caf.h: GalileoE5aNoncoherentIQAcquisitionCafHip over
// hip_e5a_noncoherent_iq_acquisition_caf).
//   caf_selftest --host   the pieces that need no GPU: the adapter's keys and defaults, the cap and the zero-padding rule of
//                         coherent_integration_time_ms, the 3 ms and the zero-padded replica layouts, the Pfa threshold rule, the
//                         refusals of the library that need no device, the failure path without an engine.  Creates no GPU context.
//   caf_selftest --gpu    on synthetic E5a signals at 2 Msps (PRN 11, both components, CN(0, 1) noise): a positive 3 ms search whose
//                         first code period is sign-flipped, with the CAF filter in both arithmetic modes; a zero-padded search; an
//                         absent PRN; a two-dwell bit-transition search from host items and from a ring.  Needs a GPU (pytest -m gpu).
#include "hip_e5a_noncoherent_iq_acquisition_caf.h"
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
    {
        InMemoryConfiguration none;
        GalileoE5aNoncoherentIQAcquisitionCafHip d(&none, "Acquisition_5X", 1, 0);
        EXPECT(d.code_length() == 32000 && d.vector_length() == 32000 && d.sampled_ms() == 1, "defaults at 32 Msps: %u %u %u", d.code_length(), d.vector_length(), d.sampled_ms());
        EXPECT(d.doppler_max() == 5000 && d.caf_window_hz() == 0 && d.zero_padding() == 0 && d.max_dwells() == 1 && !d.bit_transition_flag(), "defaults of the keys");
        EXPECT(d.both_components() && d.arithmetic() == GC_CAF_REFERENCE, "Channel.signal defaults to 5X, arithmetic to reference");
        EXPECT(d.block()->hypotheses() == 1 && d.block()->fft_size() == 32000 && d.block()->item_length() == 32000, "1 ms: one hypothesis");
        EXPECT(d.implementation() == "Galileo_E5a_Noncoherent_IQ_Acquisition_CAF_HIP" && d.item_size() == sizeof(gr_complex), "implementation name");
    }
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "10000000");
    config.set_property("Acquisition_5X.coherent_integration_time_ms", "5");
    config.set_property("Acquisition_5X.doppler_max", "10000");
    config.set_property("Acquisition_5X.CAF_window_hz", "3000");
    config.set_property("Acquisition_5X.max_dwells", "2");
    config.set_property("Acquisition_5X.bit_transition_flag", "true");
    config.set_property("Acquisition_5X.arithmetic", "exact");
    {
        GalileoE5aNoncoherentIQAcquisitionCafHip a(&config, "Acquisition_5X", 1, 0);
        EXPECT(a.sampled_ms() == 3 && a.code_length() == 10000 && a.vector_length() == 30000, "coherent time capped at 3 ms: %u %u %u", a.sampled_ms(), a.code_length(), a.vector_length());
        EXPECT(a.doppler_max() == 10000 && a.caf_window_hz() == 3000 && a.max_dwells() == 2 && a.bit_transition_flag() && a.arithmetic() == GC_CAF_EXACT, "keys");
        EXPECT(a.block()->hypotheses() == 2 && a.block()->fft_size() == 30000, "3 ms: two hypotheses");
        // the 3 ms replica layout (:245-259): three code periods of each component; 5I is (I, 0), 5Q is (0, Q)
        Gnss_Synchro g;
        g.System = 'E';
        g.Signal[0] = '5';
        g.Signal[1] = 'X';
        g.PRN = 11;
        a.set_gnss_synchro(&g);
        a.set_local_code();
        const auto& ci = a.block()->code_i();
        const auto& cq = a.block()->code_q();
        bool tiled = ci.size() == 30000 && cq.size() == 30000, unit = true;
        for (size_t i = 0; tiled && i < 10000; i++)
            {
                tiled = ci[i] == ci[i + 10000] && ci[i] == ci[i + 20000] && cq[i] == cq[i + 10000] && cq[i] == cq[i + 20000];
                unit = unit && std::abs(ci[i].real()) == 1.0f && ci[i].imag() == 0.0f && cq[i].real() == 0.0f && std::abs(cq[i].imag()) == 1.0f;
            }
        EXPECT(tiled && unit, "3 ms replicas: three periods of (I, 0) and of (0, Q)");
        // Pfa rule: ncells = vector_length * inclusive bins, lambda = vector_length
        config.set_property("Acquisition_5X.pfa", "0.001");
        a.set_doppler_max(10000);
        a.set_doppler_step(250);
        a.set_threshold(0.5f);
        const double val = std::pow(1.0 - static_cast<double>(0.001f), 1.0 / (30000.0 * 81.0));
        const float want = static_cast<float>(-std::log(1.0 - val) / 30000.0);
        EXPECT(std::abs(a.threshold() - want) <= 1e-5f * want && a.block()->threshold() == a.threshold(), "Pfa threshold %g, expected %g", a.threshold(), want);
    }
    {
        // Zero_padding forces 2 ms, one hypothesis, and the replica [code, zeros] (:260-270); a single component for 5I
        InMemoryConfiguration zp;
        zp.set_property("GNSS-SDR.internal_fs_sps", "10000000");
        zp.set_property("Acquisition_5X.coherent_integration_time_ms", "3");
        zp.set_property("Acquisition_5X.Zero_padding", "1");
        zp.set_property("Channel.signal", "5I");
        zp.set_property("Acquisition_5X.arithmetic", "fast");
        GalileoE5aNoncoherentIQAcquisitionCafHip a(&zp, "Acquisition_5X", 1, 0);
        EXPECT(a.sampled_ms() == 2 && a.vector_length() == 20000 && a.block()->fft_size() == 20000 && a.block()->hypotheses() == 1, "zero padding: %u ms, %u hypotheses", a.sampled_ms(),
            a.block()->hypotheses());
        EXPECT(!a.both_components() && a.arithmetic() == -1, "5I: one component; an unknown arithmetic is left to the engine to refuse");
        Gnss_Synchro g;
        g.System = 'E';
        g.Signal[0] = '5';
        g.Signal[1] = 'I';
        g.PRN = 11;
        a.set_gnss_synchro(&g);
        a.set_local_code();
        const auto& ci = a.block()->code_i();
        bool ok = ci.size() == 20000;
        for (size_t i = 0; ok && i < 10000; i++) ok = std::abs(ci[i].real()) == 1.0f && ci[i + 10000] == gr_complex(0.0f, 0.0f);
        EXPECT(ok, "zero-padded replica: one period, then zeros");
        a.set_threshold(0.25f);
        EXPECT(a.threshold() == 0.25f, "without pfa the given threshold is installed");
        // no engine before init(): a dwell fails the search instead of hanging the channel
        a.set_state(1);
        std::vector<gr_complex> item(20000);
        auto blk = a.block();
        EXPECT(blk->work(item.data(), 1) == 1 && blk->state() == 4 && blk->last_status() == GC_ERR_STATE, "no engine: state %d", blk->state());
        EXPECT(blk->work(item.data(), 2) == 2 && blk->events().size() == 1 && blk->events()[0] == 2 && blk->sample_counter() == 60000, "ACQ_FAIL published");
    }
    // refusals of the library that need no device
    gc_acq* h = nullptr;
    gc_acq_conf c;
    std::memset(&c, 0, sizeof c);
    c.fs_in = 10000000;
    c.sampled_ms = 3;
    c.samples_per_ms = 10000.0f;
    c.samples_per_code = 10000.0f;
    c.doppler_max = 5000;
    c.doppler_step = 250;
    c.max_dwells = 1;
    EXPECT(gc_acq_create_caf(nullptr, &c, 1, 1, 2, 0, GC_CAF_REFERENCE, &h) == GC_ERR_INVALID && h == nullptr && std::strstr(gc_last_error(), "NULL context"), "NULL context: %s",
        gc_last_error());
    EXPECT(gc_acq_create_caf(nullptr, &c, 1, 1, 3, 0, GC_CAF_REFERENCE, &h) == GC_ERR_INVALID && std::strstr(gc_last_error(), "hypotheses"), "hypotheses: %s", gc_last_error());
    EXPECT(gc_acq_create_caf(nullptr, &c, 1, 1, 2, 0, 7, &h) == GC_ERR_INVALID && std::strstr(gc_last_error(), "arithmetic"), "arithmetic: %s", gc_last_error());
    EXPECT(gc_acq_create_caf(nullptr, &c, 1, 1, 2, 499, GC_CAF_REFERENCE, &h) == GC_ERR_INVALID && std::strstr(gc_last_error(), "window"), "H == 0: %s", gc_last_error());
    EXPECT(gc_acq_set_local_code_iq(nullptr, 0, nullptr, nullptr) == GC_ERR_INVALID && gc_acq_caf_vectors(nullptr, 0, nullptr, nullptr, nullptr, nullptr) == GC_ERR_INVALID, "NULL handle");
}

// ---- GPU -------------------------------------------------------------------------------------------------------------------------

static const int kFs = 2000000, kL = 2000;  // one code period at 2 Msps

// amp * (s[p] * I + s[p] * Q) of `prn` (p the code period), delayed by `delay` samples, on a carrier of `doppler` Hz, in CN(0, 1)
static std::vector<gr_complex> synth(uint32_t prn, size_t n, float amp, const std::vector<int>& signs, int delay, double doppler, unsigned seed)
{
    std::vector<gr_complex> ci(kL + 8), cq(kL + 8), x(n);
    gc_galileo_e5_a_code_gen_complex_sampled(reinterpret_cast<float*>(ci.data()), "5I", prn, kFs, 0, nullptr);
    gc_galileo_e5_a_code_gen_complex_sampled(reinterpret_cast<float*>(cq.data()), "5Q", prn, kFs, 0, nullptr);
    std::mt19937 gen(seed);
    std::normal_distribution<float> gauss(0.0f, std::sqrt(0.5f));
    for (size_t i = 0; i < n; i++)
        {
            const size_t k = (i + n - static_cast<size_t>(delay)) % n;  // the delayed stream, circular over the whole signal
            const float s = static_cast<float>(signs[(k / kL) % signs.size()]);
            const double ph = 2.0 * M_PI * doppler * static_cast<double>(i) / kFs + 0.7;
            const gr_complex carrier(static_cast<float>(std::cos(ph)), static_cast<float>(std::sin(ph)));
            x[i] = amp * s * (ci[k % kL] + cq[k % kL]) * carrier + gr_complex(gauss(gen), gauss(gen));
        }
    return x;
}

static void setup(GalileoE5aNoncoherentIQAcquisitionCafHip& acq, Gnss_Synchro& g, uint32_t prn, float threshold, unsigned doppler_max, unsigned doppler_step)
{
    g.System = 'E';
    g.Signal[0] = '5';
    g.Signal[1] = 'X';
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

// the scheduler: hands the block whole host items until it has published an event (one more call publishes it)
static void run_items(GalileoE5aNoncoherentIQAcquisitionCafHip& acq, const std::vector<gr_complex>& x)
{
    auto blk = acq.block();
    const size_t item = acq.vector_length();
    size_t pos = 0;
    int guard = 0;
    while (blk->events().empty() && guard++ < 100)
        {
            const int avail = static_cast<int>((x.size() - pos) / item);
            if (avail == 0 && blk->state() < 3) break;  // source exhausted in the middle of a search
            pos += static_cast<size_t>(blk->work(x.data() + pos, avail)) * item;
        }
}

static void gpu_tests()
{
    const unsigned kDmax = 1000, kDstep = 250;  // nine bins
    for (const char* arithmetic : {"exact", "reference"})
        {
            // 3 ms, the first code period sign-flipped, CAF over one bin to either side, the threshold from the Pfa rule
            InMemoryConfiguration config;
            config.set_property("GNSS-SDR.internal_fs_sps", "2000000");
            config.set_property("Acquisition_5X.coherent_integration_time_ms", "3");
            config.set_property("Acquisition_5X.CAF_window_hz", "500");
            config.set_property("Acquisition_5X.pfa", "0.001");
            config.set_property("Acquisition_5X.arithmetic", arithmetic);
            Gnss_Synchro g;
            GalileoE5aNoncoherentIQAcquisitionCafHip acq(&config, "Acquisition_5X", 1, 0);
            setup(acq, g, 11, 0.0f, kDmax, kDstep);
            auto blk = acq.block();
            EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
            EXPECT(blk->fft_size() == 6000 && blk->num_doppler_bins() == 9 && blk->hypotheses() == 2, "sizes %u %u", blk->fft_size(), blk->num_doppler_bins());
            const auto x = synth(11, 2 * 6000, 0.25f, {-1, 1, 1}, 1234, 480.0, 1);
            run_items(acq, x);
            EXPECT(blk->events().size() == 1 && blk->events()[0] == 1 && blk->well_count() == 1, "%s: expected ACQ SUCCESS (statistic %g, threshold %g)", arithmetic, blk->test_statistics(),
                acq.threshold());
            EXPECT(g.Acq_delay_samples == 1234.0 && g.Acq_samplestamp_samples == 6000 && g.Acq_doppler_step == kDstep, "%s: delay %g, stamp %llu", arithmetic, g.Acq_delay_samples,
                static_cast<unsigned long long>(g.Acq_samplestamp_samples));
            EXPECT(blk->test_statistics() > 0.08f && blk->test_statistics() < 0.14f, "%s: statistic %g (2 amp^2 over the input power: 0.11)", arithmetic, blk->test_statistics());
            std::vector<float> caf(9), caf_i(9), caf_q(9);
            std::vector<uint8_t> choice(9);
            EXPECT(gc_acq_caf_vectors(blk->engine(), 0, caf.data(), caf_i.data(), caf_q.data(), choice.data()) == GC_OK, "vectors: %s", gc_last_error());
            EXPECT(choice[6] == 3, "%s: both components take hypothesis B at +500 Hz (%u)", arithmetic, choice[6]);
            if (std::string(arithmetic) == "exact")
                EXPECT(g.Acq_doppler_hz == 500.0 && blk->last_result().doppler_index == 6, "exact: Doppler %g", g.Acq_doppler_hz);
            else
                // the block as written: every bin but the last holds a wrapped weight of about -2^31, so its CAF argmax is the last bin
                EXPECT(g.Acq_doppler_hz == 1000.0 && caf[6] < 0.0f && caf[8] > 0.0f, "reference: Doppler %g, CAF %g %g", g.Acq_doppler_hz, caf[6], caf[8]);
            std::printf("E5a CAF acquisition (%s): delay %g samples, Doppler %g Hz, statistic %g, threshold %g\n", arithmetic, g.Acq_delay_samples, g.Acq_doppler_hz,
                blk->test_statistics(), acq.threshold());
        }
    {
        // zero padding: 1 ms of code + 1 ms of zeros against a 2 ms block, one hypothesis, no filter; and an absent PRN
        InMemoryConfiguration config;
        config.set_property("GNSS-SDR.internal_fs_sps", "2000000");
        config.set_property("Acquisition_5X.Zero_padding", "1");
        Gnss_Synchro g;
        GalileoE5aNoncoherentIQAcquisitionCafHip acq(&config, "Acquisition_5X", 1, 0);
        setup(acq, g, 11, 0.02f, kDmax, kDstep);
        auto blk = acq.block();
        EXPECT(blk->last_status() == GC_OK && blk->fft_size() == 4000 && blk->hypotheses() == 1, "zero padding: %s", gc_last_error());
        const auto x = synth(11, 2 * 4000, 0.4f, {1, -1}, 777, -260.0, 2);
        run_items(acq, x);
        EXPECT(blk->events().size() == 1 && blk->events()[0] == 1, "zero padding: expected ACQ SUCCESS (statistic %g)", blk->test_statistics());
        EXPECT(g.Acq_delay_samples == 777.0 && g.Acq_doppler_hz == -250.0, "zero padding: delay %g, Doppler %g", g.Acq_delay_samples, g.Acq_doppler_hz);
        std::printf("E5a CAF acquisition, zero padded: delay %g samples, Doppler %g Hz, statistic %g\n", g.Acq_delay_samples, g.Acq_doppler_hz, blk->test_statistics());
        Gnss_Synchro g2;
        GalileoE5aNoncoherentIQAcquisitionCafHip absent(&config, "Acquisition_5X", 1, 0);
        setup(absent, g2, 23, 0.02f, kDmax, kDstep);
        run_items(absent, x);
        auto b2 = absent.block();
        EXPECT(b2->events().size() == 1 && b2->events()[0] == 2 && b2->well_count() == 1, "absent PRN: expected ACQ FAIL (statistic %g)", b2->test_statistics());
        EXPECT(b2->test_statistics() > 0.0f && b2->test_statistics() < 0.02f, "absent PRN: statistic %g", b2->test_statistics());
        std::printf("E5a CAF acquisition, absent PRN 23: statistic %g\n", b2->test_statistics());
    }
    {
        // two dwells with bit_transition_flag: a strong block, then a weaker one with another delay: the first dwell's cell and stamp
        // are kept, the decision falls after the second; from host items and from a ring
        InMemoryConfiguration config;
        config.set_property("GNSS-SDR.internal_fs_sps", "2000000");
        config.set_property("Acquisition_5X.coherent_integration_time_ms", "2");
        config.set_property("Acquisition_5X.max_dwells", "2");
        config.set_property("Acquisition_5X.bit_transition_flag", "true");
        auto x = synth(11, 4000, 0.35f, {1, 1}, 300, 240.0, 3);
        const auto second = synth(11, 4000, 0.2f, {-1, 1}, 911, -510.0, 4);
        x.insert(x.end(), second.begin(), second.end());
        x.resize(3 * 4000, gr_complex(0.0f, 0.0f));
        gc_ctx* ctx = gnsscorr::shared_context();
        gc_stream* ring = nullptr;
        EXPECT(ctx && gc_stream_create(ctx, GC_IQ_F32, 16000, 4000, &ring) == GC_OK, "ring: %s", gc_last_error());
        uint64_t first = 0;
        if (ring) EXPECT(gc_stream_push(ring, x.data(), x.size(), &first) == GC_OK && first == 0, "push: %s", gc_last_error());
        float stat[2] = {0.0f, 0.0f};
        for (int from_ring = 0; from_ring < (ring ? 2 : 1); from_ring++)
            {
                Gnss_Synchro g;
                GalileoE5aNoncoherentIQAcquisitionCafHip acq(&config, "Acquisition_5X", 1, 0);
                setup(acq, g, 11, 0.02f, kDmax, kDstep);
                auto blk = acq.block();
                EXPECT(blk->last_status() == GC_OK, "engine: %s", gc_last_error());
                for (int d = 0; d < 2; d++)
                    {
                        const int used = from_ring ? blk->work_ring(ring, 4000ULL * d, 1) : blk->work(x.data() + 4000 * d, 1);
                        EXPECT(used == 1 && blk->state() == (d == 0 ? 1 : 3) && blk->well_count() == static_cast<uint32_t>(d + 1), "dwell %d: state %d (%s)", d, blk->state(), gc_last_error());
                        EXPECT(g.Acq_delay_samples == 300.0 && g.Acq_doppler_hz == 250.0 && g.Acq_samplestamp_samples == 4000, "dwell %d: delay %g, Doppler %g, stamp %llu", d,
                            g.Acq_delay_samples, g.Acq_doppler_hz, static_cast<unsigned long long>(g.Acq_samplestamp_samples));
                    }
                EXPECT(blk->last_result().mag > 0.0f && blk->last_result().mag * 2.0f < blk->test_statistics() * blk->last_result().input_power, "the second dwell is the weaker one");
                EXPECT(blk->work(x.data() + 8000, 1) == 1 && blk->events().size() == 1 && blk->events()[0] == 1 && blk->state() == 0 && blk->sample_counter() == 12000, "ACQ SUCCESS published");
                stat[from_ring] = blk->test_statistics();
            }
        if (ring) EXPECT(stat[0] == stat[1] && stat[0] > 0.1f, "host items and ring agree: %g %g", stat[0], stat[1]);
        std::printf("E5a CAF acquisition, two dwells with bit transition: kept statistic %g\n", stat[0]);
        if (ring) gc_stream_destroy(ring);
    }
}

int main(int argc, char** argv)
{
    if (argc < 2 || (std::string(argv[1]) != "--host" && std::string(argv[1]) != "--gpu"))
        {
            std::printf("usage: %s --host | --gpu\n", argv[0]);
            return 2;
        }
    if (std::string(argv[1]) == "--host")
        {
            host_tests();
            if (g_fail == 0) std::printf("caf host self-test passed\n");
            return g_fail == 0 ? 0 : 1;
        }
    gpu_tests();
    if (g_fail == 0) std::printf("caf self-test passed\n");
    return g_fail == 0 ? 0 : 1;
}
