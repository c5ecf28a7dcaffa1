// notch_selftest -- hip_notch_filter behind a gr_complex ring at 4 Msps: GPS L1 C/A PRN 1 at C/N0 50 dB-Hz, code delay 1234 samples,
// Doppler 1500 Hz, unit noise, and a continuous-wave tone 30 dB above the noise from sample 16 L on.  A 4 x 1 ms non-coherent
// hip_pcps_acquisition search on the raw samples picks a wrong cell; on the notched ring's samples it finds the PRN at its delay
// and Doppler.  The adapters' keys are checked on the way: the lite adapter's segments_coeff from coeff_rate, the refused item
// types, dump accepted and ignored.
// Usage: notch_selftest (needs a GPU).
#include "hip_notch_filter.h"
#include "hip_pcps_acquisition.h"
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

// 4 x 1 ms non-coherent search of `y`; returns true when the four dwells ran and leaves the largest cell in `syn`
static bool search(const std::vector<gr_complex>& y, std::vector<gr_complex>& replica, Gnss_Synchro* syn)
{
    Acq_Conf conf;
    conf.sampled_ms = 1;
    conf.ms_per_code = 1;
    conf.samples_per_chip = 4;
    conf.max_dwells = 4;
    conf.doppler_max = 5000;
    conf.fs_in = 4000000;
    conf.resampled_fs = 4000000;
    conf.samples_per_ms = 4000.0f;
    conf.samples_per_code = 4000.0f;
    conf.use_CFAR_algorithm_flag = true;
    conf.blocking = true;
    conf.it_size = sizeof(gr_complex);
    syn->Channel_ID = 0;
    syn->System = 'G';
    syn->Signal[0] = '1';
    syn->Signal[1] = 'C';
    syn->PRN = 1;
    hip_pcps_acquisition blk(conf);
    blk.set_channel(1);
    blk.set_gnss_synchro(syn);
    blk.set_threshold(1e30f);  // the cell is what is checked: no dwell ends the search, the fourth leaves the accumulated grid's peak
    blk.set_doppler_max(5000);
    blk.set_doppler_step(250);
    blk.init();
    blk.set_local_code(replica.data());
    blk.set_state(1);
    size_t at = 0;
    int guard = 0;
    // the fourth dwell is searched by a call behind the one that filled its buffer: that call may come with no items left
    while (blk.events().empty() && guard++ < 100) at += static_cast<size_t>(blk.work(y.data() + at, static_cast<int>(std::min<size_t>(1000, y.size() - at))));
    return blk.last_status() == GC_OK && !blk.events().empty();
}

int main()
{
    if (gc_device_count() == 0)
        {
            std::printf("no GPU: libgnsscorr has no CPU fallback\n");
            return 3;
        }
    const double fs = 4e6, doppler = 1500.0, tone = 0.0837;
    const size_t n = 16000, L = 32, delay = 1234;
    std::vector<gr_complex> replica(4008);
    gc_gps_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(replica.data()), 1, 4000000, 0, nullptr);
    std::vector<gr_complex> raw(n);
    {
        std::mt19937 gen(2024);
        std::normal_distribution<double> nd(0.0, std::sqrt(0.5));
        const double amp = std::sqrt(std::pow(10.0, 5.0) / fs), jam = std::sqrt(1000.0);
        for (size_t i = 0; i < n; i++)
            {
                const double ph = 2.0 * M_PI * std::fmod(doppler / fs * static_cast<double>(i), 1.0) + 0.4;
                const double c = replica[(i + 4000 - delay) % 4000].real();
                double re = amp * c * std::cos(ph) + nd(gen), im = amp * c * std::sin(ph) + nd(gen);
                if (i >= 16 * L)
                    {
                        const double pj = 2.0 * M_PI * std::fmod(tone * static_cast<double>(i), 1.0) + 0.3;
                        re += jam * std::cos(pj);
                        im += jam * std::sin(pj);
                    }
                raw[i] = gr_complex(static_cast<float>(re), static_cast<float>(im));
            }
    }

    gc_ctx* ctx = gnsscorr::shared_context();
    EXPECT(ctx != nullptr, "context (%s)", gc_last_error());
    gc_stream* ring = nullptr;
    if (ctx) EXPECT(gc_stream_create(ctx, GC_IQ_F32, 1 << 15, 64, &ring) == GC_OK, "ring (%s)", gc_last_error());
    if (ctx && ring)
        {
            InMemoryConfiguration config;
            config.set_property("InputFilter.length", "32");
            config.set_property("InputFilter.segments_est", "10");
            config.set_property("InputFilter.noise_floor", "linear");
            config.set_property("InputFilter.threshold", "1000");
            config.set_property("InputFilter.dump", "true");
            hip_notch_filter notch(ctx, ring, &config, "InputFilter", 1 << 15, 4000);
            EXPECT(notch.last_status() == GC_OK, "notch filter: status %d (%s)", notch.last_status(), gc_last_error());
            EXPECT(notch.conf().mode == GC_NOTCH_FULL && notch.conf().pfa == 0.001f && notch.conf().p_c_factor == 0.9f && notch.conf().segments_reset == 5000000u,
                "defaults: mode %d, pfa %g, p_c_factor %g, segments_reset %u", notch.conf().mode, notch.conf().pfa, notch.conf().p_c_factor, notch.conf().segments_reset);

            // the lite adapter: segments_coeff = max(1, int((fs / coeff_rate) / float(length)))
            InMemoryConfiguration lite_config;
            lite_config.set_property("SignalSource.sampling_frequency", "4000000");
            lite_config.set_property("InputFilter.coeff_rate", "25000");
            lite_config.set_property("InputFilter.noise_floor", "linear");
            gc_stream* ring2 = nullptr;
            EXPECT(gc_stream_create(ctx, GC_IQ_F32, 1 << 12, 64, &ring2) == GC_OK, "second ring (%s)", gc_last_error());
            if (ring2)
                {
                    hip_notch_filter_lite lite(ctx, ring2, &lite_config, "InputFilter", 1 << 12, 64);
                    EXPECT(lite.last_status() == GC_OK && lite.conf().mode == GC_NOTCH_LITE && lite.conf().segments_coeff == 5u && lite.conf().length == 32u,
                        "lite adapter: status %d, segments_coeff %u (%s)", lite.last_status(), lite.conf().segments_coeff, gc_last_error());
                    InMemoryConfiguration dflt;
                    hip_notch_filter_lite lite_default(ctx, ring, &dflt, "InputFilter", 1 << 12, 64);  // coeff_rate = fs / 10: int(10 / 32) = 0 -> 1
                    EXPECT(lite_default.last_status() == GC_OK && lite_default.conf().segments_coeff == 1u, "lite adapter defaults: status %d, segments_coeff %u",
                        lite_default.last_status(), lite_default.conf().segments_coeff);
                    // an item type the reference only warns about
                    lite_config.set_property("InputFilter.item_type", "cshort");
                    hip_notch_filter_lite refused(ctx, ring2, &lite_config, "InputFilter", 1 << 12, 64);
                    EXPECT(refused.last_status() == GC_ERR_INVALID && refused.ring() == nullptr, "item_type=cshort: status %d", refused.last_status());
                    gc_stream_destroy(ring2);
                }

            // uneven pushes, an update after each
            const size_t pieces[5] = {6001, 37, 9000, 1, n - 15039};
            size_t pos = 0;
            for (size_t piece : pieces)
                {
                    EXPECT(gc_stream_push(ring, raw.data() + pos, piece, nullptr) == GC_OK, "push (%s)", gc_last_error());
                    pos += piece;
                    EXPECT(notch.update() == GC_OK, "update at %zu: status %d (%s)", pos, notch.last_status(), gc_last_error());
                }
            uint64_t decided = 0, filtered = 0;
            EXPECT(notch.segments(&decided, &filtered) == GC_OK && notch.head() == n, "head %llu (%s)", (unsigned long long)notch.head(), gc_last_error());
            EXPECT(decided == n / L && filtered == n / L - 16, "%llu segments decided, %llu filtered; expected %zu and %zu", (unsigned long long)decided,
                (unsigned long long)filtered, n / L, n / L - 16);
            std::vector<gr_complex> y(n);
            EXPECT(gc_stream_read(notch.ring(), 0, n, y.data()) == GC_OK, "read of the notched ring (%s)", gc_last_error());

            Gnss_Synchro on_raw, on_notched;
            EXPECT(search(raw, replica, &on_raw), "no result on the raw samples (%s)", gc_last_error());
            EXPECT(search(y, replica, &on_notched), "no result on the notched samples (%s)", gc_last_error());
            std::printf("raw samples: delay %.0f, Doppler %.0f Hz; notched ring: delay %.0f, Doppler %.0f Hz; truth %zu, %.0f Hz\n", on_raw.Acq_delay_samples,
                on_raw.Acq_doppler_hz, on_notched.Acq_delay_samples, on_notched.Acq_doppler_hz, delay, doppler);
            EXPECT(!(on_raw.Acq_delay_samples == static_cast<double>(delay) && on_raw.Acq_doppler_hz == doppler), "the tone does not mislead the search on the raw samples");
            EXPECT(on_notched.Acq_delay_samples == static_cast<double>(delay) && on_notched.Acq_doppler_hz == doppler, "notched ring: delay %.0f, Doppler %.0f Hz",
                on_notched.Acq_delay_samples, on_notched.Acq_doppler_hz);
        }
    if (ring) gc_stream_destroy(ring);
    if (g_fail)
        {
            std::printf("notch self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("notch self-test passed\n");
    return 0;
}
