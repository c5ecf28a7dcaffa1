// resampler_selftest -- hip_direct_resampler behind a cshort ring at 6.625 Msps with one GPS L1 C/A satellite: in polyphase mode it
// derives a gr_complex ring at 4 Msps on the device, and hip_pcps_acquisition at N = 4000 on the derived ring's samples must find
// the PRN at its Doppler, with the code start where the signal puts it plus the filter's group delay; in direct mode (the
// reference's Direct_Resampler) the derived cshort ring must hold exactly the source samples n_m = ceil(m 2^32 / step).
// Usage: resampler_selftest (needs a GPU).
#include "hip_direct_resampler.h"
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

// distance of a and b modulo `period`
static double mod_distance(double a, double b, double period)
{
    double d = std::fmod(a - b, period);
    if (d < 0.0) d += period;
    return std::min(d, period - d);
}

int main()
{
    if (gc_device_count() == 0)
        {
            std::printf("no GPU: libgnsscorr has no CPU fallback\n");
            return 3;
        }
    const double fs_in = 6.625e6, fs_out = 4e6;
    const int prn = 17;
    const double doppler = -2250.0;
    const double start = 1234.25;  // source sample at which a code period starts
    const size_t n = 6625 * 4;     // 4 ms
    const double scale = 64.0;     // noise sigma = 45 LSB of the cshort front end
    const double cn0_db_hz = 50.0;

    std::vector<float> code(1023);
    gc_gps_l1_ca_code_gen_float(code.data(), prn, 0);
    std::vector<int16_t> raw(2 * n);
    {
        std::mt19937 gen(17);
        std::normal_distribution<double> nd(0.0, std::sqrt(0.5));
        const double amp = std::sqrt(std::pow(10.0, cn0_db_hz / 10.0) / fs_in);
        const double rate = 1.023e6 * (1.0 + doppler / 1575.42e6) / fs_in;
        for (size_t i = 0; i < n; i++)
            {
                const double ph = 2.0 * M_PI * std::fmod(doppler / fs_in * static_cast<double>(i), 1.0) + 0.7;
                const double chip_pos = (static_cast<double>(i) - start) * rate;
                const size_t chip = static_cast<size_t>(std::floor(chip_pos - 1023.0 * std::floor(chip_pos / 1023.0))) % 1023;
                raw[2 * i] = static_cast<int16_t>(std::lrint((amp * code[chip] * std::cos(ph) + nd(gen)) * scale));
                raw[2 * i + 1] = static_cast<int16_t>(std::lrint((amp * code[chip] * std::sin(ph) + nd(gen)) * scale));
            }
    }

    gc_ctx* ctx = gnsscorr::shared_context();
    EXPECT(ctx != nullptr, "context (%s)", gc_last_error());
    gc_stream* ring = nullptr;
    if (ctx) EXPECT(gc_stream_create(ctx, GC_IQ_I16, 1 << 15, 64, &ring) == GC_OK, "ring (%s)", gc_last_error());
    if (ctx && ring)
        {
            InMemoryConfiguration config;
            config.set_property("Resampler.sample_freq_in", "6625000");
            config.set_property("Resampler.sample_freq_out", "4000000");
            config.set_property("Resampler.item_type", "cshort");
            config.set_property("Resampler.resampler_mode", "polyphase");
            config.set_property("Resampler.phases", "64");
            hip_direct_resampler poly(ctx, ring, &config, "Resampler", 1 << 15, 4000);
            InMemoryConfiguration config_direct;
            config_direct.set_property("Resampler.sample_freq_in", "6625000");
            config_direct.set_property("Resampler.sample_freq_out", "4000000");
            config_direct.set_property("Resampler.item_type", "cshort");
            hip_direct_resampler direct(ctx, ring, &config_direct, "Resampler", 1 << 15, 4000);
            EXPECT(poly.last_status() == GC_OK && direct.last_status() == GC_OK, "resamplers: status %d / %d (%s)", poly.last_status(), direct.last_status(),
                gc_last_error());
            EXPECT(poly.polyphase() && poly.output_format() == GC_IQ_F32 && !direct.polyphase() && direct.output_format() == GC_IQ_I16,
                "formats: polyphase %d, direct %d", poly.output_format(), direct.output_format());
            // a key the block does not know
            config_direct.set_property("Resampler.resampler_mode", "cubic");
            hip_direct_resampler unknown(ctx, ring, &config_direct, "Resampler", 1 << 15, 4000);
            EXPECT(unknown.last_status() == GC_ERR_INVALID && unknown.ring() == nullptr, "resampler_mode=cubic: status %d", unknown.last_status());

            // uneven pushes, an update of both after each
            const size_t pieces[5] = {6001, 37, 9000, 1, n - 15039};
            size_t pos = 0;
            for (size_t piece : pieces)
                {
                    EXPECT(gc_stream_push(ring, raw.data() + 2 * pos, piece, nullptr) == GC_OK, "push (%s)", gc_last_error());
                    pos += piece;
                    EXPECT(poly.update() == GC_OK && direct.update() == GC_OK, "update at %zu: status %d / %d (%s)", pos, poly.last_status(), direct.last_status(),
                        gc_last_error());
                }
            // heads: ceil(H 2^32 / INC) with INC = 53 / 32 * 2^32 exactly, and floor((H - 1) step / 2^32) + 1
            const uint64_t inc = 53ull << 27, step = static_cast<uint32_t>(std::floor(4294967296.0 * fs_out / fs_in));
            const uint64_t want_poly = ((static_cast<uint64_t>(n) << 32) + inc - 1) / inc, want_direct = (((n - 1) * step) >> 32) + 1;
            EXPECT(poly.head() == want_poly && direct.head() == want_direct, "heads %llu / %llu, expected %llu / %llu", (unsigned long long)poly.head(),
                (unsigned long long)direct.head(), (unsigned long long)want_poly, (unsigned long long)want_direct);

            // direct mode: the picks
            std::vector<int16_t> got(2 * direct.head());
            EXPECT(gc_stream_read(direct.ring(), 0, direct.head(), got.data()) == GC_OK, "read of the direct ring (%s)", gc_last_error());
            size_t wrong = 0;
            for (uint64_t m = 0; m < direct.head(); m++)
                {
                    const uint64_t nm = ((m << 32) + step - 1) / step;
                    if (nm >= n || got[2 * m] != raw[2 * nm] || got[2 * m + 1] != raw[2 * nm + 1]) wrong++;
                }
            EXPECT(wrong == 0, "direct mode: %zu of %llu outputs are not source sample ceil(m 2^32 / step)", wrong, (unsigned long long)direct.head());

            // polyphase mode: the block searches the derived samples
            std::vector<gr_complex> y(poly.head());
            EXPECT(gc_stream_read(poly.ring(), 0, poly.head(), y.data()) == GC_OK, "read of the derived ring (%s)", gc_last_error());
            Acq_Conf conf;
            conf.sampled_ms = 1;
            conf.ms_per_code = 1;
            conf.samples_per_chip = 4;
            conf.max_dwells = 1;
            conf.doppler_max = 5000;
            conf.fs_in = 4000000;
            conf.resampled_fs = 4000000;
            conf.samples_per_ms = 4000.0f;
            conf.samples_per_code = 4000.0f;
            conf.use_CFAR_algorithm_flag = true;
            conf.blocking = true;
            conf.it_size = sizeof(gr_complex);
            std::vector<gr_complex> replica(4008);
            gc_gps_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(replica.data()), prn, 4000000, 0, nullptr);
            Gnss_Synchro syn;
            syn.Channel_ID = 0;
            syn.System = 'G';
            syn.Signal[0] = '1';
            syn.Signal[1] = 'C';
            syn.PRN = prn;
            hip_pcps_acquisition blk(conf);
            blk.set_channel(1);
            blk.set_gnss_synchro(&syn);
            blk.set_threshold(0.005f);  // noise cells average 1 / N = 0.00025, the largest of 40 x 4000 about 12 / N = 0.003
            blk.set_doppler_max(5000);
            blk.set_doppler_step(250);
            blk.init();
            blk.set_local_code(replica.data());
            blk.set_state(1);
            size_t at = 2000;  // behind the filter's start-up
            int guard = 0;
            while (blk.events().empty() && at < y.size() && guard++ < 100) at += static_cast<size_t>(blk.work(y.data() + at, static_cast<int>(std::min<size_t>(1024, y.size() - at))));
            EXPECT(blk.last_status() == GC_OK && blk.events().size() == 1 && blk.events()[0] == 1, "no positive acquisition of PRN %d on the derived ring (%s)", prn,
                gc_last_error());
            // a code period starts at derived sample (start + group delay) * fs_out / fs_in; the block counted from derived sample 2000
            const double true_start = (start + poly.group_delay_samples()) * fs_out / fs_in;
            const double found_start = 2000.0 + static_cast<double>(syn.Acq_samplestamp_samples) + syn.Acq_delay_samples;
            std::printf("PRN %d on the derived 4 Msps ring: code start at derived sample %.2f (mod 4000), truth %.2f; Doppler %.0f Hz, truth %.0f Hz; group delay %.3f source samples\n",
                prn, std::fmod(found_start, 4000.0), std::fmod(true_start, 4000.0), syn.Acq_doppler_hz, doppler, poly.group_delay_samples());
            EXPECT(std::fabs(syn.Acq_doppler_hz - doppler) <= 250.0, "Doppler %.1f Hz, truth %.1f", syn.Acq_doppler_hz, doppler);
            // one sample for the grid, one for the replica's sampling convention (chip ceil((i + 1) rate) - 1)
            EXPECT(mod_distance(found_start, true_start, 4000.0) <= 2.0, "code start at derived sample %.2f (mod 4000), truth %.2f", std::fmod(found_start, 4000.0),
                std::fmod(true_start, 4000.0));
        }
    if (ring) gc_stream_destroy(ring);
    if (g_fail)
        {
            std::printf("resampler self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("resampler self-test passed\n");
    return 0;
}
