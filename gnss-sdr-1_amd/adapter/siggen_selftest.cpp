// siggen_selftest -- hip_signal_generator, the image of the reference's Signal_Generator source, feeding acquisition on the same
// ring with no host link: configuration 1 of the reference's gps_l1_ca_pcps_acquisition_gsoc2013_test.cc (:203-228) -- one satellite,
// G PRN 10, 44 dB, 750 Hz, 600 chips, no noise, no data, BW_BB 0.97, 4 Msps -- searched by hip_acquisition_bank straight from the
// ring and by the hip_pcps_acquisition block on the ring's samples, under that test's own limits: delay error below 0.5 chip
// (without its 5-sample allowance for its GNU Radio chain), Doppler error below 2 / (3 x 1 ms) Hz.
// Usage: siggen_selftest (needs a GPU).
#include "hip_acquisition_bank.h"
#include "hip_pcps_acquisition.h"
#include "hip_signal_generator.h"
#include <cmath>
#include <cstdio>
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

static void configuration_1(InMemoryConfiguration& config)
{
    config.set_property("SignalSource.fs_hz", "4000000");
    config.set_property("SignalSource.item_type", "gr_complex");
    config.set_property("SignalSource.num_satellites", "1");
    config.set_property("SignalSource.system_0", "G");
    config.set_property("SignalSource.signal_0", "1C");
    config.set_property("SignalSource.PRN_0", "10");
    config.set_property("SignalSource.CN0_dB_0", "44");
    config.set_property("SignalSource.doppler_Hz_0", "750");
    config.set_property("SignalSource.delay_chips_0", "600");
    config.set_property("SignalSource.noise_flag", "false");
    config.set_property("SignalSource.data_flag", "false");
    config.set_property("SignalSource.BW_BB", "0.97");
}

int main()
{
    if (gc_device_count() == 0)
        {
            std::printf("no GPU: libgnsscorr has no CPU fallback\n");
            return 3;
        }
    const double expected_delay_chips = 600.0, expected_doppler_hz = 750.0;
    const double max_doppler_error_hz = 2.0 / (3.0 * 1e-3), max_delay_error_chips = 0.50;
    const int prn = 10;

    gc_ctx* ctx = gnsscorr::shared_context();
    EXPECT(ctx != nullptr, "context (%s)", gc_last_error());
    if (ctx)
        {
            InMemoryConfiguration config;
            configuration_1(config);
            hip_signal_generator source(ctx, &config, "SignalSource", 1 << 15, 4000);
            EXPECT(source.last_status() == GC_OK, "generator: status %d (%s)", source.last_status(), gc_last_error());
            EXPECT(source.vector_length() == 4000 && source.output_format() == GC_IQ_F32 && source.satellites().size() == 1, "vector_length %u, format %d",
                source.vector_length(), source.output_format());
            if (source.last_status() == GC_OK)
                {
                    const gc_siggen_sat& sat = source.satellites()[0];
                    EXPECT(sat.amplitude == 1.0 && sat.table_len == 1023 && sat.n_components == 1 && sat.doppler_hz == 750.0 && sat.comp[0].periods_per_symbol == 0,
                        "satellite: amplitude %g, table_len %u, Doppler %g", sat.amplitude, sat.table_len, sat.doppler_hz);
                    uint64_t first = 99;
                    EXPECT(source.work(3, &first) == GC_OK && first == 0 && source.work(5, &first) == GC_OK && first == 12000 && source.head() == 32000,
                        "work: status %d, first %llu, head %llu (%s)", source.last_status(), (unsigned long long)first, (unsigned long long)source.head(), gc_last_error());
                    // the host may not push into the generator's ring
                    float zero[2] = {0.0f, 0.0f};
                    EXPECT(gc_stream_push(source.ring(), zero, 1, nullptr) == GC_ERR_STATE, "a host push into the generator's ring was not refused");

                    // ---- the bank searches the ring itself ----
                    {
                        hip_acquisition_bank bank(ctx, source.ring(), 'G', "1C", std::vector<uint32_t>{static_cast<uint32_t>(prn)}, 4000000, 10000, 250, 0.005f);
                        EXPECT(bank.last_status() == GC_OK, "bank: status %d (%s)", bank.last_status(), gc_last_error());
                        const std::vector<Gnss_Synchro> found = bank.search(4000);
                        EXPECT(bank.last_status() == GC_OK && found.size() == 1, "bank: %zu detections, status %d (%s)", found.size(), bank.last_status(), gc_last_error());
                        if (found.size() == 1)
                            {
                                const double delay_error_chips = std::fabs(expected_delay_chips - found[0].Acq_delay_samples * 1023.0 / 4000.0);
                                const double doppler_error_hz = std::fabs(expected_doppler_hz - found[0].Acq_doppler_hz);
                                std::printf("bank on the generator's ring: PRN %u, delay %.1f samples (error %.3f chips), Doppler %.0f Hz (error %.0f Hz)\n", found[0].PRN,
                                    found[0].Acq_delay_samples, delay_error_chips, found[0].Acq_doppler_hz, doppler_error_hz);
                                EXPECT(found[0].PRN == static_cast<uint32_t>(prn), "PRN %u", found[0].PRN);
                                EXPECT(delay_error_chips < max_delay_error_chips, "delay error %.3f chips", delay_error_chips);
                                EXPECT(doppler_error_hz < max_doppler_error_hz, "Doppler error %.1f Hz", doppler_error_hz);
                            }
                    }

                    // ---- the block, as the reference's test drives it, on the ring's samples ----
                    std::vector<gr_complex> y(16000);
                    EXPECT(gc_stream_read(source.ring(), 0, y.size(), y.data()) == GC_OK, "read of the generator's ring (%s)", gc_last_error());
                    Acq_Conf conf;
                    conf.sampled_ms = 1;
                    conf.ms_per_code = 1;
                    conf.samples_per_chip = 4;
                    conf.max_dwells = 1;
                    conf.doppler_max = 10000;
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
                    blk.set_threshold(0.005f);
                    blk.set_doppler_max(10000);
                    blk.set_doppler_step(250);
                    blk.init();
                    blk.set_local_code(replica.data());
                    blk.set_state(1);
                    size_t at = 0;
                    int guard = 0;
                    while (blk.events().empty() && at < y.size() && guard++ < 100) at += static_cast<size_t>(blk.work(y.data() + at, static_cast<int>(std::min<size_t>(1024, y.size() - at))));
                    EXPECT(blk.last_status() == GC_OK && blk.events().size() == 1 && blk.events()[0] == 1, "no positive acquisition of PRN %d (%s)", prn, gc_last_error());
                    if (blk.events().size() == 1 && blk.events()[0] == 1)
                        {
                            const double delay_error_chips = std::fabs(expected_delay_chips - syn.Acq_delay_samples * 1023.0 / 4000.0);
                            const double doppler_error_hz = std::fabs(expected_doppler_hz - syn.Acq_doppler_hz);
                            std::printf("block on the ring's samples: delay %.1f samples (error %.3f chips), Doppler %.0f Hz (error %.0f Hz)\n", syn.Acq_delay_samples,
                                delay_error_chips, syn.Acq_doppler_hz, doppler_error_hz);
                            EXPECT(delay_error_chips < max_delay_error_chips, "delay error %.3f chips", delay_error_chips);
                            EXPECT(doppler_error_hz < max_doppler_error_hz, "Doppler error %.1f Hz", doppler_error_hz);
                        }
                }

            // a cshort ring: the same scene through the store epilogue, amplitude 1 at 1000 LSB
            {
                InMemoryConfiguration cs;
                configuration_1(cs);
                cs.set_property("SignalSource.output_item_type", "cshort");
                cs.set_property("SignalSource.output_scale", "1000");
                hip_signal_generator source16(ctx, &cs, "SignalSource", 1 << 14, 4000);
                EXPECT(source16.last_status() == GC_OK && source16.output_format() == GC_IQ_I16 && source16.output_scale() == 1000.0f, "cshort generator: status %d (%s)",
                    source16.last_status(), gc_last_error());
                EXPECT(source16.work(2) == GC_OK && source16.head() == 8000, "cshort work: status %d (%s)", source16.last_status(), gc_last_error());
                std::vector<int16_t> q(2 * 8000);
                EXPECT(gc_stream_read(source16.ring(), 0, 8000, q.data()) == GC_OK, "read of the cshort ring (%s)", gc_last_error());
                bool unit = true;
                for (size_t i = 0; i < 8000 && unit; i++)
                    {
                        const double m = std::hypot(static_cast<double>(q[2 * i]), static_cast<double>(q[2 * i + 1]));
                        unit = std::fabs(m - 1000.0) <= 1.0;  // each part rounds by at most half an LSB
                    }
                EXPECT(unit, "a cshort sample is not on the circle of radius 1000");
            }
            // keys the adapter does not know
            {
                InMemoryConfiguration bad;
                configuration_1(bad);
                bad.set_property("SignalSource.item_type", "cshort");
                hip_signal_generator g1(ctx, &bad, "SignalSource", 1 << 14, 4000);
                EXPECT(g1.last_status() == GC_ERR_INVALID && g1.ring() == nullptr, "item_type=cshort: status %d", g1.last_status());
                configuration_1(bad);
                bad.set_property("SignalSource.system_0", "C");
                hip_signal_generator g2(ctx, &bad, "SignalSource", 1 << 14, 4000);
                EXPECT(g2.last_status() == GC_ERR_INVALID && g2.ring() == nullptr, "system C: status %d", g2.last_status());
            }
        }
    if (g_fail)
        {
            std::printf("signal generator self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("signal generator self-test passed\n");
    return 0;
}
