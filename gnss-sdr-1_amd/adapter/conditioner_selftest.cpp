// conditioner_selftest -- hip_signal_conditioner in front of hip_acquisition_bank and hip_tracking_group: a cshort capture at 16 Msps
// with the GPS L1 C/A signals at a 1.25 MHz intermediate frequency goes through the conditioner (IF, decimation_factor 4, low-pass from
// bw / tw) in 40 ms blocks; the bank searches all 32 PRNs on the 4 Msps conditioned ring, its detections are handed to the group, and
// every satellite must be found and tracked at its true Doppler.  Usage: conditioner_selftest (needs a GPU).
#include "dll_pll_tracking_adapters.h"
#include "hip_acquisition_bank.h"
#include "hip_signal_conditioner.h"
#include "hip_tracking_group.h"
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

int main()
{
    if (gc_device_count() == 0)
        {
            std::printf("no GPU: libgnsscorr has no CPU fallback\n");
            return 3;
        }
    const double fs_in = 16e6, f_if = 1.25e6;
    const int D = 4;
    const int prns[3] = {5, 14, 23};
    const double dopplers[3] = {-3300.0, 450.0, 2750.0};
    const double delays_out[3] = {250.0, 2020.0, 3700.0};  // code delay in OUTPUT samples
    const size_t block = 16000 * 40, n_blocks = 10, n = block * n_blocks;  // 40 ms of raw samples per push, 400 ms
    const double scale = 64.0;                                             // noise sigma = 45 LSB of the cshort front end

    // x[i] = sum_k A c_k(tau_k + i * rate_k) exp(j 2 pi (f_if + fd_k) i / fs_in) + noise, quantised to cshort
    std::vector<double> re(n, 0.0), im(n, 0.0);
    for (int k = 0; k < 3; k++)
        {
            std::vector<float> code(1023);
            gc_gps_l1_ca_code_gen_float(code.data(), prns[k], 0);
            const double amp = std::sqrt(std::pow(10.0, 48.0 / 10.0) / fs_in);
            const double rate = 1.023e6 * (1.0 + dopplers[k] / 1575.42e6) / fs_in;
            const double tau0 = 1023.0 - delays_out[k] * D * 1.023e6 / fs_in;
            for (size_t i = 0; i < n; i++)
                {
                    const double ph = 2.0 * M_PI * std::fmod((f_if + dopplers[k]) / fs_in * static_cast<double>(i), 1.0) + 0.7;
                    const size_t chip = static_cast<size_t>(std::floor(tau0 + static_cast<double>(i) * rate)) % 1023;
                    re[i] += amp * code[chip] * std::cos(ph);
                    im[i] += amp * code[chip] * std::sin(ph);
                }
        }
    std::vector<int16_t> raw(2 * n);
    {
        std::mt19937 gen(77);
        std::normal_distribution<double> nd(0.0, std::sqrt(0.5));
        for (size_t i = 0; i < n; i++)
            {
                raw[2 * i] = static_cast<int16_t>(std::lrint((re[i] + nd(gen)) * scale));
                raw[2 * i + 1] = static_cast<int16_t>(std::lrint((im[i] + nd(gen)) * scale));
            }
    }
    re.clear();
    re.shrink_to_fit();
    im.clear();
    im.shrink_to_fit();

    InMemoryConfiguration config;
    config.set_property("InputFilter.IF", "1250000");
    config.set_property("InputFilter.sampling_frequency", "16000000");
    config.set_property("InputFilter.decimation_factor", "4");
    config.set_property("InputFilter.input_item_type", "cshort");
    config.set_property("InputFilter.filter_type", "lowpass");
    config.set_property("InputFilter.bw", "1600000");
    config.set_property("InputFilter.tw", "612000");
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Tracking_1C.pll_bw_hz", "50.0");
    GpsL1CaDllPllTrackingHip conf_source(&config, "Tracking_1C", 1, 1);

    gc_ctx* ctx = nullptr;
    EXPECT(gc_ctx_create(0, &ctx) == GC_OK, "context (%s)", gc_last_error());
    size_t n_items = 0;
    {
        hip_signal_conditioner cond(ctx, &config, "InputFilter", 4000 * 128, 8000);
        EXPECT(cond.last_status() == GC_OK && cond.ring() != nullptr, "conditioner: status %d (%s)", cond.last_status(), gc_last_error());
        EXPECT(cond.taps().size() == 63 && cond.fs_out() == 4e6 && cond.item_size() == 4 && cond.group_delay_samples() == 7.75,
            "conditioner: %zu taps, fs_out %.0f, item size %zu, group delay %.2f", cond.taps().size(), cond.fs_out(), cond.item_size(), cond.group_delay_samples());
        // a direct push into the conditioned ring is refused
        EXPECT(gc_stream_push(cond.ring(), raw.data(), 16, nullptr) == GC_ERR_STATE, "a direct push into the conditioned ring was accepted");
        // an unknown item type and a missing filter are reported at construction
        {
            InMemoryConfiguration bad;
            bad.set_property("F.input_item_type", "float");
            hip_signal_conditioner c1(ctx, &bad, "F", 8192, 1024);
            EXPECT(c1.last_status() == GC_ERR_INVALID && c1.push(raw.data(), 16) == GC_ERR_INVALID, "item type \"float\" was accepted");
            InMemoryConfiguration none;
            hip_signal_conditioner c2(ctx, &none, "F", 8192, 1024);  // filter_type is not "lowpass" and no taps were passed
            EXPECT(c2.last_status() == GC_ERR_INVALID, "a conditioner without taps was accepted");
        }
        std::vector<uint32_t> all;
        for (uint32_t p = 1; p <= 32; p++) all.push_back(p);
        // statistic = peak / N^4 / input power: noise cells average 1 / N, the largest of 32 x 100 x 4000 about 16 / N; 48 dB-Hz gives about 60 / N
        hip_acquisition_bank bank(ctx, cond.ring(), 'G', "1C", all, static_cast<int64_t>(cond.fs_out()), 5000, 100, 30.0f / 4000.0f);
        hip_tracking_group group(ctx, cond.ring(), conf_source.conf(), 8);
        EXPECT(bank.last_status() == GC_OK && bank.consumed_samples() == 4000 && group.last_status() == GC_OK, "bank / group: status %d / %d (%s)", bank.last_status(),
            group.last_status(), gc_last_error());
        std::vector<std::vector<Gnss_Synchro>> out;
        std::vector<Gnss_Synchro> detections;
        for (size_t b = 0; b < n_blocks; b++)
            {
                uint64_t first = 0, n_out = 0;
                EXPECT(cond.push(raw.data() + 2 * b * block, block, &first, &n_out) == GC_OK, "push (%s)", gc_last_error());
                EXPECT(first == b * block / D && n_out == block / D && cond.head() == (b + 1) * block / D, "block %zu: outputs [%llu, +%llu)", b,
                    static_cast<unsigned long long>(first), static_cast<unsigned long long>(n_out));
                if (b == 0)
                    {
                        detections = bank.search(0);
                        EXPECT(bank.last_status() == GC_OK, "bank: search status %d (%s)", bank.last_status(), gc_last_error());
                        for (size_t d = 0; d < detections.size() && d < 8; d++)
                            EXPECT(group.start_tracking(static_cast<int>(d), detections[d], detections[d].Acq_samplestamp_samples) == GC_OK, "group: hand-over (%s)",
                                gc_last_error());
                    }
                EXPECT(group.run(out) >= 0, "group: run status %d (%s)", group.last_status(), gc_last_error());
            }
        EXPECT(detections.size() == 3, "bank: %zu detections", detections.size());
        for (size_t d = 0; d < detections.size(); d++)
            {
                int k = -1;
                for (int j = 0; j < 3; j++)
                    if (detections[d].PRN == static_cast<uint32_t>(prns[j])) k = j;
                EXPECT(k >= 0, "bank: false detection of PRN %u", detections[d].PRN);
                if (k < 0 || d >= out.size()) continue;
                // the code delay the search reports includes the filter's group delay
                const double delay = std::fmod(delays_out[k] + cond.group_delay_samples(), 4000.0);
                EXPECT(std::fabs(detections[d].Acq_doppler_hz - dopplers[k]) <= 100.0 && std::fabs(detections[d].Acq_delay_samples - delay) <= 2.0,
                    "PRN %d: acquisition Doppler %.1f Hz (truth %.1f), delay %.1f samples (truth + group delay %.2f)", prns[k], detections[d].Acq_doppler_hz, dopplers[k],
                    detections[d].Acq_delay_samples, delay);
                const auto& items = out[d];
                n_items += items.size();
                EXPECT(items.size() >= 390 && group.active(static_cast<int>(d)), "PRN %d: %zu items", prns[k], items.size());
                if (items.size() < 50) continue;
                double mean = 0.0;
                for (size_t i = items.size() - 50; i < items.size(); i++) mean += items[i].Carrier_Doppler_hz;
                mean /= 50.0;
                EXPECT(std::fabs(mean - dopplers[k]) < 5.0, "PRN %d: mean Doppler %.2f Hz, truth %.2f", prns[k], mean, dopplers[k]);
                // sample stamps count output samples: one code period is 4000 of them, and none lies beyond the ring's head
                const uint64_t last = items.back().Tracking_sample_counter, before = items[items.size() - 2].Tracking_sample_counter;
                EXPECT(last - before >= 3999 && last - before <= 4001 && last <= cond.head(), "PRN %d: sample stamps %llu -> %llu, head %llu", prns[k],
                    static_cast<unsigned long long>(before), static_cast<unsigned long long>(last), static_cast<unsigned long long>(cond.head()));
                EXPECT(items.back().fs == 4000000, "PRN %d: items carry fs %lld", prns[k], static_cast<long long>(items.back().fs));
            }
    }
    gc_ctx_destroy(ctx);
    std::printf("signal conditioner: cshort at 16 Msps, IF 1.25 MHz -> 4 Msps ring; 3 satellites acquired by the bank and tracked by the group, %zu Gnss_Synchro\n", n_items);
    if (g_fail)
        {
            std::printf("signal conditioner self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("signal conditioner self-test passed\n");
    return 0;
}
