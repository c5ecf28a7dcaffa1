// blanking_selftest -- hip_signal_conditioner with the reference Pulse_Blanking_Filter's keys (pulse_blanking, pfa, length,
// segments_est, segments_reset): a cshort stream of noise with strong pulses on known segments is pushed in blocks that are no
// multiple of the segment length; the ring's head must advance by whole segments, the pulse segments must read back as zeros through
// gc_stream_read and every segment that was not blanked must be the converted input.  Usage: blanking_selftest (needs a GPU).
#include "hip_signal_conditioner.h"
#include <algorithm>
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
    const uint32_t L = 32, est = 20;
    const size_t n_seg = 400, n = n_seg * L + 11, block = 1000;
    const double scale = 64.0;  // noise sigma = 45 LSB per component
    std::vector<int16_t> raw(2 * n);
    std::vector<char> pulsed(n_seg, 0);
    {
        std::mt19937 gen(123);
        std::normal_distribution<double> nd(0.0, std::sqrt(0.5));
        for (size_t i = 0; i < n; i++)
            {
                const size_t s = i / L;
                const bool pulse = s >= est + 10 && s < n_seg && s % 10 == 5;  // the whole segment, amplitude 20
                if (pulse) pulsed[s] = 1;
                const double ph = 0.3 * static_cast<double>(i);
                raw[2 * i] = static_cast<int16_t>(std::lrint((nd(gen) + (pulse ? 20.0 * std::cos(ph) : 0.0)) * scale));
                raw[2 * i + 1] = static_cast<int16_t>(std::lrint((nd(gen) + (pulse ? 20.0 * std::sin(ph) : 0.0)) * scale));
            }
    }

    InMemoryConfiguration config;
    config.set_property("InputFilter.input_item_type", "cshort");
    config.set_property("InputFilter.sampling_frequency", "4000000");
    config.set_property("InputFilter.pulse_blanking", "true");
    config.set_property("InputFilter.pfa", "0.001");
    config.set_property("InputFilter.length", "32");
    config.set_property("InputFilter.segments_est", "20");
    config.set_property("InputFilter.segments_reset", "1000000");  // no re-estimate: a segment used for one is passed, pulse or not

    gc_ctx* ctx = nullptr;
    EXPECT(gc_ctx_create(0, &ctx) == GC_OK, "context (%s)", gc_last_error());
    size_t n_pulsed = 0;
    {
        // IF = 0, D = 1, one unit tap: the ring holds the blanked raw samples as gr_complex
        hip_signal_conditioner cond(ctx, &config, "InputFilter", 1 << 15, 4096, std::vector<float>(1, 1.0f));
        EXPECT(cond.last_status() == GC_OK && cond.ring() != nullptr && cond.pulse_blanking(), "conditioner: status %d (%s)", cond.last_status(), gc_last_error());
        EXPECT(cond.blanked_segments() == 0 && cond.noise_power() == 0.0f, "counters before the first push");
        size_t pushed = 0;
        while (pushed < n)
            {
                const size_t m = std::min(block, n - pushed);
                uint64_t first = 0, n_out = 0;
                EXPECT(cond.push(raw.data() + 2 * pushed, m, &first, &n_out) == GC_OK, "push (%s)", gc_last_error());
                const uint64_t before = pushed / L * L;
                pushed += m;
                const uint64_t after = pushed / L * L;
                EXPECT(first == before && n_out == after - before && cond.head() == after, "after %zu items: outputs [%llu, +%llu), head %llu, expected [%llu, %llu)", pushed,
                    static_cast<unsigned long long>(first), static_cast<unsigned long long>(n_out), static_cast<unsigned long long>(cond.head()),
                    static_cast<unsigned long long>(before), static_cast<unsigned long long>(after));
            }
        std::vector<float> y(2 * n_seg * L);
        EXPECT(gc_stream_read(cond.ring(), 0, n_seg * L, y.data()) == GC_OK, "read (%s)", gc_last_error());
        size_t n_zero = 0, n_wrong = 0, n_missed = 0;
        for (size_t s = 0; s < n_seg; s++)
            {
                bool zero = true, same = true;
                for (size_t i = 2 * s * L; i < 2 * (s + 1) * L; i++)
                    {
                        if (y[i] != 0.0f) zero = false;
                        if (y[i] != static_cast<float>(raw[i])) same = false;
                    }
                n_zero += zero;
                n_pulsed += pulsed[s];
                if (pulsed[s] && !zero) n_missed++;
                if (!zero && !same) n_wrong++;
            }
        EXPECT(n_pulsed >= 30 && n_missed == 0, "%zu of %zu pulse segments were not zeroed", n_missed, n_pulsed);
        EXPECT(n_wrong == 0, "%zu segments are neither zeros nor the converted input", n_wrong);
        // pfa 0.001 over 400 segments: a handful of false alarms at the most
        EXPECT(cond.blanked_segments() == n_zero && n_zero <= n_pulsed + 8, "%llu segments blanked, %zu read back as zeros, %zu pulsed",
            static_cast<unsigned long long>(cond.blanked_segments()), n_zero, n_pulsed);
        const double floor = scale * scale * 0.5;  // power per component
        EXPECT(std::fabs(cond.noise_power() - floor) < 0.25 * floor, "noise power %.1f, expected about %.1f", cond.noise_power(), floor);
        // a length outside the limits is reported at construction
        InMemoryConfiguration bad;
        bad.set_property("F.pulse_blanking", "true");
        bad.set_property("F.length", "5000");
        hip_signal_conditioner c1(ctx, &bad, "F", 8192, 1024, std::vector<float>(1, 1.0f));
        EXPECT(c1.last_status() == GC_ERR_INVALID, "length 5000 was accepted");
        // without the key nothing is blanked and the head follows the items
        InMemoryConfiguration off;
        off.set_property("F.input_item_type", "cshort");
        hip_signal_conditioner c2(ctx, &off, "F", 1 << 15, 4096, std::vector<float>(1, 1.0f));
        EXPECT(c2.push(raw.data(), 1000) == GC_OK && c2.head() == 1000 && !c2.pulse_blanking() && c2.blanked_segments() == 0, "conditioner without blanking: head %llu",
            static_cast<unsigned long long>(c2.head()));
    }
    gc_ctx_destroy(ctx);
    std::printf("pulse blanking: cshort, %zu pulse segments of %u samples zeroed in the ring, heads advance by whole segments\n", n_pulsed, L);
    if (g_fail)
        {
            std::printf("pulse blanking self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("pulse blanking self-test passed\n");
    return 0;
}
