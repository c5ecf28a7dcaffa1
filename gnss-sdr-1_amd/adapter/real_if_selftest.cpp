// real_if_selftest -- hip_signal_conditioner on REAL samples at an intermediate frequency: input_item_type "byte" (one int8 per
// sample) and "2bit" (four samples per byte), both with IF = sampling_frequency / 4, configured from the reference adapter's keys.  At
// a quarter of the sampling rate the mixer's cosine and sine are exactly 0 and +-1, so the host restates the ring bit for bit: z[n] =
// (x cos, -(x sin)), then h[0] z first and one fmaf per tap in tap order, in float32.  A short synthetic stream is pushed in ragged
// blocks and every output of the ring is compared with ==.  Usage: real_if_selftest (needs a GPU).
#include "hip_signal_conditioner.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
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

// y[m] for real samples x at IF = fs / 4: phi(n) = n / 4 turns exactly
static std::vector<float> restate(const std::vector<int>& x, const std::vector<float>& h, int D)
{
    static const float kCos[4] = {1.0f, 0.0f, -1.0f, 0.0f}, kSin[4] = {0.0f, 1.0f, 0.0f, -1.0f};
    const size_t n_out = (x.size() + D - 1) / D;
    std::vector<float> y(2 * n_out);
    for (size_t m = 0; m < n_out; m++)
        {
            float re = 0.0f, im = 0.0f;
            for (size_t k = 0; k < h.size(); k++)
                {
                    const long long n = static_cast<long long>(m) * D - static_cast<long long>(k);
                    float zr = 0.0f, zi = 0.0f;
                    if (n >= 0)
                        {
                            const float v = static_cast<float>(x[static_cast<size_t>(n)]);
                            zr = v * kCos[n & 3];
                            zi = -(v * kSin[n & 3]);
                        }
                    if (k == 0)
                        {
                            re = h[0] * zr;
                            im = h[0] * zi;
                        }
                    else
                        {
                            re = std::fmaf(h[k], zr, re);
                            im = std::fmaf(h[k], zi, im);
                        }
                }
            y[2 * m] = re;
            y[2 * m + 1] = im;
        }
    return y;
}

// pushes `bytes` (n samples, spb samples per byte; spb = 1: one int8 each) in ragged blocks and compares the whole ring
static void run_case(gc_ctx* ctx, const char* item_type, int spb, int D, const std::vector<int>& x, const std::vector<int8_t>& bytes)
{
    InMemoryConfiguration config;
    config.set_property("InputFilter.IF", "4000000");
    config.set_property("InputFilter.sampling_frequency", "16000000");
    config.set_property("InputFilter.decimation_factor", std::to_string(D));
    config.set_property("InputFilter.input_item_type", item_type);
    config.set_property("InputFilter.filter_type", "lowpass");
    config.set_property("InputFilter.bw", "1600000");
    config.set_property("InputFilter.tw", "612000");
    const size_t n = x.size(), n_out = (n + D - 1) / D;
    hip_signal_conditioner cond(ctx, &config, "InputFilter", 1 << 16, 4096);
    EXPECT(cond.last_status() == GC_OK && cond.ring() != nullptr, "%s: status %d (%s)", item_type, cond.last_status(), gc_last_error());
    if (cond.last_status() != GC_OK) return;
    EXPECT(cond.taps().size() == 63 && cond.fs_out() == 16e6 / D && cond.item_size() == 1 && cond.real_input() && cond.samples_per_byte() == (spb == 4 ? 4 : 0),
        "%s: %zu taps, fs_out %.0f, item size %zu, %d samples per byte", item_type, cond.taps().size(), cond.fs_out(), cond.item_size(), cond.samples_per_byte());
    const size_t blocks[] = {4, 8, 5000, 64, 12, 20000, 4, 9972, 132};  // samples; multiples of 4 for the packed type
    size_t pos = 0, b = 0;
    while (pos < n)
        {
            const size_t m = std::min(blocks[b++ % (sizeof blocks / sizeof blocks[0])], n - pos);
            uint64_t first = 0, made = 0;
            EXPECT(cond.push(bytes.data() + pos / spb, m, &first, &made) == GC_OK, "%s: push (%s)", item_type, gc_last_error());
            EXPECT(first == (pos + D - 1) / D && first + made == (pos + m + D - 1) / D, "%s: push at %zu: outputs [%llu, +%llu)", item_type, pos,
                static_cast<unsigned long long>(first), static_cast<unsigned long long>(made));
            pos += m;
        }
    EXPECT(cond.head() == n_out, "%s: head %llu, expected %zu", item_type, static_cast<unsigned long long>(cond.head()), n_out);
    if (spb == 4)
        {
            // a partial byte is refused and leaves the stream where it was; so is blanking for the packed type
            EXPECT(cond.push(bytes.data(), 6) == GC_ERR_INVALID && cond.head() == n_out, "2bit: a push of 6 samples was accepted");
            InMemoryConfiguration blank = config;
            blank.set_property("InputFilter.pulse_blanking", "true");
            hip_signal_conditioner refused(ctx, &blank, "InputFilter", 8192, 1024);
            EXPECT(refused.last_status() == GC_ERR_INVALID, "2bit: pulse_blanking was accepted (status %d)", refused.last_status());
        }
    std::vector<float> got(2 * n_out);
    EXPECT(gc_stream_read(cond.ring(), 0, n_out, got.data()) == GC_OK, "%s: read (%s)", item_type, gc_last_error());
    const std::vector<float> want = restate(x, cond.taps(), D);
    size_t bad = 0, first_bad = 0;
    double peak = 0.0;
    for (size_t i = 0; i < 2 * n_out; i++)
        {
            if (!(got[i] == want[i]) && bad++ == 0) first_bad = i;
            peak = std::max(peak, static_cast<double>(std::fabs(want[i])));
        }
    EXPECT(bad == 0, "%s: %zu of %zu components differ from the host restatement, first at output %zu: %.9g vs %.9g", item_type, bad, 2 * n_out, first_bad / 2,
        static_cast<double>(got[first_bad]), static_cast<double>(want[first_bad]));
    EXPECT(peak > 0.5, "%s: the restatement's peak is %.3g: the comparison says nothing", item_type, peak);
    std::printf("%s at 16 Msps, IF 4 MHz, D = %d: %zu samples in %zu bytes -> %zu outputs, all equal to the host restatement (peak %.3f)\n", item_type, D, n,
        bytes.size(), n_out, peak);
}

int main()
{
    if (gc_device_count() == 0)
        {
            std::printf("no GPU: libgnsscorr has no CPU fallback\n");
            return 3;
        }
    gc_ctx* ctx = nullptr;
    EXPECT(gc_ctx_create(0, &ctx) == GC_OK, "context (%s)", gc_last_error());
    if (ctx == nullptr) return 1;
    const size_t n = 60004;  // a multiple of 4, not of 64
    std::mt19937 gen(19);
    std::normal_distribution<double> nd(0.0, 1.0);
    {
        // "byte": a tone 300 kHz above the IF in noise, sigma 20 LSB
        std::vector<int> x(n);
        std::vector<int8_t> bytes(n);
        for (size_t i = 0; i < n; i++)
            {
                const double v = 20.0 * nd(gen) + 40.0 * std::cos(2.0 * M_PI * 4.3e6 / 16e6 * static_cast<double>(i) + 0.4);
                x[i] = static_cast<int>(std::lrint(std::fmax(-127.0, std::fmin(127.0, v))));
                bytes[i] = static_cast<int8_t>(x[i]);
            }
        run_case(ctx, "byte", 1, 2, x, bytes);
    }
    {
        // "2bit": the same kind of signal through a 2-bit quantiser with levels -2 .. 1; sample 4b + i in bits 2i .. 2i + 1 of byte b
        std::vector<int> x(n);
        std::vector<int8_t> bytes(n / 4);
        for (size_t i = 0; i < n; i++)
            {
                const double v = nd(gen) + 1.5 * std::cos(2.0 * M_PI * 4.3e6 / 16e6 * static_cast<double>(i) + 0.4);
                x[i] = static_cast<int>(std::fmax(-2.0, std::fmin(1.0, std::floor(v))));
            }
        for (size_t b = 0; b < n / 4; b++)
            {
                unsigned byte = 0;
                for (int i = 0; i < 4; i++) byte |= (static_cast<unsigned>(x[4 * b + i]) & 3u) << (2 * i);
                bytes[b] = static_cast<int8_t>(byte);
            }
        run_case(ctx, "2bit", 4, 4, x, bytes);
    }
    gc_ctx_destroy(ctx);
    if (g_fail)
        {
            std::printf("real IF self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("real IF self-test passed\n");
    return 0;
}
