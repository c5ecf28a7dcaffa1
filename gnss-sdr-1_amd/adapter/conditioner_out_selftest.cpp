// conditioner_out_selftest -- hip_signal_conditioner with output_item_type "cshort" and "cbyte", configured from the reference
// adapter's keys: a short cshort stream (a tone near the IF in noise) is pushed in ragged blocks through three conditioners that
// differ in output_item_type alone.  The gr_complex ring is the yardstick: the host quantises each of its components -- v = c * scale
// (one float32 product), clamp to the integer range, rintf (ties to even), NaN -> 0 -- and every stored component of the integer
// rings, and the clipped count, must be equal to that.  output_scale is absent for "cbyte", so it must come out as 127, the
// reference's complex_float_to_complex_byte; the cshort run uses a scale that makes some components clip.  An unknown
// output_item_type must fail at construction, and hip_ring_decimator must take the same keys.  Usage: conditioner_out_selftest
// (needs a GPU).
#include "hip_ring_decimator.h"
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

static InMemoryConfiguration make_config(const char* out_type, const char* out_scale)
{
    InMemoryConfiguration config;
    config.set_property("InputFilter.IF", "1250000");
    config.set_property("InputFilter.sampling_frequency", "16000000");
    config.set_property("InputFilter.decimation_factor", "4");
    config.set_property("InputFilter.input_item_type", "cshort");
    config.set_property("InputFilter.filter_type", "lowpass");
    config.set_property("InputFilter.bw", "1600000");
    config.set_property("InputFilter.tw", "612000");
    if (out_type) config.set_property("InputFilter.output_item_type", out_type);
    if (out_scale) config.set_property("InputFilter.output_scale", out_scale);
    return config;
}

// pushes the stream in ragged blocks; the whole output stays resident
static void push_all(hip_signal_conditioner& cond, const std::vector<int16_t>& raw, size_t n)
{
    const size_t blocks[] = {37, 1, 5000, 999, 250, 20001};
    size_t pos = 0, b = 0;
    while (pos < n)
        {
            const size_t m = std::min(blocks[b++ % (sizeof blocks / sizeof blocks[0])], n - pos);
            EXPECT(cond.push(raw.data() + 2 * pos, m) == GC_OK, "push at %zu (%s)", pos, gc_last_error());
            pos += m;
        }
}

static int quantise(float c, float scale, float lo, float hi, uint64_t* clipped)
{
    float v = c * scale;
    if (v > hi)
        {
            v = hi;
            ++*clipped;
        }
    else if (v < lo)
        {
            v = lo;
            ++*clipped;
        }
    return v != v ? 0 : static_cast<int>(std::rint(v));
}

template <typename T>
static void run_case(gc_ctx* ctx, const char* out_type, const char* scale_key, int want_format, float want_scale, float lo, float hi,
    const std::vector<int16_t>& raw, size_t n, const std::vector<float>& y, bool want_clipping)
{
    InMemoryConfiguration config = make_config(out_type, scale_key);
    hip_signal_conditioner cond(ctx, &config, "InputFilter", 1 << 15, 4096);
    EXPECT(cond.last_status() == GC_OK && cond.ring() != nullptr, "%s: status %d (%s)", out_type, cond.last_status(), gc_last_error());
    if (cond.last_status() != GC_OK) return;
    EXPECT(cond.output_format() == want_format && cond.output_scale() == want_scale, "%s: format %d, scale %g", out_type, cond.output_format(),
        static_cast<double>(cond.output_scale()));
    push_all(cond, raw, n);
    const size_t n_out = y.size() / 2;
    EXPECT(cond.head() == n_out, "%s: head %llu, expected %zu", out_type, static_cast<unsigned long long>(cond.head()), n_out);
    std::vector<T> got(2 * n_out);
    EXPECT(gc_stream_read(cond.ring(), 0, n_out, got.data()) == GC_OK, "%s: read (%s)", out_type, gc_last_error());
    uint64_t want_clipped = 0;
    size_t bad = 0, first_bad = 0;
    int peak = 0;
    for (size_t i = 0; i < 2 * n_out; i++)
        {
            const int q = quantise(y[i], want_scale, lo, hi, &want_clipped);
            if (static_cast<int>(got[i]) != q && bad++ == 0) first_bad = i;
            peak = std::max(peak, std::abs(q));
        }
    EXPECT(bad == 0, "%s: %zu of %zu components differ from the host quantisation, first at output %zu: %d vs %d", out_type, bad, 2 * n_out, first_bad / 2,
        static_cast<int>(got[first_bad]), quantise(y[first_bad], want_scale, lo, hi, &want_clipped));
    const uint64_t clipped = cond.clipped_components();
    EXPECT(clipped == want_clipped, "%s: %llu clipped components, the host counts %llu", out_type, static_cast<unsigned long long>(clipped),
        static_cast<unsigned long long>(want_clipped));
    EXPECT(peak > 16, "%s: the largest stored value is %d: the comparison says little", out_type, peak);
    EXPECT((want_clipped > 0) == want_clipping, "%s: %llu clipped components", out_type, static_cast<unsigned long long>(want_clipped));
    std::printf("%s, scale %g: %zu outputs equal to the host quantisation of the gr_complex ring (peak %d, %llu clipped)\n", out_type,
        static_cast<double>(want_scale), n_out, peak, static_cast<unsigned long long>(clipped));
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
    const size_t n = 60001, n_out = (n + 3) / 4;
    std::vector<int16_t> raw(2 * n);
    std::mt19937 gen(23);
    std::normal_distribution<double> nd(0.0, 1.0);
    for (size_t i = 0; i < n; i++)
        {
            // unit-power noise plus a tone of amplitude 0.9 at IF + 200 kHz, 100 LSB to the unit: the conditioned tone is about 90
            const double ph = 2.0 * M_PI * 1.45e6 / 16e6 * static_cast<double>(i) + 0.4;
            raw[2 * i] = static_cast<int16_t>(std::lrint(100.0 * (nd(gen) * std::sqrt(0.5) + 0.9 * std::cos(ph))));
            raw[2 * i + 1] = static_cast<int16_t>(std::lrint(100.0 * (nd(gen) * std::sqrt(0.5) + 0.9 * std::sin(ph))));
        }
    // the yardstick: the gr_complex ring (output_item_type absent)
    std::vector<float> y(2 * n_out);
    {
        InMemoryConfiguration config = make_config(nullptr, nullptr);
        hip_signal_conditioner cond(ctx, &config, "InputFilter", 1 << 15, 4096);
        EXPECT(cond.last_status() == GC_OK, "gr_complex: status %d (%s)", cond.last_status(), gc_last_error());
        EXPECT(cond.output_format() == GC_IQ_F32 && cond.output_scale() == 1.0f && cond.clipped_components() == 0, "gr_complex: format %d", cond.output_format());
        push_all(cond, raw, n);
        EXPECT(cond.head() == n_out && gc_stream_read(cond.ring(), 0, n_out, y.data()) == GC_OK, "gr_complex: read (%s)", gc_last_error());
    }
    // cshort with the default scale: nothing clips; with 400: the tone's peaks (about 90 x 400) pass 32767
    run_case<int16_t>(ctx, "cshort", nullptr, GC_IQ_I16, 1.0f, -32768.0f, 32767.0f, raw, n, y, false);
    run_case<int16_t>(ctx, "cshort", "400", GC_IQ_I16, 400.0f, -32768.0f, 32767.0f, raw, n, y, true);
    // cbyte: the scale is 127 when the key is absent, and values near 90 x 127 clip; 1.25 keeps most of them inside
    run_case<int8_t>(ctx, "cbyte", nullptr, GC_IQ_I8, 127.0f, -128.0f, 127.0f, raw, n, y, true);
    run_case<int8_t>(ctx, "cbyte", "1.25", GC_IQ_I8, 1.25f, -128.0f, 127.0f, raw, n, y, true);
    {
        InMemoryConfiguration config = make_config("cint", nullptr);
        hip_signal_conditioner refused(ctx, &config, "InputFilter", 8192, 1024);
        EXPECT(refused.last_status() == GC_ERR_INVALID && refused.ring() == nullptr, "output_item_type cint was accepted (status %d)", refused.last_status());
        uint64_t made = 0;
        EXPECT(refused.push(raw.data(), 16, nullptr, &made) == GC_ERR_INVALID, "a refused conditioner took samples");
    }
    {
        // the ring decimator's adapter takes the same keys: 4 Msps -> 1 Msps into a cbyte ring, scale 127 by default
        InMemoryConfiguration config;
        config.set_property("Resampler.output_item_type", "cbyte");
        gc_stream* src = nullptr;
        EXPECT(gc_stream_create(ctx, GC_IQ_I16, 1 << 15, 4096, &src) == GC_OK, "source ring (%s)", gc_last_error());
        hip_ring_decimator dec(ctx, src, 4000000, 1000000, &config, "Resampler");
        EXPECT(dec.enabled() && dec.open(4096, 1000) == GC_OK, "decimator: status %d (%s)", dec.last_status(), gc_last_error());
        EXPECT(dec.output_format() == GC_IQ_I8 && dec.output_scale() == 127.0f, "decimator: format %d, scale %g", dec.output_format(),
            static_cast<double>(dec.output_scale()));
        uint64_t made = 0;
        EXPECT(gc_stream_push(src, raw.data(), 20000, nullptr) == GC_OK && dec.update(nullptr, &made) == GC_OK && made == 5000, "decimator: update made %llu (%s)",
            static_cast<unsigned long long>(made), gc_last_error());
        EXPECT(dec.clipped_components() > 0, "decimator: nothing clipped at scale 127");
        config.set_property("Resampler.output_item_type", "short");
        hip_ring_decimator refused(ctx, src, 4000000, 1000000, &config, "Resampler");
        EXPECT(refused.last_status() == GC_ERR_INVALID && !refused.enabled(), "decimator: output_item_type short was accepted");
        gc_stream_destroy(src);
    }
    gc_ctx_destroy(ctx);
    if (g_fail)
        {
            std::printf("conditioner output self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("conditioner output self-test passed\n");
    return 0;
}
