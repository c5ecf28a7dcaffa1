// hybrid_group_selftest -- one hip_tracking_group over GPS L1 C/A, Galileo E1 (5 taps, 4 ms) and BeiDou B1I slots on one RF stream ring
// (one mixed device loop, one launch per pushed block) against three per-signal groups fed the same blocks and the same hand-overs:
// every Gnss_Synchro item must be equal, and every satellite must be tracked.
#include "dll_pll_tracking_adapters.h"
#include "hip_tracking_group.h"
#include <cmath>
#include <cstdio>
#include <random>
#include <utility>
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

// x[n] += A c(tau0 + n * rate / fs) exp(j (2 pi fd n / fs + 0.7)); rate in replica samples per second
static void add_signal(std::vector<gr_complex>& x, const std::vector<float>& code, double rate_hz, double carrier_hz, double fs, double fd, double delay_samples,
    double cn0_dbhz)
{
    const double amp = std::sqrt(std::pow(10.0, cn0_dbhz / 10.0) / fs);
    const double rate = rate_hz * (1.0 + fd / carrier_hz) / fs;
    const size_t L = code.size();
    const double tau0 = static_cast<double>(L) - delay_samples * rate_hz / fs;
    for (size_t i = 0; i < x.size(); i++)
        {
            const double ph = 2.0 * M_PI * fd * static_cast<double>(i) / fs + 0.7;
            const size_t chip = static_cast<size_t>(std::floor(tau0 + static_cast<double>(i) * rate)) % L;
            x[i] += gr_complex(static_cast<float>(amp * code[chip] * std::cos(ph)), static_cast<float>(amp * code[chip] * std::sin(ph)));
        }
}

struct Sat
{
    char system;
    const char* signal;
    int prn;
    double doppler, delay;
    int slot;        // slot in its per-signal group
    size_t handover; // block index of the hand-over
};

static bool same(const Gnss_Synchro& a, const Gnss_Synchro& b)
{
    return a.System == b.System && a.Signal[0] == b.Signal[0] && a.Signal[1] == b.Signal[1] && a.PRN == b.PRN && a.fs == b.fs &&
           a.Tracking_sample_counter == b.Tracking_sample_counter && a.Prompt_I == b.Prompt_I && a.Prompt_Q == b.Prompt_Q && a.CN0_dB_hz == b.CN0_dB_hz &&
           a.Carrier_Doppler_hz == b.Carrier_Doppler_hz && a.Carrier_phase_rads == b.Carrier_phase_rads && a.Code_phase_samples == b.Code_phase_samples &&
           a.Flag_valid_symbol_output == b.Flag_valid_symbol_output && a.correlation_length_ms == b.correlation_length_ms;
}

int main()
{
    if (gc_device_count() == 0)
        {
            std::printf("no GPU: libgnsscorr has no CPU fallback\n");
            return 3;
        }
    const double fs = 4e6;
    const size_t block = 4000 * 40, n_blocks = 12, n = block * n_blocks;  // 40 ms per push, 480 ms
    InMemoryConfiguration config;
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Tracking_1C.pll_bw_hz", "35.0");
    config.set_property("Tracking_1B.pll_bw_hz", "15.0");
    config.set_property("Tracking_1B.dll_bw_hz", "2.0");
    config.set_property("Tracking_B1.pll_bw_hz", "35.0");
    GpsL1CaDllPllTrackingHip gps_src(&config, "Tracking_1C", 1, 1);
    GalileoE1DllPllVemlTrackingHip gal_src(&config, "Tracking_1B", 1, 1);
    BeidouB1iDllPllTrackingHip bds_src(&config, "Tracking_B1", 1, 1);
    const Dll_Pll_Conf confs[3] = {gps_src.conf(), gal_src.conf(), bds_src.conf()};
    const int slots[3] = {3, 2, 3};
    EXPECT(confs[1].vector_length == 16000 && confs[0].vector_length == 4000 && confs[2].vector_length == 4000, "vector lengths %u / %u / %u",
        confs[0].vector_length, confs[1].vector_length, confs[2].vector_length);

    const std::vector<Sat> sats = {{'G', "1C", 3, 1200.0, 1500.0, 0, 0}, {'G', "1C", 19, -2500.0, 2900.0, 1, 0}, {'G', "1C", 27, 300.0, 100.0, 2, 3},
        {'E', "1B", 11, -1234.0, 5000.0, 0, 0}, {'E', "1B", 4, 2100.0, 12345.0, 1, 2}, {'C', "B1", 6, 800.0, 700.0, 0, 0}, {'C', "B1", 9, -3100.0, 3300.0, 2, 1}};
    std::vector<gr_complex> x(n);
    {
        std::mt19937 gen(2024);
        std::normal_distribution<float> nd(0.0f, std::sqrt(0.5f));
        for (auto& v : x) v = gr_complex(nd(gen), nd(gen));
    }
    for (const Sat& s : sats)
        {
            if (s.system == 'G')
                {
                    std::vector<float> c(1023);
                    gc_gps_l1_ca_code_gen_float(c.data(), s.prn, 0);
                    add_signal(x, c, 1.023e6, 1575.42e6, fs, s.doppler, s.delay, 47.0);
                }
            else if (s.system == 'E')
                {
                    std::vector<float> c(8184);
                    char e1b[3] = "1B";
                    gc_galileo_e1_code_gen_sinboc11_float(c.data(), e1b, s.prn);
                    add_signal(x, c, 2.046e6, 1575.42e6, fs, s.doppler, s.delay, 47.0);
                }
            else
                {
                    std::vector<float> c(2046);
                    gc_beidou_b1i_code_gen_float(c.data(), s.prn, 0);
                    add_signal(x, c, 2.046e6, 1561.098e6, fs, s.doppler, s.delay, 47.0);
                }
        }

    gc_ctx* ctx = nullptr;
    gc_stream *ring_h = nullptr, *ring_s = nullptr;
    EXPECT(gc_ctx_create(0, &ctx) == GC_OK, "context");
    EXPECT(gc_stream_create(ctx, GC_IQ_F32, 4000 * 128, 20000, &ring_h) == GC_OK && gc_stream_create(ctx, GC_IQ_F32, 4000 * 128, 20000, &ring_s) == GC_OK,
        "rings (%s)", gc_last_error());
    size_t n_h = 0, n_s = 0, bad = 0;
    std::vector<std::vector<Gnss_Synchro>> out_h, out_s[3];
    {
        // one group, one mixed engine: slots 0-2 GPS, 3-4 Galileo, 5-7 BeiDou
        std::vector<std::pair<Dll_Pll_Conf, int>> list;
        for (int k = 0; k < 3; k++) list.emplace_back(confs[k], slots[k]);
        hip_tracking_group hybrid(ctx, ring_h, list);
        EXPECT(hybrid.last_status() == GC_OK && hybrid.n_channels() == 8, "hybrid group: status %d (%s)", hybrid.last_status(), gc_last_error());
        EXPECT(hybrid.signal_of(0) == 0 && hybrid.signal_of(3) == 1 && hybrid.signal_of(4) == 1 && hybrid.signal_of(5) == 2, "hybrid group: slot ranges");
        // the same receiver as three per-signal groups on one ring
        hip_tracking_group g0(ctx, ring_s, confs[0], slots[0]), g1(ctx, ring_s, confs[1], slots[1]), g2(ctx, ring_s, confs[2], slots[2]);
        hip_tracking_group* per[3] = {&g0, &g1, &g2};
        for (int k = 0; k < 3; k++) EXPECT(per[k]->last_status() == GC_OK, "group %d: status %d (%s)", k, per[k]->last_status(), gc_last_error());
        const int offset[3] = {0, slots[0], slots[0] + slots[1]};
        auto sig_index = [](const Sat& s) { return s.system == 'G' ? 0 : s.system == 'E' ? 1 : 2; };
        for (size_t b = 0; b < n_blocks; b++)
            {
                const size_t pos = b * block;
                EXPECT(gc_stream_push(ring_h, x.data() + pos, block, nullptr) == GC_OK && gc_stream_push(ring_s, x.data() + pos, block, nullptr) == GC_OK,
                    "push (%s)", gc_last_error());
                for (const Sat& s : sats)
                    if (s.handover == b)
                        {
                            Gnss_Synchro a;
                            a.System = s.system;
                            a.Signal[0] = s.signal[0];
                            a.Signal[1] = s.signal[1];
                            a.PRN = static_cast<uint32_t>(s.prn);
                            a.Acq_delay_samples = s.delay;
                            a.Acq_doppler_hz = s.doppler + 20.0;
                            a.Acq_samplestamp_samples = 0;
                            const int k = sig_index(s);
                            EXPECT(hybrid.start_tracking(offset[k] + s.slot, a, pos) == GC_OK, "hybrid start %c%d (%s)", s.system, s.prn, gc_last_error());
                            EXPECT(per[k]->start_tracking(s.slot, a, pos) == GC_OK, "group start %c%d (%s)", s.system, s.prn, gc_last_error());
                        }
                const int ph = hybrid.run(out_h);
                EXPECT(ph >= 0, "hybrid run: status %d (%s)", hybrid.last_status(), gc_last_error());
                for (int k = 0; k < 3; k++)
                    {
                        const int ps = per[k]->run(out_s[k]);
                        EXPECT(ps >= 0, "group %d run: status %d (%s)", k, per[k]->last_status(), gc_last_error());
                    }
            }
        for (const Sat& s : sats)
            {
                const int k = sig_index(s);
                const auto& h = out_h[offset[k] + s.slot];
                const auto& g = out_s[k][s.slot];
                n_h += h.size();
                n_s += g.size();
                EXPECT(h.size() == g.size(), "%c%d: %zu items in the hybrid group, %zu in its signal's group", s.system, s.prn, h.size(), g.size());
                for (size_t i = 0; i < std::min(h.size(), g.size()); i++)
                    if (!same(h[i], g[i])) bad++;
                const double period_ms = s.system == 'E' ? 4.0 : 1.0;
                const size_t expect = static_cast<size_t>((n - s.handover * block) / fs * 1e3 / period_ms) - 3;  // the pull-in skips up to two periods; the last one is incomplete
                EXPECT(h.size() >= expect && hybrid.active(offset[k] + s.slot), "%c%d: %zu items, expected >= %zu", s.system, s.prn, h.size(), expect);
                if (h.size() < 20) continue;
                double mean = 0.0;
                for (size_t i = h.size() - 20; i < h.size(); i++) mean += h[i].Carrier_Doppler_hz;
                mean /= 20.0;
                EXPECT(std::fabs(mean - s.doppler) < 5.0 && h.back().PRN == static_cast<uint32_t>(s.prn), "%c%d: mean Doppler %.2f Hz, truth %.2f", s.system, s.prn, mean,
                    s.doppler);
            }
        EXPECT(!hybrid.active(slots[0] + slots[1] + 1) && out_h[slots[0] + slots[1] + 1].empty(), "hybrid group: the unused BeiDou slot");
        EXPECT(bad == 0, "%zu Gnss_Synchro items differ between the hybrid group and the per-signal groups", bad);
    }
    gc_stream_destroy(ring_h);
    gc_stream_destroy(ring_s);
    gc_ctx_destroy(ctx);
    std::printf("hybrid group: GPS + Galileo E1 + BeiDou B1I slots in one group (one mixed engine, one launch per block): %zu Gnss_Synchro, "
                "per-signal groups %zu, %zu differing\n",
        n_h, n_s, bad);
    if (g_fail)
        {
            std::printf("hybrid group self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("hybrid group self-test passed\n");
    return 0;
}
