// acq_resampler_selftest -- hip_acquisition_bank with use_acquisition_resampler next to one without, on ONE cshort ring at 4 Msps with
// three GPS L1 C/A satellites: the flagged bank derives a 1 Msps ring on the device (decimation 4, 97 taps, latency 48) and searches
// that; both banks must find the same satellites with Doppler within one step and code delay within one derived sample (4 ring
// samples), the flagged bank's sample stamp must be rint(derived stamp * ratio), and a hip_tracking_group on the FULL-RATE ring
// started from either bank's Gnss_Synchro must track every satellite at its true Doppler.  A BeiDou B1I bank (no optimal rate in the
// reference) must ignore the flag.  The flagged banks are updated after every push, so a second search 360 ms (three ring
// capacities) later still works; one that is not updated reports GC_ERR_STATE.  Usage: acq_resampler_selftest (needs a GPU).
#include "dll_pll_tracking_adapters.h"
#include "hip_acquisition_bank.h"
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
    const double fs = 4e6;
    const int prns[3] = {5, 14, 23};
    const double dopplers[3] = {-3300.0, 450.0, 2750.0};
    const double delays[3] = {253.0, 2020.0, 3700.0};                  // ring sample (mod 4000) at which a code period starts
    const size_t block = 4000 * 40, n_blocks = 10, n = block * n_blocks;  // 40 ms per push, 400 ms
    const double scale = 64.0;                                         // noise sigma = 45 LSB of the cshort front end
    // 55 dB-Hz: a code start half a derived sample off the 1 Msps grid costs about 4 dB of the peak, and the late search below
    // meets the satellites wherever 360 ms of code Doppler have carried them
    const double cn0_db_hz = 55.0;

    std::vector<double> re(n, 0.0), im(n, 0.0);
    for (int k = 0; k < 3; k++)
        {
            std::vector<float> code(1023);
            gc_gps_l1_ca_code_gen_float(code.data(), prns[k], 0);
            const double amp = std::sqrt(std::pow(10.0, cn0_db_hz / 10.0) / fs);
            const double rate = 1.023e6 * (1.0 + dopplers[k] / 1575.42e6) / fs;
            const double tau0 = 1023.0 - delays[k] * 1.023e6 / fs;
            for (size_t i = 0; i < n; i++)
                {
                    const double ph = 2.0 * M_PI * std::fmod(dopplers[k] / fs * static_cast<double>(i), 1.0) + 0.7;
                    const size_t chip = static_cast<size_t>(std::floor(tau0 + static_cast<double>(i) * rate)) % 1023;
                    re[i] += amp * code[chip] * std::cos(ph);
                    im[i] += amp * code[chip] * std::sin(ph);
                }
        }
    std::vector<int16_t> raw(2 * n);
    {
        std::mt19937 gen(91);
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
    config.set_property("GNSS-SDR.internal_fs_sps", "4000000");
    config.set_property("Tracking_1C.pll_bw_hz", "50.0");
    GpsL1CaDllPllTrackingHip conf_source(&config, "Tracking_1C", 1, 1);

    gc_ctx* ctx = nullptr;
    EXPECT(gc_ctx_create(0, &ctx) == GC_OK, "context (%s)", gc_last_error());
    gc_stream* ring = nullptr;
    EXPECT(gc_stream_create(ctx, GC_IQ_I16, 4000 * 128, 8000, &ring) == GC_OK, "ring (%s)", gc_last_error());
    size_t n_items = 0;
    if (ctx && ring)
        {
            std::vector<uint32_t> all;
            for (uint32_t p = 1; p <= 32; p++) all.push_back(p);
            const uint32_t step = 100;
            // statistic = peak / N^4 / input power: noise cells average 1 / N, the largest of 32 x 100 x N about 16 / N; 55 dB-Hz gives about
            // 300 / N at full rate and, with the main lobe cut at +-476 kHz, 100 - 200 / N on the derived ring
            hip_acquisition_bank full(ctx, ring, 'G', "1C", all, 4000000, 5000, step, 30.0f / 4000.0f, 1, true, GC_IQ_I16);
            hip_acquisition_bank res(ctx, ring, 'G', "1C", all, 4000000, 5000, step, 25.0f / 1000.0f, 1, true, GC_IQ_I16, true);
            // two dwells (first-to-second-peak statistic): the stamp is that of the LAST dwell
            hip_acquisition_bank res2(ctx, ring, 'G', "1C", all, 4000000, 5000, step, 2.0f, 2, true, GC_IQ_I16, true);
            EXPECT(full.last_status() == GC_OK && res.last_status() == GC_OK && res2.last_status() == GC_OK, "banks: status %d / %d / %d (%s)", full.last_status(),
                res.last_status(), res2.last_status(), gc_last_error());
            EXPECT(full.resampler_ratio() == 1 && full.consumed_samples() == 4000, "full-rate bank: ratio %u, %u samples per dwell", full.resampler_ratio(),
                full.consumed_samples());
            EXPECT(res.resampler_ratio() == 4 && res.resampler_latency_samples() == 48 && res.consumed_samples() == 4000,
                "resampled bank: ratio %u, latency %u, %u ring samples per dwell", res.resampler_ratio(), res.resampler_latency_samples(), res.consumed_samples());
            // BeiDou B1I has no optimal acquisition rate: the flag changes nothing
            std::vector<uint32_t> few = {1, 2, 3, 4, 5};
            hip_acquisition_bank b1(ctx, ring, 'C', "B1", few, 4000000, 5000, 250, 1.0f, 1, true, GC_IQ_I16);
            hip_acquisition_bank b1_flag(ctx, ring, 'C', "B1", few, 4000000, 5000, 250, 1.0f, 1, true, GC_IQ_I16, true);
            EXPECT(b1.last_status() == GC_OK && b1_flag.last_status() == GC_OK && b1_flag.resampler_ratio() == 1 && b1_flag.consumed_samples() == b1.consumed_samples(),
                "B1I banks: status %d / %d, ratio %u, %u / %u samples per dwell (%s)", b1.last_status(), b1_flag.last_status(), b1_flag.resampler_ratio(),
                b1.consumed_samples(), b1_flag.consumed_samples(), gc_last_error());

            hip_tracking_group group_full(ctx, ring, conf_source.conf(), 8, GC_IQ_I16);
            hip_tracking_group group_res(ctx, ring, conf_source.conf(), 8, GC_IQ_I16);
            EXPECT(group_full.last_status() == GC_OK && group_res.last_status() == GC_OK, "groups: status %d / %d (%s)", group_full.last_status(),
                group_res.last_status(), gc_last_error());
            std::vector<std::vector<Gnss_Synchro>> out_full, out_res;
            std::vector<Gnss_Synchro> det_full, det_res, det_res2, det_late;
            // a flagged bank nobody updates while the ring runs three capacities ahead
            hip_acquisition_bank res_idle(ctx, ring, 'G', "1C", all, 4000000, 5000, step, 25.0f / 1000.0f, 1, true, GC_IQ_I16, true);
            const uint64_t late_index = 9 * block + 1002;
            const uint64_t first_index = 1002;  // not a multiple of the decimation: the derived search starts at ceil(1002 / 4) = 251
            for (size_t b = 0; b < n_blocks; b++)
                {
                    EXPECT(gc_stream_push(ring, raw.data() + 2 * b * block, block, nullptr) == GC_OK, "push (%s)", gc_last_error());
                    if (b == 0)
                        {
                            det_full = full.search(first_index);
                            det_res = res.search(first_index);
                            det_res2 = res2.search(first_index);
                            EXPECT(full.last_status() == GC_OK && res.last_status() == GC_OK && res2.last_status() == GC_OK, "search: status %d / %d / %d (%s)",
                                full.last_status(), res.last_status(), res2.last_status(), gc_last_error());
                            for (size_t d = 0; d < det_full.size() && d < 8; d++)
                                EXPECT(group_full.start_tracking(static_cast<int>(d), det_full[d], det_full[d].Acq_samplestamp_samples) == GC_OK,
                                    "full-rate hand-over (%s)", gc_last_error());
                            for (size_t d = 0; d < det_res.size() && d < 8; d++)
                                EXPECT(group_res.start_tracking(static_cast<int>(d), det_res[d], det_res[d].Acq_samplestamp_samples) == GC_OK,
                                    "resampled hand-over (%s)", gc_last_error());
                            const std::vector<Gnss_Synchro> c0 = b1.search(first_index), c1 = b1_flag.search(first_index);
                            EXPECT(b1.last_status() == GC_OK && b1_flag.last_status() == GC_OK && c0.size() == c1.size(), "B1I search: status %d / %d, %zu / %zu detections (%s)",
                                b1.last_status(), b1_flag.last_status(), c0.size(), c1.size(), gc_last_error());
                            for (size_t s = 0; s < few.size(); s++)
                                EXPECT(b1.statistic(s) == b1_flag.statistic(s), "B1I PRN %u: statistic %.9g without the flag, %.9g with it", few[s], b1.statistic(s),
                                    b1_flag.statistic(s));
                        }
                    // sporadic searches, continuous pushes: the derived rings follow the ring push by push
                    EXPECT(res.update() == GC_OK && res2.update() == GC_OK && full.update() == GC_OK, "update after push %zu: status %d / %d (%s)", b,
                        res.last_status(), res2.last_status(), gc_last_error());
                    if (b == n_blocks - 1)
                        {
                            det_late = res.search(late_index);
                            EXPECT(res.last_status() == GC_OK, "late search: status %d (%s)", res.last_status(), gc_last_error());
                            const std::vector<Gnss_Synchro> none = res_idle.search(late_index);
                            EXPECT(none.empty() && res_idle.last_status() == GC_ERR_STATE && res_idle.update() == GC_ERR_STATE,
                                "a flagged bank that was never updated: %zu detections, status %d", none.size(), res_idle.last_status());
                        }
                    EXPECT(group_full.run(out_full) >= 0, "full-rate group: run status %d (%s)", group_full.last_status(), gc_last_error());
                    EXPECT(group_res.run(out_res) >= 0, "resampled group: run status %d (%s)", group_res.last_status(), gc_last_error());
                }
            EXPECT(det_full.size() == 3 && det_res.size() == 3, "detections: %zu at full rate, %zu resampled", det_full.size(), det_res.size());
            // Acq_samplestamp_samples = rint(samp_count * ratio), samp_count = the derived index of the last dwell's first sample
            const uint64_t derived_first = (first_index + 3) / 4;
            for (const Gnss_Synchro& g : det_res)
                EXPECT(g.Acq_samplestamp_samples == static_cast<uint64_t>(std::rint(static_cast<double>(derived_first) * 4.0)), "PRN %u: resampled stamp %llu", g.PRN,
                    static_cast<unsigned long long>(g.Acq_samplestamp_samples));
            for (const Gnss_Synchro& g : det_full)
                EXPECT(g.Acq_samplestamp_samples == first_index, "PRN %u: full-rate stamp %llu", g.PRN, static_cast<unsigned long long>(g.Acq_samplestamp_samples));
            int seen2 = 0;
            for (const Gnss_Synchro& g : det_res2)
                {
                    EXPECT(g.Acq_samplestamp_samples == static_cast<uint64_t>(std::rint(static_cast<double>(derived_first + 1000) * 4.0)), "PRN %u: two-dwell stamp %llu",
                        g.PRN, static_cast<unsigned long long>(g.Acq_samplestamp_samples));
                    for (int k = 0; k < 3; k++)
                        if (g.PRN == static_cast<uint32_t>(prns[k])) seen2++;
                }
            int seen_late = 0;
            for (const Gnss_Synchro& g : det_late)
                {
                    EXPECT(g.Acq_samplestamp_samples == (late_index + 3) / 4 * 4, "PRN %u: late stamp %llu", g.PRN, static_cast<unsigned long long>(g.Acq_samplestamp_samples));
                    for (int k = 0; k < 3; k++)
                        if (g.PRN == static_cast<uint32_t>(prns[k]) && std::fabs(g.Acq_doppler_hz - dopplers[k]) <= step) seen_late++;
                }
            EXPECT(seen_late == 3 && det_late.size() == 3, "search after 360 ms of pushes: %d of the 3 satellites among %zu detections", seen_late, det_late.size());
            EXPECT(seen2 == 3, "two-dwell resampled bank: %d of the 3 satellites among %zu detections", seen2, det_res2.size());
            for (int k = 0; k < 3; k++)
                {
                    int df = -1, dr = -1;
                    for (size_t d = 0; d < det_full.size(); d++)
                        if (det_full[d].PRN == static_cast<uint32_t>(prns[k])) df = static_cast<int>(d);
                    for (size_t d = 0; d < det_res.size(); d++)
                        if (det_res[d].PRN == static_cast<uint32_t>(prns[k])) dr = static_cast<int>(d);
                    EXPECT(df >= 0 && dr >= 0, "PRN %d: found at full rate %d, resampled %d", prns[k], df >= 0, dr >= 0);
                    if (df < 0 || dr < 0) continue;
                    const Gnss_Synchro &gf = det_full[df], &gr = det_res[dr];
                    EXPECT(std::fabs(gf.Acq_doppler_hz - dopplers[k]) <= step && std::fabs(gr.Acq_doppler_hz - gf.Acq_doppler_hz) <= step,
                        "PRN %d: Doppler %.1f Hz at full rate, %.1f Hz resampled (truth %.1f)", prns[k], gf.Acq_doppler_hz, gr.Acq_doppler_hz, dopplers[k]);
                    // both delays as ring positions of a code start, modulo the 4000 samples of a code period: stamp + delay
                    const double pos_f = static_cast<double>(gf.Acq_samplestamp_samples) + gf.Acq_delay_samples;
                    const double pos_r = static_cast<double>(gr.Acq_samplestamp_samples) + gr.Acq_delay_samples;
                    EXPECT(mod_distance(pos_f, delays[k], 4000.0) <= 2.0 && mod_distance(pos_r, pos_f, 4000.0) <= 4.0,
                        "PRN %d: code start at ring sample %.1f at full rate, %.1f resampled (delay %.1f), truth %.1f", prns[k], std::fmod(pos_f, 4000.0),
                        std::fmod(pos_r + 4000.0, 4000.0), gr.Acq_delay_samples, delays[k]);
                    // tracking on the full-rate ring from either hand-over
                    double mean[2] = {0.0, 0.0};
                    const std::vector<Gnss_Synchro>* items[2] = {df < static_cast<int>(out_full.size()) ? &out_full[df] : nullptr,
                        dr < static_cast<int>(out_res.size()) ? &out_res[dr] : nullptr};
                    const bool active[2] = {group_full.active(df), group_res.active(dr)};
                    for (int w = 0; w < 2; w++)
                        {
                            const char* name = w == 0 ? "full-rate" : "resampled";
                            EXPECT(items[w] != nullptr && items[w]->size() >= 390 && active[w], "PRN %d, %s hand-over: %zu items, tracking %d", prns[k], name,
                                items[w] ? items[w]->size() : static_cast<size_t>(0), static_cast<int>(active[w]));
                            if (items[w] == nullptr || items[w]->size() < 50) continue;
                            n_items += items[w]->size();
                            for (size_t i = items[w]->size() - 50; i < items[w]->size(); i++) mean[w] += (*items[w])[i].Carrier_Doppler_hz;
                            mean[w] /= 50.0;
                            EXPECT(std::fabs(mean[w] - dopplers[k]) < 5.0, "PRN %d, %s hand-over: mean Doppler %.2f Hz, truth %.2f", prns[k], name, mean[w], dopplers[k]);
                        }
                    // "as closely as from the full-rate result": the same bound for both (the one conditioner_selftest holds this loop to),
                    // and the resampled hand-over keeps lock for as many code periods -- its start differs by at most the 2 samples
                    // between the stamps and the pull-in's alignment, one period
                    if (items[0] != nullptr && items[1] != nullptr)
                        EXPECT(items[1]->size() + 1 >= items[0]->size(), "PRN %d: %zu items from the full-rate hand-over, %zu from the resampled one", prns[k],
                            items[0]->size(), items[1]->size());
                    std::printf("PRN %d: Doppler %.0f / %.0f Hz, delay %.1f / %.1f, tracked Doppler error %.2f / %.2f Hz (full rate / resampled)\n", prns[k],
                        gf.Acq_doppler_hz, gr.Acq_doppler_hz, gf.Acq_delay_samples, gr.Acq_delay_samples, mean[0] - dopplers[k], mean[1] - dopplers[k]);
                }
        }
    if (ring) gc_stream_destroy(ring);
    if (ctx) gc_ctx_destroy(ctx);
    std::printf("acquisition resampler: cshort ring at 4 Msps, search at 1 Msps on a derived ring; 3 satellites acquired by both banks and tracked, %zu Gnss_Synchro\n",
        n_items);
    if (g_fail)
        {
            std::printf("acquisition resampler self-test: %d failure(s)\n", g_fail);
            return 1;
        }
    std::printf("acquisition resampler self-test passed\n");
    return 0;
}
