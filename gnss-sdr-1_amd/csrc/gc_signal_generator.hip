// gc_signal_generator.hip -- gc_signal_generator_*: the source stage of an RF ring.  A generator is the ring's producer, as a
// conditioner is (gc_ring_stage.h: the claim, the geometry of a piece, the state of a quantised output), but has no input: its
// kernel (siggen_kernels.hip) synthesises scenario samples straight into HBM.  The ring does the bookkeeping of every append
// (gc_stream_produce): the split at the wrap, the wait for readers of what is evicted, the event, the head.
//
// Which scenario sample a ring sample is, and every phase in it, is a closed form of the sample's absolute number
// (siggen_phase.h); the doubles of the C ABI become Q0.64 words here, by the one rule gnsscorr.h states (sg_plan).
// gc_siggen_reference_satellite maps the reference block's keys to a satellite with the code generators of gc_codes.cpp.
#include "gc_ring_stage.h"
#include "siggen_kernels.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

struct gc_signal_generator
{
    gc_ctx* ctx = nullptr;
    gc_ctx_ref ctx_ref;
    gc_stream* out = nullptr;  // holds a reference
    SiggenSat* d_sats = nullptr;
    float* d_tables = nullptr;
    signed char* d_secondary = nullptr;
    unsigned n_sats = 0, n_table_floats = 0;
    int tables_in_lds = 0;
    float sigma = 0.0f;
    uint64_t seed = 0, t0 = 0;
    uint64_t head = 0;  // samples generated so far
    gc_quantised_output quant;
    std::mutex mtx;  // one generate at a time
};

namespace
{
// floor(x 2^64) of x in [0, 1): exact, a double has 53 bits
inline uint64_t sg_q64(double x) { return (uint64_t)std::ldexp(x, 64); }
// q - floor(q) in [0, 1); a tiny negative q rounds to 1, which is 0 turns
inline double sg_frac(double q)
{
    const double f = q - std::floor(q);
    return f >= 1.0 ? 0.0 : f;
}

struct sg_words
{
    uint64_t code_step_q, code_phase0_q, carr_step_q, carr_phase0_q;
};

gc_status sg_plan(const char* who, const gc_siggen_sat* sat, double fs_hz, sg_words* w)
{
    GC_REQUIRE(sat, "%s: NULL satellite", who);
    GC_REQUIRE(std::isfinite(fs_hz) && fs_hz > 0.0, "%s: fs_hz must be finite and positive", who);
    GC_REQUIRE(sat->code_periods_per_sample > 0.0 && sat->code_periods_per_sample < 1.0, "%s: code_periods_per_sample %g is outside (0, 1)", who,
        sat->code_periods_per_sample);
    GC_REQUIRE(sat->code_phase0_periods >= 0.0 && sat->code_phase0_periods < 1.0, "%s: code_phase0_periods %g is outside [0, 1)", who, sat->code_phase0_periods);
    GC_REQUIRE(std::isfinite(sat->doppler_hz), "%s: doppler_hz is not finite", who);
    GC_REQUIRE(std::isfinite(sat->carrier_phase0_turns), "%s: carrier_phase0_turns is not finite", who);
    w->code_step_q = sg_q64(sat->code_periods_per_sample);
    w->code_phase0_q = sg_q64(sat->code_phase0_periods);
    w->carr_step_q = sg_q64(sg_frac(sat->doppler_hz / fs_hz));
    w->carr_phase0_q = sg_q64(sg_frac(sat->carrier_phase0_turns));
    GC_REQUIRE(w->code_step_q != 0, "%s: code_periods_per_sample %g rounds to a step of 0", who, sat->code_periods_per_sample);
    return GC_OK;
}

// every argument of create that can be judged without a device; *total: table entries of all components
gc_status sg_check_conf(const gc_siggen_conf* conf, unsigned* total)
{
    static const char who[] = "gc_signal_generator_create";
    GC_REQUIRE(conf, "%s: NULL configuration", who);
    GC_REQUIRE(conf->n_sats >= 1 && conf->n_sats <= GC_SIGGEN_MAX_SATS, "%s: %u satellites, outside 1..%d", who, conf->n_sats, GC_SIGGEN_MAX_SATS);
    GC_REQUIRE(conf->sats, "%s: NULL satellites", who);
    GC_REQUIRE(std::isfinite(conf->fs_hz) && conf->fs_hz > 0.0, "%s: fs_hz must be finite and positive", who);
    GC_REQUIRE(std::isfinite(conf->noise_sigma) && conf->noise_sigma >= 0.0, "%s: noise_sigma %g is not finite and non-negative", who, conf->noise_sigma);
    GC_REQUIRE(conf->table_placement <= GC_SIGGEN_TABLES_LDS, "%s: unknown table placement %u", who, conf->table_placement);
    *total = 0;
    for (uint32_t s = 0; s < conf->n_sats; s++)
        {
            const gc_siggen_sat& sat = conf->sats[s];
            GC_REQUIRE(sat.n_components >= 1 && sat.n_components <= 2, "%s: satellite %u has %u components, outside 1..2", who, s, sat.n_components);
            GC_REQUIRE(sat.table_len >= 1 && sat.table_len <= GC_SIGGEN_MAX_TABLE, "%s: satellite %u has table_len %u, outside 1..%d", who, s, sat.table_len,
                GC_SIGGEN_MAX_TABLE);
            sg_words w;
            const gc_status st = sg_plan(who, &sat, conf->fs_hz, &w);
            if (st != GC_OK) return st;
            GC_REQUIRE(std::isfinite(sat.amplitude), "%s: the amplitude of satellite %u is not finite", who, s);
            for (uint32_t c = 0; c < sat.n_components; c++)
                {
                    const gc_siggen_component& k = sat.comp[c];
                    GC_REQUIRE(k.table, "%s: component %u of satellite %u has a NULL table", who, c, s);
                    GC_REQUIRE(k.secondary_len <= GC_SIGGEN_MAX_SECONDARY, "%s: component %u of satellite %u has secondary_len %u, above %d", who, c, s,
                        k.secondary_len, GC_SIGGEN_MAX_SECONDARY);
                    GC_REQUIRE(k.secondary_len == 0 || k.secondary, "%s: component %u of satellite %u has a NULL secondary code", who, c, s);
                    GC_REQUIRE(k.axis == 0 || k.axis == 1, "%s: component %u of satellite %u has axis %d, neither 0 nor 1", who, c, s, (int)k.axis);
                    GC_REQUIRE(std::isfinite(k.gain), "%s: the gain of component %u of satellite %u is not finite", who, c, s);
                    for (uint32_t i = 0; i < sat.table_len; i++)
                        GC_REQUIRE(std::isfinite(k.table[i]), "%s: entry %u of the table of component %u of satellite %u is not finite", who, i, c, s);
                    for (uint32_t i = 0; i < k.secondary_len; i++)
                        GC_REQUIRE(k.secondary[i] == 1 || k.secondary[i] == -1, "%s: symbol %u of the secondary code of component %u of satellite %u is not +-1", who,
                            i, c, s);
                    *total += sat.table_len;
                }
        }
    GC_REQUIRE(conf->table_placement != GC_SIGGEN_TABLES_LDS || *total <= GC_SIGGEN_LDS_FLOATS, "%s: %u table entries do not fit in LDS (%d at most)", who, *total,
        GC_SIGGEN_LDS_FLOATS);
    return GC_OK;
}

// Where a launch's tables live when the caller leaves it to the library.  Measured on MI355X ("Signal generator
// on the ring"): the copy every workgroup makes costs more than the L2 hits it saves, so HBM through L2 it is.
inline bool sg_auto_in_lds(unsigned /*total_table_floats*/) { return false; }

struct sg_writer : gc_ring_writer
{
    gc_signal_generator* g;
    explicit sg_writer(gc_signal_generator* g_) : g(g_) {}
    bool writes_mirror() const override { return true; }
    gc_status write(gc_stream* s, uint64_t idx, uint64_t pos, uint64_t* len) override
    {
        SiggenJob job;
        job.sats = g->d_sats;
        job.tables = g->d_tables;
        job.secondary = g->d_secondary;
        job.n_sats = g->n_sats;
        job.n_table_floats = g->n_table_floats;
        job.tables_in_lds = g->tables_in_lds;
        job.sigma = g->sigma;
        job.seed = g->seed;
        job.t_first = g->t0 + idx;
        job.n_out = (unsigned)*len;
        job.ring_pos = (unsigned)pos;
        job.out = gc_ring_stage_piece(s, pos, *len, g->quant.scale, g->quant.d_clipped);
        const int per_cu = g->tables_in_lds ? 2 : 8;
        GC_HIP(siggen_launch(s->iq_format, s->copy_stream, job, per_cu * std::max(1, g->ctx->n_cus)));
        return GC_OK;
    }
};

void sg_release(gc_signal_generator* g)
{
    if (g->out) gc_ring_stage_release(g->out);  // waits for the kernels that read what is freed below
    (void)hipFree(g->d_sats);
    (void)hipFree(g->d_tables);
    (void)hipFree(g->d_secondary);
    gc_quantised_output_free(&g->quant);
    delete g;
}

// slot -> frequency channel of the constellation the reference was written against (its GLONASS_PRN; the adapters carry the same)
const int kGlonassChannel[24] = {8, 1, -4, 5, 6, 1, -4, 5, 6, -2, -7, 0, -1, -2, -7, 0, -1, 4, -3, 3, -5, 4, -3, 3};

gc_status sg_secondary(const char* signal, uint32_t prn, int8_t* dest, uint32_t* len)
{
    char text[GC_SIGGEN_MAX_SECONDARY + 1];
    int32_t n = 0;
    const gc_status st = gc_secondary_code(signal, prn, text, (int32_t)sizeof text, &n);
    if (st != GC_OK) return st;
    for (int32_t i = 0; i < n; i++) dest[i] = text[i] == '0' ? 1 : -1;
    *len = (uint32_t)n;
    return GC_OK;
}
}  // namespace

extern "C" {

size_t gc_siggen_component_size(void) { return sizeof(gc_siggen_component); }
size_t gc_siggen_sat_size(void) { return sizeof(gc_siggen_sat); }
size_t gc_siggen_conf_size(void) { return sizeof(gc_siggen_conf); }

gc_status gc_signal_generator_plan(const gc_siggen_sat* sat, double fs_hz, uint64_t* code_step_q, uint64_t* code_phase0_q, uint64_t* carr_step_q,
    uint64_t* carr_phase0_q)
{
    sg_words w;
    const gc_status st = sg_plan("gc_signal_generator_plan", sat, fs_hz, &w);
    if (st != GC_OK) return st;
    if (code_step_q) *code_step_q = w.code_step_q;
    if (code_phase0_q) *code_phase0_q = w.code_phase0_q;
    if (carr_step_q) *carr_step_q = w.carr_step_q;
    if (carr_phase0_q) *carr_phase0_q = w.carr_phase0_q;
    return GC_OK;
}

gc_status gc_signal_generator_create(gc_ctx* ctx, const gc_siggen_conf* conf, gc_stream* out_ring, gc_signal_generator** out)
{
    static const char who[] = "gc_signal_generator_create";
    if (out) *out = nullptr;
    // the configuration first, before anything that needs a device
    unsigned total = 0;
    gc_status st = sg_check_conf(conf, &total);
    if (st != GC_OK) return st;
    GC_REQUIRE(ctx && out_ring && out, "%s: NULL argument", who);
    GC_REQUIRE(out_ring->ctx == ctx, "%s: the output ring belongs to another context", who);
    GC_REQUIRE(out_ring->iq_format == GC_IQ_F32 || out_ring->quantised_output,
        "%s: the output ring must be GC_IQ_F32, or an integer ring opened with gc_stream_accept_quantised_output", who);
    // the device's image of the configuration
    std::vector<SiggenSat> sats(conf->n_sats);
    std::vector<float> tables;
    std::vector<signed char> secondary(1, 1);  // never empty: hipMalloc(0) returns no pointer
    tables.reserve(total);
    for (uint32_t s = 0; s < conf->n_sats; s++)
        {
            const gc_siggen_sat& in = conf->sats[s];
            sg_words w;
            st = sg_plan(who, &in, conf->fs_hz, &w);
            if (st != GC_OK) return st;
            SiggenSat& d = sats[s];
            std::memset(&d, 0, sizeof d);
            d.code_step_q = w.code_step_q;
            d.code_phase0_q = w.code_phase0_q;
            d.carr_step_q = w.carr_step_q;
            d.carr_phase0_q = w.carr_phase0_q;
            d.amplitude = (float)in.amplitude;
            d.table_len = in.table_len;
            d.n_comp = in.n_components;
            for (uint32_t c = 0; c < in.n_components; c++)
                {
                    const gc_siggen_component& k = in.comp[c];
                    SiggenComp& dc = d.comp[c];
                    dc.table_off = (unsigned)tables.size();
                    tables.insert(tables.end(), k.table, k.table + in.table_len);
                    dc.secondary_off = (unsigned)secondary.size();
                    dc.secondary_len = k.secondary_len;
                    if (k.secondary_len) secondary.insert(secondary.end(), k.secondary, k.secondary + k.secondary_len);
                    dc.periods_per_symbol = k.periods_per_symbol;
                    dc.period_offset = k.period_offset;
                    dc.axis = k.axis;
                    dc.gain = k.gain;
                }
        }
    gc_device_guard dev(ctx->device);
    const unsigned why = gc_ring_stage_claim(out_ring);
    if (why & GC_RING_HAS_PRODUCER) return gc_fail(GC_ERR_STATE, "%s: the ring already has a producer on the device", who);
    if (why) return gc_fail(GC_ERR_STATE, "%s: samples have been pushed into the ring already", who);
    gc_signal_generator* g = new gc_signal_generator();
    g->ctx = ctx;
    g->ctx_ref.bind(ctx);
    g->out = out_ring;
    gc_stream_keep(out_ring);
    g->n_sats = conf->n_sats;
    g->n_table_floats = (unsigned)tables.size();
    g->tables_in_lds = conf->table_placement == GC_SIGGEN_TABLES_LDS || (conf->table_placement == GC_SIGGEN_TABLES_AUTO && sg_auto_in_lds(total)) ? 1 : 0;
    g->sigma = (float)conf->noise_sigma;
    g->seed = conf->seed;
    g->t0 = conf->t0;
    hipError_t e = hipMalloc(&g->d_sats, sizeof(SiggenSat) * sats.size());
    if (e == hipSuccess) e = hipMemcpy(g->d_sats, sats.data(), sizeof(SiggenSat) * sats.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&g->d_tables, sizeof(float) * tables.size());
    if (e == hipSuccess) e = hipMemcpy(g->d_tables, tables.data(), sizeof(float) * tables.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&g->d_secondary, secondary.size());
    if (e == hipSuccess) e = hipMemcpy(g->d_secondary, secondary.data(), secondary.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = gc_quantised_output_alloc(&g->quant, out_ring);
    if (e != hipSuccess)
        {
            sg_release(g);
            return gc_fail(GC_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
        }
    *out = g;
    return GC_OK;
}

gc_status gc_signal_generator_destroy(gc_signal_generator* g)
{
    if (!g) return GC_OK;
    gc_device_guard dev(g->ctx->device);
    sg_release(g);
    return GC_OK;
}

gc_status gc_signal_generator_generate(gc_signal_generator* g, uint64_t n_samples, uint64_t* first_index)
{
    if (first_index) *first_index = 0;
    GC_REQUIRE(g, "gc_signal_generator_generate: NULL handle");
    std::lock_guard<std::mutex> one_call(g->mtx);
    if (first_index) *first_index = g->head;
    gc_device_guard dev(g->ctx->device);
    sg_writer w(g);
    uint64_t left = n_samples;
    while (left > 0)
        {
            const uint64_t n = std::min<uint64_t>(left, g->out->capacity);
            uint64_t first = 0;
            const gc_status st = gc_stream_produce(g->out, n, &first, w, true);
            if (st != GC_OK) return st;
            if (first != g->head)
                return gc_fail(GC_ERR_STATE, "gc_signal_generator_generate: the ring's head %llu is not the generator's sample %llu", (unsigned long long)first,
                    (unsigned long long)g->head);
            g->head += n;
            left -= n;
        }
    return GC_OK;
}

gc_status gc_signal_generator_info(gc_signal_generator* g, uint64_t* head)
{
    GC_REQUIRE(g, "gc_signal_generator_info: NULL handle");
    std::lock_guard<std::mutex> one_call(g->mtx);
    if (head) *head = g->head;
    return GC_OK;
}

gc_status gc_signal_generator_set_output_scale(gc_signal_generator* g, float scale)
{
    const gc_status st = gc_quantised_output_check_scale("gc_signal_generator_set_output_scale", scale, g ? g->out : nullptr);
    if (st != GC_OK) return st;
    std::lock_guard<std::mutex> one_call(g->mtx);
    if (g->head != 0) return gc_fail(GC_ERR_STATE, "gc_signal_generator_set_output_scale: samples have been generated already");
    g->quant.scale = scale;
    return GC_OK;
}

gc_status gc_signal_generator_output_info(gc_signal_generator* g, int32_t* out_format, float* scale, uint64_t* clipped_components)
{
    GC_REQUIRE(g, "gc_signal_generator_output_info: NULL handle");
    std::lock_guard<std::mutex> one_call(g->mtx);
    return gc_quantised_output_info(&g->quant, g->ctx, g->out, out_format, scale, clipped_components);
}

gc_status gc_siggen_reference_satellite(const char* system, const char* signal, uint32_t prn, double cn0_db, double doppler_hz, uint32_t delay_chips,
    uint32_t delay_sec, double fs_hz, double bw_bb, int data_flag, int noise_flag, double intermediate_freq_hz, gc_siggen_sat* sat, float* tables,
    uint32_t table_capacity, int8_t* secondaries, double* noise_sigma)
{
    static const char who[] = "gc_siggen_reference_satellite";
    GC_REQUIRE(system && signal && sat && tables && secondaries, "%s: NULL argument", who);
    GC_REQUIRE(std::isfinite(fs_hz) && fs_hz >= 1000.0 && fs_hz <= 2147483647.0, "%s: fs_hz %g is outside 1e3 .. 2^31 - 1", who, fs_hz);
    GC_REQUIRE(std::isfinite(bw_bb) && bw_bb > 0.0, "%s: BW_BB must be finite and positive", who);
    GC_REQUIRE(std::isfinite(cn0_db) && std::isfinite(doppler_hz) && std::isfinite(intermediate_freq_hz), "%s: an argument is not finite", who);
    const std::string sys(system), sig(signal);
    std::memset(sat, 0, sizeof *sat);
    float* table[2] = {tables, tables + table_capacity};
    int8_t* secondary[2] = {secondaries, secondaries + GC_SIGGEN_MAX_SECONDARY};
    double period_s = 1e-3, carrier_hz = doppler_hz, galileo = 1.0;
    uint32_t chips = 0, delay_samples_of_chips = 0;  // the code's chips; chips the reference delays as whole samples
    gc_siggen_component* c0 = &sat->comp[0];
    gc_siggen_component* c1 = &sat->comp[1];
    sat->n_components = 1;
    c0->gain = c1->gain = 1.0f;
    if (sys == "G" && sig == "1C")
        {
            chips = 1023;
            sat->table_len = 1023;
            GC_REQUIRE(table_capacity >= sat->table_len, "%s: table_capacity %u is below %u", who, table_capacity, sat->table_len);
            GC_REQUIRE(delay_chips < chips, "%s: delay_chips %u is not below %u", who, delay_chips, chips);
            // the block delays by a chip shift of the code, not by samples
            const gc_status st = gc_gps_l1_ca_code_gen_float(table[0], (int32_t)prn, chips - delay_chips);
            if (st != GC_OK) return st;
            c0->periods_per_symbol = data_flag ? 20u : 0u;
        }
    else if (sys == "R" && sig == "1G")
        {
            chips = 511;
            sat->table_len = 511;
            GC_REQUIRE(table_capacity >= sat->table_len, "%s: table_capacity %u is below %u", who, table_capacity, sat->table_len);
            GC_REQUIRE(delay_chips < chips, "%s: delay_chips %u is not below %u", who, delay_chips, chips);
            GC_REQUIRE(prn < 24, "%s: no frequency channel for GLONASS slot %u (0..23)", who, prn);
            const gc_status st = gc_glonass_l1_ca_code_gen_float(table[0], chips - delay_chips);
            if (st != GC_OK) return st;
            carrier_hz = intermediate_freq_hz + 562500.0 * kGlonassChannel[prn] + doppler_hz;
            c0->periods_per_symbol = data_flag ? 20u : 0u;  // the block's 50 bit/s
        }
    else if (sys == "E" && sig == "1B")
        {
            chips = 4092;
            period_s = 4e-3;
            galileo = std::sqrt(0.5);
            sat->table_len = 12 * 4092;
            sat->n_components = 2;
            GC_REQUIRE(table_capacity >= sat->table_len, "%s: table_capacity %u is below %u", who, table_capacity, sat->table_len);
            GC_REQUIRE(delay_chips < chips, "%s: delay_chips %u is not below %u", who, delay_chips, chips);
            // one period of CBOC at its own rate, 12 entries per chip: the sampled generator at 12 x 1.023 MHz does not resample
            std::vector<float> one(2 * (size_t)sat->table_len);
            for (int c = 0; c < 2; c++)
                {
                    int32_t n = 0;
                    const gc_status st = gc_galileo_e1_code_gen_complex_sampled(one.data(), c == 0 ? "1B" : "1C", 1, prn, 12 * 1023000, 0, &n);
                    if (st != GC_OK) return st;
                    if ((uint32_t)n != sat->table_len) return gc_fail(GC_ERR_STATE, "%s: %d samples in a CBOC period", who, (int)n);
                    for (uint32_t i = 0; i < sat->table_len; i++) table[c][i] = one[2 * (size_t)i];
                }
            delay_samples_of_chips = delay_chips;
            c0->periods_per_symbol = data_flag ? 1u : 0u;
            c1->gain = -1.0f;
            const gc_status st = sg_secondary("1C", prn, secondary[1], &c1->secondary_len);
            if (st != GC_OK) return st;
            c1->secondary = secondary[1];
        }
    else if (sys == "E" && sig == "5X")
        {
            chips = 10230;
            galileo = std::sqrt(0.5);
            sat->table_len = 10230;
            sat->n_components = 2;
            GC_REQUIRE(table_capacity >= sat->table_len, "%s: table_capacity %u is below %u", who, table_capacity, sat->table_len);
            GC_REQUIRE(delay_chips < chips, "%s: delay_chips %u is not below %u", who, delay_chips, chips);
            std::vector<float> iq(2 * (size_t)10230);
            gc_status st = gc_galileo_e5_a_code_gen_complex_primary(iq.data(), (int32_t)prn, "5X");
            if (st != GC_OK) return st;
            for (uint32_t i = 0; i < 10230; i++)
                {
                    table[0][i] = iq[2 * (size_t)i];
                    table[1][i] = iq[2 * (size_t)i + 1];
                }
            delay_samples_of_chips = delay_chips;
            c0->periods_per_symbol = data_flag ? 20u : 0u;
            c1->axis = 1;
            c0->period_offset = c1->period_offset = delay_sec;
            st = sg_secondary("5I", prn, secondary[0], &c0->secondary_len);
            if (st == GC_OK) st = sg_secondary("5Q", prn, secondary[1], &c1->secondary_len);
            if (st != GC_OK) return st;
            c0->secondary = secondary[0];
            c1->secondary = secondary[1];
        }
    else
        return gc_fail(GC_ERR_INVALID, "%s: unknown system / signal \"%s\" / \"%s\" (G 1C, R 1G, E 1B, E 5X)", who, system, signal);
    c0->table = table[0];
    if (sat->n_components > 1) c1->table = table[1];
    // samples per code period as the block rounds them, and its whole-sample delay of the Galileo codes
    const double n_per = std::round(fs_hz * period_s);
    const double delay_samples = std::floor((double)delay_samples_of_chips * n_per / (double)chips);
    sat->code_periods_per_sample = 1.0 / n_per;
    // one sample less 2^-16 in front of the boundary: floor() of the table index then picks the sampler's ceil((i + 1) L / N) - 1
    sat->code_phase0_periods = sg_frac((std::fmod(n_per - delay_samples, n_per) + 1.0 - 1.0 / 65536.0) / n_per);
    sat->doppler_hz = carrier_hz;
    sat->carrier_phase0_turns = 0.0;
    sat->amplitude = noise_flag ? std::sqrt(std::pow(10.0, cn0_db / 10.0) / (bw_bb * fs_hz / 2.0)) * galileo : 1.0;
    if (noise_sigma) *noise_sigma = noise_flag ? 1.0 : 0.0;
    return GC_OK;
}

}  // extern "C"
