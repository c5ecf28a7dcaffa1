/*!
 * \file hip_signal_conditioner.h
 * \brief The signal conditioner of one RF source on the GPU: data-type adapter + frequency-translating FIR input filter + decimation,
 * writing the RF stream ring that hip_acquisition_bank and hip_tracking_group read.
 *
 * In the reference a signal conditioner (data_type_adapter, input_filter, resampler) sits between every source and its channels
 * (gnss_flowgraph.cc:496-499); for a capture at an intermediate frequency or from a wide-band front end the input filter is
 * Freq_Xlating_Fir_Filter (src/algorithms/input_filter/adapters/freq_xlating_fir_filter.cc).  This class takes that adapter's
 * configuration keys under its role --
 *   IF                   [Hz]  frequency moved to 0                           (default 0)
 *   sampling_frequency   [Hz]  rate of the raw samples                        (default 4000000)
 *   decimation_factor          D, 1..64                                       (default 1)
 *   input_item_type            "gr_complex" | "cshort" | "cbyte": complex samples, 8 / 4 / 2 bytes each (default "gr_complex");
 *                              "float" | "short" | "byte": REAL samples at an intermediate frequency, 4 / 2 / 1 bytes each, the
 *                              reference adapter's other three item types (GC_RAW_REAL_F32 / _I16 / _I8);
 *                              "2bit": real samples packed four to a byte, least-significant pair first, two's complement -- the
 *                              input of the reference's unpack_byte_2bit_samples block, taken packed (GC_RAW_REAL_2BIT)
 *   filter_type                "lowpass": a windowed-sinc design from bw / tw (gc_fir_low_pass, the counterpart of
 *                              gr::filter::firdes::low_pass(1.0, sampling_frequency, bw, tw)); anything else: the caller passes
 *                              the taps (e.g. a Remez design from the band keys) to the constructor
 *   bw, tw               [Hz]  cut-off and transition width                   (defaults (sampling_frequency / D) / 2 and bw / 10)
 *   pulse_blanking             true: the reference's Pulse_Blanking_Filter (src/algorithms/input_filter/adapters/
 *                              pulse_blanking_filter.cc) on the raw samples   (default false), with that adapter's keys
 *   pfa                        false-alarm probability of a segment           (default 0.04)
 *   length                     samples per segment                            (default 32)
 *   segments_est               segments of a noise-floor estimate             (default 12500)
 *   segments_reset             segments after which the floor is re-estimated (default 5000000)
 *   output_item_type           "gr_complex" | "cshort" | "cbyte": the ring's format, GC_IQ_F32 / GC_IQ_I16 / GC_IQ_I8 -- 8 / 4 / 2 bytes
 *                              per sample for everything that reads it           (default "gr_complex")
 *   output_scale               factor in front of the clamp of a cshort / cbyte ring: q = rint(clamp(y * output_scale))
 *                              (default 1; 127 for "cbyte" when the key is absent, the reference's complex_float_to_complex_byte)
 * -- owns a ring of output_item_type at sampling_frequency / D plus the device conditioner (gc_conditioner) that writes it, and hands the
 * ring to the acquisition bank and the tracking group.  general_work of the source-side block
 * calls push(items, n) with n counted in SAMPLES for every item type (a multiple of 4 for "2bit": samples_per_byte() is 4 there,
 * which item_size() cannot express); pulse_blanking is not available with "2bit".  Everything downstream addresses the ring by sample number at the OUTPUT rate.  The filter delays the signal
 * by group_delay_samples() output samples; as in the reference, that is left in the observables.
 *
 * Order: blanking acts on the raw samples BEFORE the translating filter, so that a pulse is removed before the low-pass smears it over
 * its neighbours.  The reference's Pulse_Blanking_Filter adapter with IF != 0 translates and filters first and blanks second; for
 * IF = 0 the two are the same definition.  With blanking on, the ring's head advances by whole segments: head() is
 * ceil(floor(items / length) * length / D).
 */
#ifndef GNSSCORR_HIP_SIGNAL_CONDITIONER_H_
#define GNSSCORR_HIP_SIGNAL_CONDITIONER_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include <string>
#include <vector>

class hip_signal_conditioner
{
public:
    /*! ring_capacity / max_window: size of the output ring and its longest window, in OUTPUT samples (gc_stream_create);
     *  taps: used unless filter_type is "lowpass" */
    hip_signal_conditioner(gc_ctx* ctx, ConfigurationInterface* configuration, const std::string& role, uint64_t ring_capacity, uint32_t max_window,
        const std::vector<float>& taps = std::vector<float>())
        : d_role(role), d_taps(taps)
    {
        d_if = configuration->property(role + ".IF", 0.0);
        d_fs_in = configuration->property(role + ".sampling_frequency", 4000000.0);
        d_decimation = configuration->property(role + ".decimation_factor", static_cast<int32_t>(1));
        d_item_type = configuration->property(role + ".input_item_type", std::string("gr_complex"));
        const std::string filter_type = configuration->property(role + ".filter_type", std::string("bandpass"));
        int format = GC_IQ_F32;
        if (d_item_type == "float") format = GC_RAW_REAL_F32;
        else if (d_item_type == "short") format = GC_RAW_REAL_I16;
        else if (d_item_type == "byte") format = GC_RAW_REAL_I8;
        else if (d_item_type == "2bit") format = GC_RAW_REAL_2BIT;
        else if (!gnsscorr_iq_format(d_item_type, &format))
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        if (d_decimation < 1 || d_fs_in <= 0.0)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        d_out_item_type = configuration->property(role + ".output_item_type", std::string("gr_complex"));
        if (!gnsscorr_iq_format(d_out_item_type, &d_out_format))
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        d_out_scale = configuration->property(role + ".output_scale", d_out_format == GC_IQ_I8 ? 127.0f : 1.0f);
        if (filter_type == "lowpass")
            {
                const double bw = configuration->property(role + ".bw", (d_fs_in / d_decimation) / 2.0);
                const double tw = configuration->property(role + ".tw", bw / 10.0);
                int n = 0;
                d_status = gc_fir_low_pass(1.0, d_fs_in, bw, tw, nullptr, 0, &n);
                if (d_status != GC_OK) return;
                d_taps.assign(static_cast<size_t>(n), 0.0f);
                d_status = gc_fir_low_pass(1.0, d_fs_in, bw, tw, d_taps.data(), n, &n);
                if (d_status != GC_OK) return;
            }
        gc_conditioner_conf c;
        c.fs_in = d_fs_in;
        c.translate_hz = d_if;
        c.decimation = static_cast<uint32_t>(d_decimation);
        c.n_taps = static_cast<uint32_t>(d_taps.size());
        c.in_format = format;
        d_format = format;
        c.reserved = 0;
        d_blanking = configuration->property(role + ".pulse_blanking", false);
        gc_blanking_conf b;
        b.pfa = configuration->property(role + ".pfa", 0.04f);
        b.threshold = 0.0f;  // from pfa and length
        const int32_t length = configuration->property(role + ".length", static_cast<int32_t>(32));
        const int32_t segments_est = configuration->property(role + ".segments_est", static_cast<int32_t>(12500));
        const int32_t segments_reset = configuration->property(role + ".segments_reset", static_cast<int32_t>(5000000));
        if (d_blanking && (length < 1 || segments_est < 1 || segments_reset < 0))
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        b.length = static_cast<uint32_t>(length);
        b.segments_est = static_cast<uint32_t>(segments_est);
        b.segments_reset = static_cast<uint32_t>(segments_reset);
        b.reserved = 0;
        d_status = gc_stream_create(ctx, d_out_format, ring_capacity, max_window, &d_ring);
        if (d_status == GC_OK && d_out_format != GC_IQ_F32) d_status = gc_stream_accept_quantised_output(d_ring);
        if (d_status == GC_OK) d_status = gc_conditioner_create(ctx, &c, d_taps.data(), d_ring, &d_cond);
        if (d_status == GC_OK && d_out_format != GC_IQ_F32) d_status = gc_conditioner_set_output_scale(d_cond, d_out_scale);
        if (d_status == GC_OK && d_blanking) d_status = gc_conditioner_set_pulse_blanking(d_cond, &b);
        if (d_status != GC_OK && d_cond != nullptr)
            {
                // a half-configured conditioner takes no samples: push() keeps reporting the construction failure
                gc_conditioner_destroy(d_cond);
                d_cond = nullptr;
            }
    }
    ~hip_signal_conditioner()
    {
        if (d_cond) gc_conditioner_destroy(d_cond);
        if (d_ring) gc_stream_destroy(d_ring);
    }
    hip_signal_conditioner(const hip_signal_conditioner&) = delete;
    hip_signal_conditioner& operator=(const hip_signal_conditioner&) = delete;

    //! the conditioned ring: pass it to hip_acquisition_bank / hip_tracking_group together with fs_out()
    gc_stream* ring() const { return d_ring; }
    //! GNSS-SDR.internal_fs_sps of everything downstream
    double fs_out() const { return d_fs_in / d_decimation; }
    double fs_in() const { return d_fs_in; }
    int decimation() const { return d_decimation; }
    const std::vector<float>& taps() const { return d_taps; }
    //! delay of a symmetric filter, in output samples
    double group_delay_samples() const { return d_taps.empty() ? 0.0 : (static_cast<double>(d_taps.size()) - 1.0) / 2.0 / d_decimation; }
    //! bytes of one raw item; for "2bit" an item is a byte of four samples: see samples_per_byte()
    size_t item_size() const
    {
        switch (d_format)
            {
            case GC_IQ_F32: return 8;
            case GC_IQ_I16:
            case GC_RAW_REAL_F32: return 4;
            case GC_IQ_I8:
            case GC_RAW_REAL_I16: return 2;
            default: return 1;
            }
    }
    //! raw samples in one byte: 4 for "2bit", 0 for every type whose samples are whole bytes (item_size() of them)
    int samples_per_byte() const { return d_format == GC_RAW_REAL_2BIT ? 4 : 0; }
    //! true when the raw samples are real ("float", "short", "byte", "2bit")
    bool real_input() const { return d_format >= GC_RAW_REAL_F32; }
    //! gc_iq_format of the ring (output_item_type) and the factor in front of its clamp (1 for gr_complex)
    int output_format() const { return d_out_format; }
    float output_scale() const { return d_out_format == GC_IQ_F32 ? 1.0f : d_out_scale; }
    //! components of a cshort / cbyte ring that hit the clamp so far (0 for gr_complex); waits for the pushes so far
    uint64_t clipped_components() const
    {
        uint64_t n = 0;
        if (d_cond) gc_conditioner_output_info(d_cond, nullptr, nullptr, &n);
        return n;
    }
    std::string role() const { return d_role; }
    std::string implementation() const { return "Freq_Xlating_Fir_Filter"; }

    /*! n_items raw SAMPLES of input_item_type (for "2bit" a multiple of 4, in n_items / 4 bytes); first_out / n_out (optional): the
     *  outputs they completed.  Asynchronous. */
    gc_status push(const void* items, uint64_t n_items, uint64_t* first_out = nullptr, uint64_t* n_out = nullptr)
    {
        if (d_cond == nullptr) return d_status;  // construction failed
        d_status = gc_conditioner_push(d_cond, items, n_items, first_out, n_out);
        return d_status;
    }
    //! output samples produced so far (the ring's head)
    uint64_t head() const
    {
        uint64_t h = 0;
        if (d_cond) gc_conditioner_info(d_cond, nullptr, &h);
        return h;
    }
    bool pulse_blanking() const { return d_blanking; }
    //! segments zeroed so far (0 without pulse_blanking); waits for the pushes so far
    uint64_t blanked_segments() const
    {
        uint64_t n = 0;
        if (d_cond && d_blanking) gc_conditioner_blanking_info(d_cond, nullptr, &n, nullptr, nullptr, nullptr);
        return n;
    }
    //! the blanking stage's noise-floor estimate, power per real component in raw units (0 without pulse_blanking); waits likewise
    float noise_power() const
    {
        float p = 0.0f;
        if (d_cond && d_blanking) gc_conditioner_blanking_info(d_cond, nullptr, nullptr, &p, nullptr, nullptr);
        return p;
    }
    gc_status last_status() const { return d_status; }

private:
    std::string d_role, d_item_type, d_out_item_type;
    std::vector<float> d_taps;
    double d_if = 0.0, d_fs_in = 0.0;
    int32_t d_decimation = 1;
    int d_format = GC_IQ_F32, d_out_format = GC_IQ_F32;
    float d_out_scale = 1.0f;
    bool d_blanking = false;
    gc_stream* d_ring = nullptr;
    gc_conditioner* d_cond = nullptr;
    gc_status d_status = GC_OK;
};

#endif  // GNSSCORR_HIP_SIGNAL_CONDITIONER_H_
