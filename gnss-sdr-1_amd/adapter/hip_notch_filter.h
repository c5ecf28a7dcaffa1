/*!
 * \file hip_notch_filter.h
 * \brief The notch input filters of a signal conditioner on the GPU: a ring derived from another ring with continuous-wave
 * interference excised.
 *
 * The reference's input filters Notch_Filter and Notch_Filter_Lite (src/algorithms/input_filter/adapters/notch_filter.cc,
 * notch_filter_lite.cc; blocks notch_cc.cc, notch_lite_cc.cc) detect, segment by segment, energy above the estimated noise floor
 * and run a one-pole notch on the segments that carry it.  These classes take those adapters' configuration keys under their role --
 *   pfa                     false-alarm probability of one segment                       (default 0.001)
 *   p_c_factor              the pole's radius                                            (default 0.9)
 *   length                  samples per segment                                          (default 32)
 *   segments_est            segments of a noise-floor estimate                           (default 12500)
 *   segments_reset          segments after which the floor is estimated again            (default 5000000)
 *   item_type               "gr_complex" only: anything else is refused, where the reference warns and builds no block
 *   dump, dump_filename     accepted and ignored
 *   coeff_rate       [Hz]   lite: how often a coefficient is computed, with SignalSource.sampling_frequency (default 4000000):
 *                           segments_coeff = max(1, int((fs / coeff_rate) / float(length)))      (default fs * 0.1)
 * -- and two of this library:
 *   noise_floor             "reference" (default): the block's mean of decibels; "linear": the mean of powers (gnsscorr.h)
 *   threshold               0 (default): from pfa and length; otherwise used as is
 * -- own the derived ring and the device stage (gc_ring_notch) that writes it from `source`, and update() appends the segments the
 * source's samples so far complete.  `source` is any gr_complex ring: pushed from the host, or hip_signal_conditioner::ring().
 */
#ifndef GNSSCORR_HIP_NOTCH_FILTER_H_
#define GNSSCORR_HIP_NOTCH_FILTER_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include <algorithm>
#include <string>

class hip_notch_filter_base
{
public:
    ~hip_notch_filter_base()
    {
        if (d_notch) gc_ring_notch_destroy(d_notch);
        if (d_ring) gc_stream_destroy(d_ring);
    }
    hip_notch_filter_base(const hip_notch_filter_base&) = delete;
    hip_notch_filter_base& operator=(const hip_notch_filter_base&) = delete;

    //! appends the segments the source's samples so far complete (asynchronous)
    gc_status update(uint64_t* first_out = nullptr, uint64_t* n_out = nullptr)
    {
        if (d_notch == nullptr) return d_status;
        d_status = gc_ring_notch_update(d_notch, first_out, n_out);
        return d_status;
    }
    //! the derived ring, at the source's rate
    gc_stream* ring() const { return d_ring; }
    const gc_notch_conf& conf() const { return d_conf; }
    //! samples made so far (the derived ring's head)
    uint64_t head() const
    {
        uint64_t h = 0;
        if (d_notch) gc_ring_notch_info(d_notch, nullptr, &h);
        return h;
    }
    //! segments decided and filtered so far (synchronous)
    gc_status segments(uint64_t* decided, uint64_t* filtered) { return d_notch ? gc_ring_notch_state(d_notch, decided, filtered, nullptr, nullptr, nullptr, nullptr, nullptr) : d_status; }
    gc_status last_status() const { return d_status; }

protected:
    hip_notch_filter_base(gc_ctx* ctx, gc_stream* source, ConfigurationInterface* configuration, const std::string& role, bool lite, uint64_t ring_capacity,
        uint32_t max_window)
    {
        const std::string item_type = configuration->property(role + ".item_type", std::string("gr_complex"));
        (void)configuration->property(role + ".dump", false);
        d_conf.pfa = configuration->property(role + ".pfa", 0.001f);
        d_conf.p_c_factor = configuration->property(role + ".p_c_factor", 0.9f);
        const int32_t length = configuration->property(role + ".length", static_cast<int32_t>(32));
        const int32_t est = configuration->property(role + ".segments_est", static_cast<int32_t>(12500));
        const int32_t reset = configuration->property(role + ".segments_reset", static_cast<int32_t>(5000000));
        d_conf.threshold = configuration->property(role + ".threshold", 0.0f);
        const std::string floor = configuration->property(role + ".noise_floor", std::string("reference"));
        d_conf.segments_coeff = 1;
        if (lite)
            {
                const float samp_freq = configuration->property("SignalSource.sampling_frequency", 4000000.0f);
                const float coeff_rate = configuration->property(role + ".coeff_rate", samp_freq * 0.1f);
                if (length > 0 && coeff_rate > 0.0f) d_conf.segments_coeff = static_cast<uint32_t>(std::max(1, static_cast<int>((samp_freq / coeff_rate) / static_cast<float>(length))));
            }
        if (item_type != "gr_complex" || (floor != "reference" && floor != "linear") || length < 0 || est < 0 || reset < 0)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        d_conf.length = static_cast<uint32_t>(length);
        d_conf.segments_est = static_cast<uint32_t>(est);
        d_conf.segments_reset = static_cast<uint32_t>(reset);
        d_conf.mode = lite ? GC_NOTCH_LITE : GC_NOTCH_FULL;
        d_conf.noise_floor = floor == "linear" ? GC_NOTCH_FLOOR_LINEAR : GC_NOTCH_FLOOR_REFERENCE;
        d_status = gc_stream_create(ctx, GC_IQ_F32, std::max<uint64_t>(ring_capacity, 2ull * max_window), max_window, &d_ring);
        if (d_status == GC_OK) d_status = gc_ring_notch_create(ctx, source, &d_conf, d_ring, &d_notch);
        if (d_status != GC_OK && d_ring)
            {
                gc_stream_destroy(d_ring);
                d_ring = nullptr;
            }
    }

private:
    gc_notch_conf d_conf = {};
    gc_stream* d_ring = nullptr;
    gc_ring_notch* d_notch = nullptr;
    gc_status d_status = GC_OK;
};

/*! Notch_Filter: a coefficient per sample.  ring_capacity / max_window: size of the derived ring and its longest window */
class hip_notch_filter : public hip_notch_filter_base
{
public:
    hip_notch_filter(gc_ctx* ctx, gc_stream* source, ConfigurationInterface* configuration, const std::string& role, uint64_t ring_capacity, uint32_t max_window)
        : hip_notch_filter_base(ctx, source, configuration, role, false, ring_capacity, max_window)
    {
    }
};

/*! Notch_Filter_Lite: a coefficient per segments_coeff filtered segments */
class hip_notch_filter_lite : public hip_notch_filter_base
{
public:
    hip_notch_filter_lite(gc_ctx* ctx, gc_stream* source, ConfigurationInterface* configuration, const std::string& role, uint64_t ring_capacity, uint32_t max_window)
        : hip_notch_filter_base(ctx, source, configuration, role, true, ring_capacity, max_window)
    {
    }
};

#endif  // GNSSCORR_HIP_NOTCH_FILTER_H_
