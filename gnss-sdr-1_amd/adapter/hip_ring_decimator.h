/*!
 * \file hip_ring_decimator.h
 * \brief The acquisition resampler of one signal on the GPU: a decimating low-pass FIR from the RF stream ring into a derived ring
 * that the acquisition searches at a fraction of the channels' rate, while tracking stays on the full-rate ring.
 *
 * With GNSS-SDR.use_acquisition_resampler=true the reference connects one fir_filter_ccf per signal between the signal conditioner
 * and the acquisition blocks (gnss_flowgraph.cc:375-499): decimation = floor(fs / opt_acq_fs) stepped down to a divisor of fs, taps
 * from firdes::low_pass(1.0, fs, acq_fs / 2.1, acq_fs / 10), and set_resampler_latency((taps - 1) / 2) on the acquisition.  This class
 * is that block: it plans with gc_acq_resampler_plan (the same rule, plus the library's limits D <= 64, T <= 1024), owns a ring
 * at resampled_fs() -- gr_complex, or what the keys <role>.output_item_type ("gr_complex" | "cshort" | "cbyte") and <role>.output_scale
 * (default 1; 127 for "cbyte" when the key is absent) of the second constructor ask for, with hip_signal_conditioner's meaning -- and the device decimator (gc_ring_decimator) that writes it from `source`, and update() appends what the
 * source's samples so far complete.  Derived sample m is source sample m * decimation(), delayed by latency() source samples.
 * Deviation: the reference switches the resampler off for item types other than gr_complex; this one reads every ring format.
 * enabled() is false -- and nothing is allocated -- when the plan's decimation is 1 ("Disabled acquisition resampler because the input
 * sampling frequency is too low").
 */
#ifndef GNSSCORR_HIP_RING_DECIMATOR_H_
#define GNSSCORR_HIP_RING_DECIMATOR_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include <algorithm>
#include <string>
#include <vector>

class hip_ring_decimator
{
public:
    /*! fs_in: rate of `source`; opt_acq_fs_hz: the signal's optimal search rate (0: none).  The derived ring is created by open(). */
    hip_ring_decimator(gc_ctx* ctx, gc_stream* source, int64_t fs_in, uint32_t opt_acq_fs_hz) : d_ctx(ctx), d_source(source), d_resampled_fs(fs_in)
    {
        if (opt_acq_fs_hz == 0) return;
        int n = 0;
        d_status = gc_acq_resampler_plan(fs_in, opt_acq_fs_hz, &d_decimation, &d_resampled_fs, nullptr, 0, &n, &d_latency);
        if (d_status != GC_OK || d_decimation <= 1) return;
        d_taps.assign(static_cast<size_t>(n), 0.0f);
        d_status = gc_acq_resampler_plan(fs_in, opt_acq_fs_hz, &d_decimation, &d_resampled_fs, d_taps.data(), n, &n, &d_latency);
    }
    /*! The same with the derived ring's item type and scale taken from the configuration under `role`. */
    hip_ring_decimator(gc_ctx* ctx, gc_stream* source, int64_t fs_in, uint32_t opt_acq_fs_hz, ConfigurationInterface* configuration, const std::string& role)
        : hip_ring_decimator(ctx, source, fs_in, opt_acq_fs_hz)
    {
        const std::string type = configuration->property(role + ".output_item_type", std::string("gr_complex"));
        if (!gnsscorr_iq_format(type, &d_out_format))
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        d_out_scale = configuration->property(role + ".output_scale", d_out_format == GC_IQ_I8 ? 127.0f : 1.0f);
    }
    ~hip_ring_decimator()
    {
        if (d_decim) gc_ring_decimator_destroy(d_decim);
        if (d_ring) gc_stream_destroy(d_ring);
    }
    hip_ring_decimator(const hip_ring_decimator&) = delete;
    hip_ring_decimator& operator=(const hip_ring_decimator&) = delete;

    //! the plan found a decimation above 1
    bool enabled() const { return d_status == GC_OK && d_decimation > 1; }
    /*! Creates the derived ring (capacity / max_window in DERIVED samples; the capacity is raised to what the source ring holds,
     *  divided by the decimation) and the decimator. */
    gc_status open(uint64_t ring_capacity, uint32_t max_window)
    {
        if (!enabled()) return d_status;
        uint64_t src_cap = 0;
        d_status = gc_stream_info(d_source, nullptr, nullptr, &src_cap);
        if (d_status != GC_OK) return d_status;
        const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(ring_capacity, 2ull * max_window), src_cap / d_decimation + 1);
        d_status = gc_stream_create(d_ctx, d_out_format, cap, max_window, &d_ring);
        if (d_status == GC_OK && d_out_format != GC_IQ_F32) d_status = gc_stream_accept_quantised_output(d_ring);
        if (d_status == GC_OK)
            d_status = gc_ring_decimator_create(d_ctx, d_source, d_decimation, d_taps.data(), static_cast<uint32_t>(d_taps.size()), d_ring, &d_decim);
        if (d_status == GC_OK && d_out_format != GC_IQ_F32) d_status = gc_ring_decimator_set_output_scale(d_decim, d_out_scale);
        return d_status;
    }
    //! appends the outputs the source's samples so far complete (asynchronous)
    gc_status update(uint64_t* first_out = nullptr, uint64_t* n_out = nullptr)
    {
        if (d_decim == nullptr) return d_status;
        d_status = gc_ring_decimator_update(d_decim, first_out, n_out);
        return d_status;
    }
    //! the derived ring: pass it to the acquisition together with resampled_fs()
    gc_stream* ring() const { return d_ring; }
    uint32_t decimation() const { return d_decimation; }
    int64_t resampled_fs() const { return d_resampled_fs; }
    //! acq_parameters.resampler_latency_samples: (taps - 1) / 2 source samples
    uint32_t latency() const { return d_latency; }
    const std::vector<float>& taps() const { return d_taps; }
    //! derived samples made so far (the derived ring's head)
    uint64_t head() const
    {
        uint64_t h = 0;
        if (d_decim) gc_ring_decimator_info(d_decim, nullptr, &h);
        return h;
    }
    //! gc_iq_format of the derived ring and the factor in front of its clamp (1 for gr_complex)
    int output_format() const { return d_out_format; }
    float output_scale() const { return d_out_format == GC_IQ_F32 ? 1.0f : d_out_scale; }
    //! components of a cshort / cbyte ring that hit the clamp so far (0 for gr_complex); waits for the updates so far
    uint64_t clipped_components() const
    {
        uint64_t n = 0;
        if (d_decim) gc_ring_decimator_output_info(d_decim, nullptr, nullptr, &n);
        return n;
    }
    gc_status last_status() const { return d_status; }

private:
    gc_ctx* d_ctx;
    gc_stream* d_source;
    uint32_t d_decimation = 1, d_latency = 0;
    int64_t d_resampled_fs;
    std::vector<float> d_taps;
    gc_stream* d_ring = nullptr;
    gc_ring_decimator* d_decim = nullptr;
    gc_status d_status = GC_OK;
    int d_out_format = GC_IQ_F32;
    float d_out_scale = 1.0f;
};

#endif  // GNSSCORR_HIP_RING_DECIMATOR_H_
