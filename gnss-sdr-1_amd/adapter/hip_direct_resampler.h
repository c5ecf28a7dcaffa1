/*!
 * \file hip_direct_resampler.h
 * \brief The resampler of a signal conditioner on the GPU: a ring derived from another ring at an arbitrary rate ratio.
 *
 * The reference's signal conditioner is data_type_adapter -> input_filter -> resampler, and its resampler adapter is Direct_Resampler
 * (src/algorithms/resampler/adapters/direct_resampler_conditioner.cc; blocks direct_resampler_conditioner_{cc,cs,cb}.cc): nearest
 * earlier sample, no filter.  This class takes that adapter's configuration keys under its role --
 *   sample_freq_in     [Hz]  rate of the source ring                                (default 4000000)
 *   sample_freq_out    [Hz]  rate of the derived ring                               (default 2048000)
 *   item_type                "gr_complex" | "cshort" | "cbyte": the format of both rings in direct mode, GC_IQ_F32 / GC_IQ_I16 /
 *                            GC_IQ_I8 (default "gr_complex"); it must be the source ring's
 * -- and two of this library:
 *   resampler_mode           "direct" (default): the reference's block, the same picks (gnsscorr.h, GC_RESAMP_DIRECT);
 *                            "polyphase": band-limited, a bank from gc_resampler_design; the derived ring is gr_complex whatever
 *                            item_type says about the source (GC_RESAMP_POLYPHASE; not bit compatible with the reference's
 *                            Mmse_Resampler)
 *   phases                   P of polyphase mode, a power of two in 1..256           (default 32)
 * -- owns the derived ring and the device resampler (gc_ring_resampler) that writes it from `source`, and update() appends what
 * the source's samples so far complete.  `source` is any ring: pushed from the host, or hip_signal_conditioner::ring(), so the block
 * chains behind the input filter as in the reference.  Polyphase mode delays the signal by group_delay_samples() SOURCE samples; as
 * everywhere in the library, that is left in the observables.
 */
#ifndef GNSSCORR_HIP_DIRECT_RESAMPLER_H_
#define GNSSCORR_HIP_DIRECT_RESAMPLER_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include <algorithm>
#include <string>
#include <vector>

class hip_direct_resampler
{
public:
    /*! ring_capacity / max_window: size of the derived ring and its longest window, in DERIVED samples (gc_stream_create) */
    hip_direct_resampler(gc_ctx* ctx, gc_stream* source, ConfigurationInterface* configuration, const std::string& role, uint64_t ring_capacity,
        uint32_t max_window)
    {
        d_fs_in = configuration->property(role + ".sample_freq_in", 4000000.0);
        d_fs_out = configuration->property(role + ".sample_freq_out", 2048000.0);
        d_item_type = configuration->property(role + ".item_type", std::string("gr_complex"));
        const std::string mode = configuration->property(role + ".resampler_mode", std::string("direct"));
        const int32_t phases = configuration->property(role + ".phases", static_cast<int32_t>(32));
        int format = GC_IQ_F32;
        if (!gnsscorr_iq_format(d_item_type, &format))
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        if ((mode != "direct" && mode != "polyphase") || phases < 1)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        d_polyphase = mode == "polyphase";
        gc_resampler_conf c;
        c.fs_in = d_fs_in;
        c.fs_out = d_fs_out;
        c.mode = d_polyphase ? GC_RESAMP_POLYPHASE : GC_RESAMP_DIRECT;
        c.phases = 0;
        c.taps_per_phase = 0;
        c.reserved = 0;
        c.bank = nullptr;
        if (d_polyphase)
            {
                int T = 0;
                d_status = gc_resampler_design(d_fs_in, d_fs_out, static_cast<uint32_t>(phases), nullptr, 0, &T);
                if (d_status != GC_OK) return;
                d_bank.assign(static_cast<size_t>(phases) * static_cast<size_t>(T), 0.0f);
                d_status = gc_resampler_design(d_fs_in, d_fs_out, static_cast<uint32_t>(phases), d_bank.data(), static_cast<int>(d_bank.size()), &T);
                if (d_status != GC_OK) return;
                // the prototype's length, for the group delay: the same call gc_resampler_design makes
                const double low = std::min(d_fs_in, d_fs_out);
                int n = 0;
                d_status = gc_fir_low_pass(static_cast<double>(phases), phases * d_fs_in, low / 2.1, low / 10.0, nullptr, 0, &n);
                if (d_status != GC_OK) return;
                d_group_delay = static_cast<double>(n - 1) / (2.0 * phases);
                c.phases = static_cast<uint32_t>(phases);
                c.taps_per_phase = static_cast<uint32_t>(T);
                c.bank = d_bank.data();
                format = GC_IQ_F32;
            }
        d_out_format = format;
        d_status = gc_stream_create(ctx, format, std::max<uint64_t>(ring_capacity, 2ull * max_window), max_window, &d_ring);
        if (d_status == GC_OK) d_status = gc_ring_resampler_create(ctx, source, &c, d_ring, &d_resampler);
    }
    ~hip_direct_resampler()
    {
        if (d_resampler) gc_ring_resampler_destroy(d_resampler);
        if (d_ring) gc_stream_destroy(d_ring);
    }
    hip_direct_resampler(const hip_direct_resampler&) = delete;
    hip_direct_resampler& operator=(const hip_direct_resampler&) = delete;

    //! appends the outputs the source's samples so far complete (asynchronous)
    gc_status update(uint64_t* first_out = nullptr, uint64_t* n_out = nullptr)
    {
        if (d_resampler == nullptr) return d_status;
        d_status = gc_ring_resampler_update(d_resampler, first_out, n_out);
        return d_status;
    }
    //! the derived ring: pass it to the acquisition bank and the tracking group together with sample_freq_out()
    gc_stream* ring() const { return d_ring; }
    double sample_freq_in() const { return d_fs_in; }
    double sample_freq_out() const { return d_fs_out; }
    bool polyphase() const { return d_polyphase; }
    //! gc_iq_format of the derived ring
    int output_format() const { return d_out_format; }
    //! polyphase mode: the bank (phases rows of taps_per_phase() floats); empty in direct mode
    const std::vector<float>& bank() const { return d_bank; }
    //! delay of the polyphase filter in SOURCE samples, (prototype taps - 1) / (2 phases); 0 in direct mode
    double group_delay_samples() const { return d_group_delay; }
    //! derived samples made so far (the derived ring's head)
    uint64_t head() const
    {
        uint64_t h = 0;
        if (d_resampler) gc_ring_resampler_info(d_resampler, nullptr, &h);
        return h;
    }
    gc_status last_status() const { return d_status; }

private:
    double d_fs_in = 0.0, d_fs_out = 0.0, d_group_delay = 0.0;
    std::string d_item_type;
    bool d_polyphase = false;
    int d_out_format = GC_IQ_F32;
    std::vector<float> d_bank;
    gc_stream* d_ring = nullptr;
    gc_ring_resampler* d_resampler = nullptr;
    gc_status d_status = GC_OK;
};

#endif  // GNSSCORR_HIP_DIRECT_RESAMPLER_H_
