/*!
 * \file hip_tracking_group.h
 * \brief All tracking channels of one signal on one GPU as ONE object: the MI355X-native shape of the receiver's tracking stage.
 *
 * In the reference every channel is its own GNU Radio block reading the same RF stream (gnss_flowgraph.cc:496-499), and every block
 * runs its own loop one code period at a time.  Here the stream lives once in an HBM ring (gc_stream) and a group holds N channel
 * slots of a device loop (gc_trk_loop): start_tracking(ch, acquisition result) fills a slot the way
 * dll_pll_veml_tracking::start_tracking does, run() executes every code period that is complete in the ring for ALL active
 * channels in one launch and returns the Gnss_Synchro items per channel -- what N blocks of the reference would have written to
 * their N outputs.  Slots that are not tracking (never started, stopped, lost lock) cost nothing.  A hybrid receiver (e.g. GPS L1 C/A +
 * Galileo E1 + BeiDou B1I on one conditioner output) is ONE group over a list of (Dll_Pll_Conf, slots) entries: one mixed device loop
 * (gc_trk_loop_set_mixed) in which each slot range belongs to one signal, with its own tap count, pilot mode, replica and code period,
 * all in one launch on one stream.
 *
 * In a GNSS-SDR tree this is one gr::block with one input and N Gnss_Synchro outputs: general_work pushes the new items into the
 * ring, calls run() and copies each channel's items to its output (produce(ch, n)); the channel state machine calls
 * start_tracking / stop_tracking through N thin TrackingInterface adapters that hold (group, slot).
 *
 * start_tracking(ch, acq, start_index), stop_tracking(ch), run(out) and the slot accessors are hip_loop_group_base's
 * (tracking_block_base.h), under the veml policy; this class holds the signal list and what a start and a record mean for a slot.
 */
#ifndef GNSSCORR_HIP_TRACKING_GROUP_H_
#define GNSSCORR_HIP_TRACKING_GROUP_H_

#include "hip_dll_pll_veml_tracking_dev.h"
#include <memory>
#include <utility>
#include <vector>

class hip_tracking_group : public hip_loop_group_base
{
public:
    /*! ctx / ring: the GPU context and the RF stream the channels read; signals: one (Dll_Pll_Conf, slots) entry per signal -- the
     *  first entry owns slots [0, n_0), the next [n_0, n_0 + n_1), and so on; iq_format: the ring's sample format (GC_IQ_F32 gr_complex,
     *  GC_IQ_I16 cshort, GC_IQ_I8 cbyte -- integer samples are converted on load, the stream crosses PCIe and sits in HBM in its native
     *  size).  With more than one entry the device loop is a mixed engine; high_dyn must be the same for every entry. */
    hip_tracking_group(gc_ctx* ctx, gc_stream* ring, const std::vector<std::pair<Dll_Pll_Conf, int>>& signals, int iq_format = GC_IQ_F32)
        : hip_loop_group_base(gnsscorr::kVemlLoopPolicy, ring)
    {
        int max_code_len = 0;
        for (const auto& e : signals)
            {
                Signal sg;
                sg.conf = e.first;
                sg.sig = gnsscorr::trk_signal_find(sg.conf.system, std::string(sg.conf.signal));
                if (e.second <= 0 || sg.sig == nullptr)
                    {
                        d_status = GC_ERR_INVALID;
                        return;
                    }
                if (!sg.sig->has_pilot) sg.conf.track_pilot = false;
                sg.interchange_iq = sg.conf.track_pilot && sg.sig->interchange_iq_with_pilot;
                max_code_len = std::max(max_code_len, static_cast<int>(sg.sig->code_length_chips * sg.sig->code_samples_per_chip));
                for (int k = 0; k < e.second; k++) d_slot_signal.push_back(static_cast<int>(d_signals.size()));
                d_n += e.second;
                d_signals.push_back(sg);
            }
        if (d_n == 0)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        create_loop(ctx, max_code_len, iq_format, d_signals.size() > 1);
    }
    /*! One signal: conf is the Dll_Pll_Conf every channel of the group shares (signal, loop settings); n_channels: slots */
    hip_tracking_group(gc_ctx* ctx, gc_stream* ring, const Dll_Pll_Conf& conf, int n_channels, int iq_format = GC_IQ_F32)
        : hip_tracking_group(ctx, ring, std::vector<std::pair<Dll_Pll_Conf, int>>{{conf, n_channels}}, iq_format)
    {
    }

    //! the reference waits 10 s before looking for the telemetry preamble (dll_pll_veml_tracking.cc:1648); tests shorten it
    void set_bit_sync_min_time_s(float t) { d_bit_sync_min_time_s = t; }
    //! index (in the constructor's list) of the signal slot `ch` belongs to
    int signal_of(int ch) const { return d_slot_signal[ch]; }

protected:
    //! fills the slot the way dll_pll_veml_tracking::start_tracking does
    gc_status start_slot(int ch, const Gnss_Synchro& acq, uint64_t start_index, Gnss_Synchro*) override
    {
        const Signal& sg = signal(ch);
        return gnsscorr::loop_start_channel(d_loop, ch, sg.conf, *sg.sig, acq, start_index, d_bit_sync_min_time_s);
    }
    uint32_t vector_length_of(int ch) const override { return signal(ch).conf.vector_length; }
    Gnss_Synchro to_synchro(int ch, const gc_loop_record& r) const override
    {
        const Signal& sg = signal(ch);
        return gnsscorr::synchro_from_record(r, d_acq[ch], *sg.sig, sg.interchange_iq, sg.conf.fs_in);
    }

private:
    // per signal of the group: its Dll_Pll_Conf (track_pilot cleared where the signal has no pilot), its row of the signal table, and
    // whether the pilot's prompt is reported with I and Q interchanged
    struct Signal
    {
        Dll_Pll_Conf conf;
        const gnsscorr::TrkSignalInfo* sig = nullptr;
        bool interchange_iq = false;
    };
    const Signal& signal(int ch) const { return d_signals[d_slot_signal[ch]]; }

    std::vector<Signal> d_signals;
    std::vector<int> d_slot_signal;  // per slot: index into d_signals
    float d_bit_sync_min_time_s = 10.0f;
};

#endif  // GNSSCORR_HIP_TRACKING_GROUP_H_
