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
 * In a GNSS-SDR tree this is one gr::block with one input and N Gnss_Synchro outputs: general_work pushes the new items
 * (gc_stream_push), calls run() and copies each channel's items to its output (produce(ch, n)); the channel state machine calls
 * start_tracking / stop_tracking through N thin TrackingInterface adapters that hold (group, slot).
 */
#ifndef GNSSCORR_HIP_TRACKING_GROUP_H_
#define GNSSCORR_HIP_TRACKING_GROUP_H_

#include "hip_dll_pll_veml_tracking_dev.h"
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

class hip_tracking_group
{
public:
    /*! ctx / ring: the GPU context and the RF stream the channels read; signals: one (Dll_Pll_Conf, slots) entry per signal -- the
     *  first entry owns slots [0, n_0), the next [n_0, n_0 + n_1), and so on; iq_format: the ring's sample format (GC_IQ_F32 gr_complex,
     *  GC_IQ_I16 cshort, GC_IQ_I8 cbyte -- integer samples are converted on load, the stream crosses PCIe and sits in HBM in its native
     *  size).  With more than one entry the device loop is a mixed engine; high_dyn must be the same for every entry. */
    hip_tracking_group(gc_ctx* ctx, gc_stream* ring, const std::vector<std::pair<Dll_Pll_Conf, int>>& signals, int iq_format = GC_IQ_F32)
        : d_ring(ring)
    {
        d_n = 0;
        int max_code_len = 0;
        for (const auto& e : signals)
            {
                Signal sg;
                sg.conf = e.first;
                if (e.second <= 0 || !gnsscorr::trk_signal_constants(sg.conf.system, std::string(sg.conf.signal), &sg.sig))
                    {
                        d_status = GC_ERR_INVALID;
                        return;
                    }
                if (!sg.sig.has_pilot) sg.conf.track_pilot = false;
                sg.interchange_iq = sg.conf.track_pilot && sg.sig.interchange_iq_with_pilot;
                max_code_len = std::max(max_code_len, static_cast<int>(sg.sig.code_length_chips * sg.sig.code_samples_per_chip));
                for (int k = 0; k < e.second; k++) d_slot_signal.push_back(static_cast<int>(d_signals.size()));
                d_n += e.second;
                d_signals.push_back(sg);
            }
        if (d_n == 0)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        d_status = gc_trk_loop_create(ctx, d_n, max_code_len, &d_loop);
        if (d_status == GC_OK && d_signals.size() > 1) d_status = gc_trk_loop_set_mixed(d_loop, 1);
        if (d_status == GC_OK) d_status = gc_trk_loop_set_input_format(d_loop, iq_format);
        for (int ch = 0; ch < d_n && d_status == GC_OK; ch++) d_status = gc_trk_loop_set_input_stream(d_loop, ch, ring);
        d_acq.resize(d_n);
        d_active.assign(d_n, 0);
        d_position.assign(d_n, 0);
        d_events.resize(d_n);
    }
    /*! One signal: conf is the Dll_Pll_Conf every channel of the group shares (signal, loop settings); n_channels: slots */
    hip_tracking_group(gc_ctx* ctx, gc_stream* ring, const Dll_Pll_Conf& conf, int n_channels, int iq_format = GC_IQ_F32)
        : hip_tracking_group(ctx, ring, std::vector<std::pair<Dll_Pll_Conf, int>>{{conf, n_channels}}, iq_format)
    {
    }
    ~hip_tracking_group()
    {
        if (d_loop) gc_trk_loop_destroy(d_loop);
    }
    hip_tracking_group(const hip_tracking_group&) = delete;
    hip_tracking_group& operator=(const hip_tracking_group&) = delete;

    //! the reference waits 10 s before looking for the telemetry preamble (dll_pll_veml_tracking.cc:1648); tests shorten it
    void set_bit_sync_min_time_s(float t) { d_bit_sync_min_time_s = t; }

    /*! Channel slot `ch` starts tracking the satellite of `acq` (PRN, Acq_delay_samples, Acq_doppler_hz, Acq_samplestamp_samples) at
     *  stream sample `start_index` -- any resident sample; the pull-in aligns the first code period after it. */
    gc_status start_tracking(int ch, const Gnss_Synchro& acq, uint64_t start_index)
    {
        std::lock_guard<std::mutex> l(d_mutex);
        if (d_loop == nullptr) return d_status;  // construction failed
        if (ch < 0 || ch >= d_n) return GC_ERR_INVALID;
        if (d_active[ch]) gc_trk_loop_stop(d_loop, ch);
        const Signal& sg = d_signals[d_slot_signal[ch]];
        gc_status st = gnsscorr::loop_start_channel(d_loop, ch, sg.conf, sg.sig, acq, start_index, d_bit_sync_min_time_s);
        if (st != GC_OK) return st;
        d_acq[ch] = acq;
        d_active[ch] = 1;
        d_position[ch] = start_index;
        return GC_OK;
    }

    gc_status stop_tracking(int ch)
    {
        std::lock_guard<std::mutex> l(d_mutex);
        if (ch < 0 || ch >= d_n) return GC_ERR_INVALID;
        d_active[ch] = 0;
        return gc_trk_loop_stop(d_loop, ch);
    }

    /*! Every complete code period of every active channel, one launch; out[ch] receives the channel's Gnss_Synchro items (appended).
     *  Returns the number of items produced over all channels, or -1 (last_status()). */
    int run(std::vector<std::vector<Gnss_Synchro>>& out)
    {
        std::lock_guard<std::mutex> l(d_mutex);
        if (d_loop == nullptr) return -1;  // construction failed; a failed run() is NOT sticky: the next call tries again
        out.resize(d_n);
        uint64_t head = 0;
        gc_stream_info(d_ring, nullptr, &head, nullptr);
        int n_periods = 0;
        bool any = false;
        for (int ch = 0; ch < d_n; ch++)
            if (d_active[ch])
                {
                    any = true;
                    // each slot's own code period: a mixed group sizes the launch for its shortest one
                    const uint32_t vlen = d_signals[d_slot_signal[ch]].conf.vector_length;
                    if (head > d_position[ch]) n_periods = std::max<int>(n_periods, static_cast<int>((head - d_position[ch]) / vlen) + 1);
                }
        if (!any || n_periods == 0) return 0;
        d_records.resize(static_cast<size_t>(d_n) * n_periods);
        d_status = gc_trk_loop_run(d_loop, n_periods, d_records.data());
        if (d_status != GC_OK)
            {
                // e.g. a channel that was not serviced in time fell behind the ring (GC_ERR_STATE): the caller parks that channel
                // (stop_tracking / a new start_tracking) and goes on; the other channels are unaffected
                return -1;
            }
        int produced = 0;
        for (int ch = 0; ch < d_n; ch++)
            {
                if (!d_active[ch]) continue;
                const Signal& sg = d_signals[d_slot_signal[ch]];
                uint64_t position = d_position[ch];
                for (int k = 0; k < n_periods; k++)
                    {
                        const gc_loop_record& r = d_records[static_cast<size_t>(ch) * n_periods + k];
                        if (r.sample_counter == position && r.valid == 0 && r.state >= 2) break;  // out of input
                        position = r.sample_counter;
                        if (r.valid)
                            {
                                out[ch].push_back(gnsscorr::synchro_from_record(r, d_acq[ch], sg.sig, sg.interchange_iq, sg.conf.fs_in));
                                produced++;
                            }
                        if (r.state == 0)
                            {
                                d_events[ch].push_back(3);  // loss of lock: the slot is free for the next acquisition
                                d_active[ch] = 0;
                                break;
                            }
                    }
                d_position[ch] = position;
            }
        return produced;
    }

    int n_channels() const { return d_n; }
    //! index (in the constructor's list) of the signal slot `ch` belongs to
    int signal_of(int ch) const { return d_slot_signal[ch]; }
    bool active(int ch) const { return d_active[ch] != 0; }
    //! stream sample up to which channel `ch` has consumed (a producer may evict everything before the minimum over the channels)
    uint64_t position(int ch) const { return d_position[ch]; }
    const std::vector<int>& events(int ch) const { return d_events[ch]; }
    gc_status last_status() const { return d_status; }

private:
    // per signal of the group: its Dll_Pll_Conf (track_pilot cleared where the signal has no pilot), the constants of the block's
    // constructor, and whether the pilot's prompt is reported with I and Q interchanged
    struct Signal
    {
        Dll_Pll_Conf conf;
        gnsscorr::TrkSignalConstants sig{};
        bool interchange_iq = false;
    };
    std::vector<Signal> d_signals;
    std::vector<int> d_slot_signal;  // per slot: index into d_signals
    gc_stream* d_ring;
    gc_trk_loop* d_loop = nullptr;
    int d_n = 0;
    float d_bit_sync_min_time_s = 10.0f;
    gc_status d_status = GC_OK;
    std::mutex d_mutex;
    std::vector<Gnss_Synchro> d_acq;
    std::vector<char> d_active;
    std::vector<uint64_t> d_position;
    std::vector<std::vector<int>> d_events;
    std::vector<gc_loop_record> d_records;
};

#endif  // GNSSCORR_HIP_TRACKING_GROUP_H_
