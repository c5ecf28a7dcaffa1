/*!
 * \file hip_glonass_tracking_group.h
 * \brief N GLONASS C/A channel slots of ONE band on one RF stream ring as one object: the GLONASS counterpart of
 * hip_tracking_group.  The FDMA satellites of a band share one conditioner output; every slot runs the GLONASS block's own loop
 * (gc_trk_loop_start_glonass) with the frequency channel of its satellite, and run() executes every code period that is complete
 * in the ring for ALL active slots in one launch.  A GLONASS engine holds GLONASS slots only (its loop is not the veml loop), so
 * a four-constellation receiver runs one hip_glonass_tracking_group per band beside its hip_tracking_group.
 *
 * start_tracking(ch, acquisition result, start index), stop_tracking(ch) and run(out) behave as in hip_tracking_group; out[ch]
 * receives the item of the pull-in alignment first (what the block writes when it aligns to the code), then one Gnss_Synchro per
 * valid period -- what N blocks of the reference would have written to their N outputs.
 */
#ifndef GNSSCORR_HIP_GLONASS_TRACKING_GROUP_H_
#define GNSSCORR_HIP_GLONASS_TRACKING_GROUP_H_

#include "hip_glonass_ca_dll_pll_tracking_dev.h"
#include <mutex>
#include <vector>

class hip_glonass_tracking_group
{
public:
    /*! ctx / ring: the GPU context and the RF stream the slots read (two block lengths must fit its max_window); conf: band, sampling
     *  rate and loop settings every slot shares; iq_format: the ring's sample format */
    hip_glonass_tracking_group(gc_ctx* ctx, gc_stream* ring, const gnsscorr::GlonassTrkConf& conf, int n_channels, int iq_format = GC_IQ_F32)
        : d_conf(conf), d_ring(ring), d_n(n_channels), d_glonass_prn(gnsscorr::glonass_default_channels())
    {
        if (n_channels <= 0)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        d_status = gc_trk_loop_create(ctx, d_n, 511, &d_loop);
        if (d_status == GC_OK) d_status = gc_trk_loop_set_input_format(d_loop, iq_format);
        for (int ch = 0; ch < d_n && d_status == GC_OK; ch++) d_status = gc_trk_loop_set_input_stream(d_loop, ch, ring);
        d_acq.resize(d_n);
        d_pull_in_item.resize(d_n);
        d_pull_in.assign(d_n, 0);
        d_active.assign(d_n, 0);
        d_position.assign(d_n, 0);
        d_events.resize(d_n);
    }
    ~hip_glonass_tracking_group()
    {
        if (d_loop) gc_trk_loop_destroy(d_loop);
    }
    hip_glonass_tracking_group(const hip_glonass_tracking_group&) = delete;
    hip_glonass_tracking_group& operator=(const hip_glonass_tracking_group&) = delete;

    //! the slot -> frequency channel map comes from the almanac in a live receiver
    void set_glonass_channel_map(const std::map<uint32_t, int32_t>& prn_to_channel) { d_glonass_prn = prn_to_channel; }

    /*! Channel slot `ch` starts tracking the satellite of `acq` (PRN -> frequency channel, Acq_delay_samples, Acq_doppler_hz,
     *  Acq_samplestamp_samples) at stream sample `start_index` -- any resident sample; the pull-in aligns the first code period after it. */
    gc_status start_tracking(int ch, const Gnss_Synchro& acq, uint64_t start_index)
    {
        std::lock_guard<std::mutex> l(d_mutex);
        if (d_loop == nullptr) return d_status;  // construction failed
        if (ch < 0 || ch >= d_n) return GC_ERR_INVALID;
        if (d_active[ch]) gc_trk_loop_stop(d_loop, ch);
        d_active[ch] = 0;
        const gc_status st = gnsscorr::glonass_loop_start_channel(d_loop, ch, d_conf, d_glonass_prn, acq, start_index, &d_pull_in_item[ch]);
        if (st != GC_OK) return st;
        d_acq[ch] = acq;
        d_active[ch] = 1;
        d_pull_in[ch] = 1;
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

    /*! Every complete code period of every active slot, one launch; out[ch] receives the slot's Gnss_Synchro items (appended).
     *  Returns the number of items produced over all slots, or -1 (last_status()). */
    int run(std::vector<std::vector<Gnss_Synchro>>& out)
    {
        std::lock_guard<std::mutex> l(d_mutex);
        if (d_loop == nullptr) return -1;  // construction failed; a failed run() is NOT sticky: the next call tries again
        out.resize(d_n);
        uint64_t head = 0;
        gc_stream_info(d_ring, nullptr, &head, nullptr);
        int n_periods = 0, produced = 0;
        bool any = false;
        for (int ch = 0; ch < d_n; ch++)
            if (d_active[ch])
                {
                    any = true;
                    if (d_pull_in[ch])
                        {
                            out[ch].push_back(d_pull_in_item[ch]);
                            d_pull_in[ch] = 0;
                            produced++;
                        }
                    if (head > d_position[ch]) n_periods = std::max<int>(n_periods, static_cast<int>((head - d_position[ch]) / d_conf.vector_length) + 1);
                }
        if (!any || n_periods == 0) return produced;
        d_records.resize(static_cast<size_t>(d_n) * n_periods);
        d_status = gc_trk_loop_run(d_loop, n_periods, d_records.data());
        if (d_status != GC_OK) return -1;  // e.g. a slot that was not serviced in time fell behind the ring: the caller parks it
        for (int ch = 0; ch < d_n; ch++)
            {
                if (!d_active[ch]) continue;
                uint64_t position = d_position[ch];
                for (int k = 0; k < n_periods; k++)
                    {
                        const gc_loop_record& r = d_records[static_cast<size_t>(ch) * n_periods + k];
                        if (r.valid == 0) break;  // out of input
                        position = r.sample_counter;
                        out[ch].push_back(gnsscorr::glonass_synchro_from_record(r, d_acq[ch], d_conf.fs_in));
                        produced++;
                        if (r.state == 0)
                            {
                                d_events[ch].push_back(3);  // loss of lock: the slot is free for the next acquisition
                                d_active[ch] = 0;
                                gc_trk_loop_stop(d_loop, ch);
                                break;
                            }
                    }
                d_position[ch] = position;
            }
        return produced;
    }

    int n_channels() const { return d_n; }
    bool active(int ch) const { return d_active[ch] != 0; }
    //! stream sample up to which slot `ch` has consumed (a producer may evict everything before the minimum over the slots)
    uint64_t position(int ch) const { return d_position[ch]; }
    const std::vector<int>& events(int ch) const { return d_events[ch]; }
    gc_status last_status() const { return d_status; }

private:
    gnsscorr::GlonassTrkConf d_conf;
    gc_stream* d_ring;
    gc_trk_loop* d_loop = nullptr;
    int d_n = 0;
    std::map<uint32_t, int32_t> d_glonass_prn;
    gc_status d_status = GC_OK;
    std::mutex d_mutex;
    std::vector<Gnss_Synchro> d_acq, d_pull_in_item;
    std::vector<char> d_pull_in, d_active;
    std::vector<uint64_t> d_position;
    std::vector<std::vector<int>> d_events;
    std::vector<gc_loop_record> d_records;
};

#endif  // GNSSCORR_HIP_GLONASS_TRACKING_GROUP_H_
