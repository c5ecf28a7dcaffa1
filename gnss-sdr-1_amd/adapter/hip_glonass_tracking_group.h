/*!
 * \file hip_glonass_tracking_group.h
 * \brief N GLONASS C/A channel slots of ONE band on one RF stream ring as one object: the GLONASS counterpart of
 * hip_tracking_group.  The FDMA satellites of a band share one conditioner output; every slot runs the GLONASS block's own loop
 * (gc_trk_loop_start_glonass) with the frequency channel of its satellite, and run() executes every code period that is complete
 * in the ring for ALL active slots in one launch.  A GLONASS engine holds GLONASS slots only (its loop is not the veml loop), so
 * a four-constellation receiver runs one hip_glonass_tracking_group per band beside its hip_tracking_group.
 *
 * start_tracking(ch, acquisition result, start index), stop_tracking(ch) and run(out) are hip_loop_group_base's
 * (tracking_block_base.h), as in hip_tracking_group, here under the GLONASS policy; out[ch]
 * receives the item of the pull-in alignment first (what the block writes when it aligns to the code), then one Gnss_Synchro per
 * valid period -- what N blocks of the reference would have written to their N outputs.
 */
#ifndef GNSSCORR_HIP_GLONASS_TRACKING_GROUP_H_
#define GNSSCORR_HIP_GLONASS_TRACKING_GROUP_H_

#include "hip_glonass_ca_dll_pll_tracking_dev.h"
#include <vector>

class hip_glonass_tracking_group : public hip_loop_group_base
{
public:
    /*! ctx / ring: the GPU context and the RF stream the slots read (two block lengths must fit its max_window); conf: band, sampling
     *  rate and loop settings every slot shares; iq_format: the ring's sample format */
    hip_glonass_tracking_group(gc_ctx* ctx, gc_stream* ring, const gnsscorr::GlonassTrkConf& conf, int n_channels, int iq_format = GC_IQ_F32)
        : hip_loop_group_base(gnsscorr::kGlonassLoopPolicy, ring), d_conf(conf), d_glonass_prn(gnsscorr::glonass_default_channels())
    {
        d_n = n_channels;
        if (n_channels <= 0)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        create_loop(ctx, gnsscorr::kGlonassCaCodeLengthChips, iq_format, false);
    }

    //! the slot -> frequency channel map comes from the almanac in a live receiver
    void set_glonass_channel_map(const std::map<uint32_t, int32_t>& prn_to_channel) { d_glonass_prn = prn_to_channel; }

protected:
    //! PRN -> frequency channel; a PRN that is not in the map is GC_ERR_INVALID
    gc_status start_slot(int ch, const Gnss_Synchro& acq, uint64_t start_index, Gnss_Synchro* pull_in) override
    {
        return gnsscorr::glonass_loop_start_channel(d_loop, ch, d_conf, d_glonass_prn, acq, start_index, pull_in);
    }
    uint32_t vector_length_of(int) const override { return d_conf.vector_length; }
    Gnss_Synchro to_synchro(int ch, const gc_loop_record& r) const override { return gnsscorr::glonass_synchro_from_record(r, d_acq[ch], d_conf.fs_in); }

private:
    gnsscorr::GlonassTrkConf d_conf;
    std::map<uint32_t, int32_t> d_glonass_prn;
};

#endif  // GNSSCORR_HIP_GLONASS_TRACKING_GROUP_H_
