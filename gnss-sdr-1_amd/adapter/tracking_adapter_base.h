/*!
 * \file tracking_adapter_base.h
 * \brief What the TrackingInterface adapters of this directory share: TrackingAdapterRole with the role, the stream counts and the
 * sampling-rate look-up, and TrackingAdapterBase<Block> with the block and the overrides that only forward to it.  A concrete
 * adapter holds its constructor (keys, defaults, derived sizes) and implementation(); an adapter that picks one of two blocks
 * (the carrier-aided one) derives from TrackingAdapterRole and forwards itself.
 */
#ifndef GNSSCORR_TRACKING_ADAPTER_BASE_H_
#define GNSSCORR_TRACKING_ADAPTER_BASE_H_

#include "gnss_sdr_types.h"
#include <memory>
#include <string>

class TrackingAdapterRole : public TrackingInterface
{
public:
    std::string role() override { return role_; }

protected:
    TrackingAdapterRole(const std::string& role, unsigned int in_streams, unsigned int out_streams) : role_(role), in_streams_(in_streams), out_streams_(out_streams) {}

    //! the receiver's sampling rate, else the deprecated key that one replaced, else 2048000
    static int read_fs(ConfigurationInterface* configuration)
    {
        int fs_in_deprecated = configuration->property("GNSS-SDR.internal_fs_hz", 2048000);
        return configuration->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
    }

    std::string role_;
    unsigned int in_streams_, out_streams_;
    unsigned int channel_ = 0;
};

template <class Block>
class TrackingAdapterBase : public TrackingAdapterRole
{
public:
    size_t item_size() override { return sizeof(gr_complex); }
    void start_tracking() override { tracking_->start_tracking(); }
    void stop_tracking() override { tracking_->stop_tracking(); }
    void set_channel(unsigned int channel) override
    {
        channel_ = channel;
        tracking_->set_channel(channel);
    }
    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) override { tracking_->set_gnss_synchro(p_gnss_synchro); }

    //! the block (get_left_block()/get_right_block() in the reference)
    std::shared_ptr<Block> block() { return tracking_; }

protected:
    using TrackingAdapterRole::TrackingAdapterRole;

    std::shared_ptr<Block> tracking_;
};

#endif  // GNSSCORR_TRACKING_ADAPTER_BASE_H_
