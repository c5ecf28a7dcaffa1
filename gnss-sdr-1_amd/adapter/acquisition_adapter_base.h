/*!
 * \file acquisition_adapter_base.h
 * \brief What the AcquisitionInterface adapters of this directory share: AcquisitionAdapterBase<Block> with the members and the
 * overrides that only forward to the block, the sampling-rate and Pfa look-ups, and the free helpers for the Pfa -> threshold rule,
 * the Galileo E1 replica and the tiling of a code period.  A concrete adapter holds its constructor (keys, defaults, derived sizes),
 * implementation(), set_threshold() and set_local_code(), and overrides a forwarder only where its reference adapter differs.
 */
#ifndef GNSSCORR_ACQUISITION_ADAPTER_BASE_H_
#define GNSSCORR_ACQUISITION_ADAPTER_BASE_H_

#include "acquisition_block_base.h"
#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include <cmath>
#include <cstring>
#include <memory>
#include <string>

namespace gnsscorr
{
/*! calculate_threshold of the reference's adapters (gps_l1_ca_pcps_acquisition.cc:262-279,
 *  galileo_e1_pcps_8ms_ambiguous_acquisition.cc:245-263): the quantile of an exponential distribution of rate lambda = vector_length,
 *  -ln(1 - p) / lambda, at p = (1 - pfa)^(1 / ncells) with ncells = vector_length * inclusive bins (an unsigned product, as there).
 *  With a doppler_step of 0 there are no cells and no rule: callers keep the threshold they were given. */
inline float exponential_quantile_threshold(float pfa, unsigned int vector_length, unsigned int doppler_max, unsigned int doppler_step)
{
    const unsigned int frequency_bins = inclusive_doppler_bins(doppler_max, doppler_step);
    unsigned int ncells = vector_length * frequency_bins;
    double exponent = 1 / static_cast<double>(ncells);
    double val = std::pow(1.0 - pfa, exponent);
    auto lambda = double(vector_length);
    return static_cast<float>(-std::log(1.0 - val) / lambda);
}

/*! One sampled Galileo E1 code period into dst (code_length + 8 complex at least): Acquisition<ch>.cboc is looked up per channel
 *  (galileo_e1_pcps_ambiguous_acquisition.cc:240-284); the signal is force_signal if given, else "1C" when the synchro says so and "1B"
 *  otherwise -- without a synchro signal the data component is searched, as "1B" selects it in the reference's generator */
inline void e1_code_sampled(ConfigurationInterface* configuration, unsigned int channel, const Gnss_Synchro* synchro, int64_t fs, gr_complex* dst, const char* force_signal = nullptr)
{
    const bool cboc = configuration->property("Acquisition" + std::to_string(channel) + ".cboc", false);
    const char* sig = force_signal ? force_signal : ((synchro->Signal[0] == '1' && synchro->Signal[1] == 'C') ? "1C" : "1B");
    gc_galileo_e1_code_gen_complex_sampled(reinterpret_cast<float*>(dst), sig, cboc ? 1 : 0, synchro->PRN, static_cast<int32_t>(fs), 0, nullptr);
}

//! `reps` copies of one code period of code_length samples, one behind the other in dst
inline void tile_code(const gr_complex* one_period, unsigned int code_length, unsigned int reps, gr_complex* dst)
{
    for (unsigned int i = 0; i < reps; i++) std::memcpy(dst + static_cast<size_t>(i) * code_length, one_period, sizeof(gr_complex) * code_length);
}
}  // namespace gnsscorr

template <class Block>
class AcquisitionAdapterBase : public AcquisitionInterface
{
public:
    std::string role() override { return role_; }
    size_t item_size() override { return sizeof(gr_complex); }

    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) override
    {
        gnss_synchro_ = p_gnss_synchro;
        acquisition_->set_gnss_synchro(gnss_synchro_);
    }

    void set_channel(unsigned int channel) override
    {
        channel_ = channel;
        acquisition_->set_channel(channel_);
    }

    void set_channel_fsm(std::shared_ptr<ChannelFsm> channel_fsm) override { channel_fsm_ = channel_fsm; }

    void set_doppler_max(unsigned int doppler_max) override
    {
        doppler_max_ = doppler_max;
        acquisition_->set_doppler_max(doppler_max_);
    }

    void set_doppler_step(unsigned int doppler_step) override
    {
        doppler_step_ = doppler_step;
        acquisition_->set_doppler_step(doppler_step_);
    }

    void init() override { acquisition_->init(); }
    void set_state(int state) override { acquisition_->set_state(state); }
    signed int mag() override { return acquisition_->mag(); }
    void reset() override { acquisition_->set_active(true); }
    void stop_acquisition() override {}
    void set_resampler_latency(uint32_t) override {}

    //! the block (get_left_block() in the reference, behind a stream_to_vector of vector_length() samples where it takes items)
    std::shared_ptr<Block> block() { return acquisition_; }
    unsigned int vector_length() const { return vector_length_; }
    float threshold() const { return threshold_; }

protected:
    //! reads item_type and the sampling rate; the concrete constructor reads its own keys and makes acquisition_
    AcquisitionAdapterBase(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams, int64_t default_fs)
        : configuration_(configuration), role_(role), in_streams_(in_streams), out_streams_(out_streams)
    {
        item_type_ = configuration_->property(role + ".item_type", std::string("gr_complex"));
        fs_in_ = read_fs(configuration_, default_fs);
    }

    //! GNSS-SDR.internal_fs_sps, else the deprecated key it replaced, else the adapter's default
    static int64_t read_fs(ConfigurationInterface* configuration, int64_t default_fs)
    {
        int64_t fs_in_deprecated = configuration->property("GNSS-SDR.internal_fs_hz", default_fs);
        return configuration->property("GNSS-SDR.internal_fs_sps", fs_in_deprecated);
    }

    //! <role><ch>.pfa, then <role>.pfa; 0 when neither is set
    float pfa_for_channel()
    {
        float pfa = configuration_->property(role_ + std::to_string(channel_) + ".pfa", 0.0f);
        if (pfa == 0.0f) pfa = configuration_->property(role_ + ".pfa", 0.0f);
        return pfa;
    }

    ConfigurationInterface* configuration_;
    std::shared_ptr<Block> acquisition_;
    std::string item_type_;
    std::string role_;
    unsigned int in_streams_;
    unsigned int out_streams_;
    unsigned int vector_length_ = 0;
    unsigned int code_length_ = 0;
    unsigned int channel_ = 0;
    unsigned int doppler_max_ = 0;
    unsigned int doppler_step_ = 0;
    float threshold_ = 0.0f;
    int64_t fs_in_ = 0;
    std::shared_ptr<ChannelFsm> channel_fsm_;
    Gnss_Synchro* gnss_synchro_ = nullptr;
};

#endif  // GNSSCORR_ACQUISITION_ADAPTER_BASE_H_
