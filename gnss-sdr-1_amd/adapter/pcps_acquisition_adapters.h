/*!
 * \file pcps_acquisition_adapters.h
 * \brief AcquisitionInterface adapters (GPS L1 C/A, L2C(M), L5I; Galileo E1, E5a; BeiDou B1I, B3I; GLONASS L1 C/A) backed by
 * hip_pcps_acquisition.
 *
 * Configuration keys, derived sizes, local-code generation and the Pfa -> threshold rule follow
 *   GpsL1CaPcpsAcquisition           src/algorithms/acquisition/adapters/gps_l1_ca_pcps_acquisition.cc:46-358
 *   GalileoE1PcpsAmbiguousAcquisition src/algorithms/acquisition/adapters/galileo_e1_pcps_ambiguous_acquisition.cc:46-330
 *   BeidouB1iPcpsAcquisition          src/algorithms/acquisition/adapters/beidou_b1i_pcps_acquisition.cc:45-330
 *   GlonassL1CaPcpsAcquisition        src/algorithms/acquisition/adapters/glonass_l1_ca_pcps_acquisition.cc:44-330
 *   GpsL2MPcpsAcquisition, GpsL5iPcpsAcquisition, GalileoE5aPcpsAcquisition, BeidouB3iPcpsAcquisition (same directory)
 *   GalileoE1PcpsCccwsrAmbiguousAcquisition, GalileoE1Pcps8msAmbiguousAcquisition (same directory): both E1 components, or both sign
 *   hypotheses of an 8 ms replica, in one search -- backed by hip_pcps_paired_acquisition (at the end of this file)
 *   GpsL1CaPcpsAcquisitionFineDoppler (same directory): the search that ends in a 12.5 Hz Doppler estimate -- backed by
 *   hip_pcps_acquisition_fine_doppler (at the end of this file)
 * The members and the overrides that only forward to the block are AcquisitionAdapterBase<Block> (acquisition_adapter_base.h); each
 * adapter here holds its constructor, implementation(), set_threshold(), set_local_code() and the forwarders in which its reference
 * adapter differs.
 * (item_type gr_complex only; `dump` / `dump_filename` / `dump_channel` write the reference's .mat
 * variables, see hip_pcps_acquisition::dump_results; the acquisition resampler and the GNU Radio
 * connect()/get_left_block() plumbing are outside this path).  Registration in a GNSS-SDR tree is one
 * more `else if (implementation == "GPS_L1_CA_PCPS_Acquisition_HIP")` in
 * GNSSBlockFactory::GetAcqBlock (src/core/receiver/gnss_block_factory.cc:1946), see INTEGRATION.md.
 */
#ifndef GNSSCORR_PCPS_ACQUISITION_ADAPTERS_H_
#define GNSSCORR_PCPS_ACQUISITION_ADAPTERS_H_

#include "acquisition_adapter_base.h"
#include "hip_pcps_acquisition.h"
#include "hip_pcps_paired_acquisition.h"
#include "hip_pcps_acquisition_fine_doppler.h"
#include <cmath>
#include <memory>
#include <string>
#include <vector>

namespace gnsscorr
{
enum class AcqSignal
{
    GPS_L1_CA,
    GALILEO_E1,
    BEIDOU_B1I,
    GLONASS_L1_CA,
    GPS_L2_M,
    GPS_L5I,
    GALILEO_E5A,
    BEIDOU_B3I
};

// constants of GPS_L1_CA.h:54-61, Galileo_E1.h:55-60, Beidou_B1I.h:52-56
struct AcqSignalTraits
{
    double code_rate_hz;
    double code_length_chips;
    double chip_period_s;
    double code_period_s;
    uint32_t ms_per_code;
    const char* implementation;
};

inline AcqSignalTraits acq_traits(AcqSignal s)
{
    switch (s)
        {
        case AcqSignal::GALILEO_E1:
            return {1.023e6, 4092.0, 1.0 / 1.023e6, 0.004, 4, "Galileo_E1_PCPS_Ambiguous_Acquisition_HIP"};
        case AcqSignal::BEIDOU_B1I:
            return {2.046e6, 2046.0, 4.8875e-07, 0.001, 1, "BEIDOU_B1I_PCPS_Acquisition_HIP"};
        case AcqSignal::GLONASS_L1_CA:
            return {0.511e6, 511.0, 1.9569e-06, 0.001, 1, "GLONASS_L1_CA_PCPS_Acquisition_HIP"};  // GLONASS_L1_L2_CA.h:93-97
        case AcqSignal::GPS_L2_M:
            return {0.5115e6, 10230.0, 1.0 / 0.5115e6, 0.02, 20, "GPS_L2_M_PCPS_Acquisition_HIP"};  // GPS_L2C.h:56-58
        case AcqSignal::GPS_L5I:
            return {10.23e6, 10230.0, 1.0 / 10.23e6, 0.001, 1, "GPS_L5i_PCPS_Acquisition_HIP"};  // GPS_L5.h:54-57
        case AcqSignal::GALILEO_E5A:
            return {1.023e7, 10230.0, 1.0 / 1.023e7, 0.001, 1, "Galileo_E5a_Pcps_Acquisition_HIP"};  // Galileo_E5a.h:44-51
        case AcqSignal::BEIDOU_B3I:
            return {10.23e6, 10230.0, 1.0 / 10.23e6, 0.001, 1, "BEIDOU_B3I_PCPS_Acquisition_HIP"};  // Beidou_B3I.h:41-44
        default:
            return {1.023e6, 1023.0, 9.7752e-07, 0.001, 1, "GPS_L1_CA_PCPS_Acquisition_HIP"};
        }
}
}  // namespace gnsscorr


template <gnsscorr::AcqSignal SIG>
class PcpsAcquisitionHip : public AcquisitionAdapterBase<hip_pcps_acquisition>
{
public:
    PcpsAcquisitionHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : AcquisitionAdapterBase<hip_pcps_acquisition>(configuration, role, in_streams, out_streams, 2048000)
    {
        using gnsscorr::AcqSignal;
        const gnsscorr::AcqSignalTraits t = gnsscorr::acq_traits(SIG);
        acq_parameters_.fs_in = fs_in_;
        acq_parameters_.resampled_fs = fs_in_;
        acq_parameters_.blocking = configuration_->property(role + ".blocking", true);
        doppler_max_ = configuration_->property(role + ".doppler_max", 5000);
        acq_parameters_.doppler_max = doppler_max_;
        acq_parameters_.bit_transition_flag = configuration_->property(role + ".bit_transition_flag", false);
        acq_parameters_.use_CFAR_algorithm_flag = configuration_->property(role + ".use_CFAR_algorithm", true);
        acq_parameters_.max_dwells = configuration_->property(role + ".max_dwells", 1);
        acq_parameters_.num_doppler_bins_step2 = configuration_->property(role + ".second_nbins", 4);
        acq_parameters_.doppler_step2 = configuration_->property(role + ".second_doppler_step", 125.0f);
        acq_parameters_.make_2_steps = configuration_->property(role + ".make_two_steps", false);
        // gps_l1_ca_pcps_acquisition.cc:56,64-66,84-85
        acq_parameters_.dump = configuration_->property(role + ".dump", false);
        acq_parameters_.dump_channel = configuration_->property(role + ".dump_channel", 0);
        acq_parameters_.dump_filename = configuration_->property(role + ".dump_filename", std::string("./acquisition.mat"));
        acq_parameters_.it_size = sizeof(gr_complex);
        if (SIG == AcqSignal::GPS_L1_CA)
            {
                // gps_l1_ca_pcps_acquisition.cc:75-120
                sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", 1);
                acq_parameters_.sampled_ms = sampled_ms_;
                acq_parameters_.ms_per_code = 1;
                code_length_ = static_cast<unsigned int>(std::floor(static_cast<double>(fs_in_) / (t.code_rate_hz / t.code_length_chips)));
                acq_parameters_.samples_per_ms = static_cast<float>(fs_in_) * 0.001;
                acq_parameters_.samples_per_chip = static_cast<unsigned int>(std::ceil(t.chip_period_s * static_cast<float>(acq_parameters_.fs_in)));
                acq_parameters_.samples_per_code = acq_parameters_.samples_per_ms * static_cast<float>(t.code_period_s * 1000.0);
                vector_length_ = std::floor(acq_parameters_.sampled_ms * acq_parameters_.samples_per_ms) * (acq_parameters_.bit_transition_flag ? 2 : 1);
            }
        else if (SIG == AcqSignal::GALILEO_E1)
            {
                // galileo_e1_pcps_ambiguous_acquisition.cc:67-123
                acq_parameters_.ms_per_code = 4;
                sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", acq_parameters_.ms_per_code);
                acq_parameters_.sampled_ms = sampled_ms_;
                if ((acq_parameters_.sampled_ms % acq_parameters_.ms_per_code) != 0)
                    {
                        acq_parameters_.sampled_ms = acq_parameters_.ms_per_code;
                        sampled_ms_ = acq_parameters_.ms_per_code;
                    }
                acquire_pilot_ = configuration_->property(role + ".acquire_pilot", false);
                code_length_ = static_cast<unsigned int>(std::floor(static_cast<double>(fs_in_) / (t.code_rate_hz / t.code_length_chips)));
                acq_parameters_.samples_per_ms = static_cast<float>(fs_in_) * 0.001;
                acq_parameters_.samples_per_chip = static_cast<unsigned int>(std::ceil((1.0 / t.code_rate_hz) * static_cast<float>(acq_parameters_.fs_in)));
                acq_parameters_.samples_per_code = acq_parameters_.samples_per_ms * static_cast<float>(4);
                vector_length_ = sampled_ms_ * acq_parameters_.samples_per_ms;
                if (acq_parameters_.bit_transition_flag) vector_length_ *= 2;
            }
        else if (SIG == AcqSignal::GPS_L2_M)
            {
                // gps_l2_m_pcps_acquisition.cc:81-128,155: whole 20 ms codes
                acq_parameters_.ms_per_code = 20;
                sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", acq_parameters_.ms_per_code);
                if ((sampled_ms_ % acq_parameters_.ms_per_code) != 0) sampled_ms_ = acq_parameters_.ms_per_code;
                acq_parameters_.sampled_ms = sampled_ms_;
                code_length_ = static_cast<unsigned int>(std::floor(static_cast<double>(fs_in_) / (t.code_rate_hz / t.code_length_chips)));
                acq_parameters_.samples_per_ms = static_cast<float>(fs_in_) * 0.001;
                acq_parameters_.samples_per_chip = static_cast<unsigned int>(std::ceil((1.0 / t.code_rate_hz) * static_cast<float>(acq_parameters_.fs_in)));
                acq_parameters_.samples_per_code = acq_parameters_.samples_per_ms * static_cast<float>(t.code_period_s * 1000.0);
                vector_length_ = acq_parameters_.sampled_ms * acq_parameters_.samples_per_ms * (acq_parameters_.bit_transition_flag ? 2 : 1);
            }
        else if (SIG == AcqSignal::GPS_L5I)
            {
                // gps_l5i_pcps_acquisition.cc:82-135
                sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", 1);
                acq_parameters_.sampled_ms = sampled_ms_;
                acq_parameters_.ms_per_code = 1;
                code_length_ = static_cast<unsigned int>(std::floor(static_cast<double>(fs_in_) / (t.code_rate_hz / t.code_length_chips)));
                acq_parameters_.samples_per_ms = static_cast<float>(fs_in_) * 0.001;
                acq_parameters_.samples_per_chip = static_cast<unsigned int>(std::ceil((1.0 / t.code_rate_hz) * static_cast<float>(acq_parameters_.fs_in)));
                acq_parameters_.samples_per_code = acq_parameters_.samples_per_ms * static_cast<float>(t.code_period_s * 1000.0);
                vector_length_ = std::floor(acq_parameters_.sampled_ms * acq_parameters_.samples_per_ms) * (acq_parameters_.bit_transition_flag ? 2 : 1);
            }
        else if (SIG == AcqSignal::GALILEO_E5A)
            {
                // galileo_e5a_pcps_acquisition.cc:60-144: 1 ms, data (5I), pilot (5Q) or both components (5X) in the replica
                acquire_pilot_ = configuration_->property(role + ".acquire_pilot", false);
                acquire_iq_ = configuration_->property(role + ".acquire_iq", false);
                if (acquire_iq_) acquire_pilot_ = false;
                sampled_ms_ = 1;
                acq_parameters_.sampled_ms = sampled_ms_;
                acq_parameters_.ms_per_code = 1;
                acq_parameters_.samples_per_ms = static_cast<float>(fs_in_) * 0.001;
                acq_parameters_.samples_per_chip = static_cast<unsigned int>(std::ceil((1.0 / t.code_rate_hz) * static_cast<float>(acq_parameters_.fs_in)));
                code_length_ = static_cast<unsigned int>(std::round(static_cast<double>(fs_in_) / t.code_rate_hz * t.code_length_chips));
                vector_length_ = code_length_ * sampled_ms_;
                if (acq_parameters_.bit_transition_flag) vector_length_ *= 2;
                acq_parameters_.samples_per_code = acq_parameters_.samples_per_ms * 1.0f;
            }
        else if (SIG == AcqSignal::GLONASS_L1_CA)
            {
                // glonass_l1_ca_pcps_acquisition.cc:62-113
                sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", 1);
                acq_parameters_.sampled_ms = sampled_ms_;
                acq_parameters_.ms_per_code = 1;
                acq_parameters_.samples_per_chip = static_cast<unsigned int>(std::ceil(t.chip_period_s * static_cast<float>(acq_parameters_.fs_in)));
                code_length_ = static_cast<unsigned int>(std::round(static_cast<double>(fs_in_) / (t.code_rate_hz / t.code_length_chips)));
                vector_length_ = code_length_ * sampled_ms_;
                if (acq_parameters_.bit_transition_flag) vector_length_ *= 2;
                acq_parameters_.samples_per_ms = static_cast<float>(fs_in_) * 0.001;
                acq_parameters_.samples_per_code = acq_parameters_.samples_per_ms * static_cast<float>(t.code_period_s * 1000.0);
            }
        else
            {
                // beidou_b1i_pcps_acquisition.cc:73-104, beidou_b3i_pcps_acquisition.cc:71-104: ms_per_code and samples_per_chip keep
                // Acq_Conf's zeros
                sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", 1);
                acq_parameters_.sampled_ms = sampled_ms_;
                code_length_ = static_cast<uint32_t>(std::round(static_cast<double>(fs_in_) / (t.code_rate_hz / t.code_length_chips)));
                vector_length_ = code_length_ * sampled_ms_;
                if (acq_parameters_.bit_transition_flag) vector_length_ *= 2;
                acq_parameters_.samples_per_ms = code_length_;
                acq_parameters_.samples_per_code = code_length_;
            }
        code_.resize(vector_length_);
        acquisition_ = std::make_shared<hip_pcps_acquisition>(acq_parameters_);
    }

    std::string implementation() override { return gnsscorr::acq_traits(SIG).implementation; }

    //! this block notifies the channel state machine itself (pcps_acquisition.cc:432-436)
    void set_channel_fsm(std::shared_ptr<ChannelFsm> channel_fsm) override
    {
        channel_fsm_ = channel_fsm;
        acquisition_->set_channel_fsm(channel_fsm);
    }

    //! <role>.pfa only, no per-channel key (gps_l1_ca_pcps_acquisition.cc:262-279, same rule in the Galileo and BeiDou adapters).
    //! Departure: with a doppler_step of 0 (set_threshold before set_doppler_step) the reference's bin loop would not end; the given
    //! threshold stays installed
    void set_threshold(float threshold) override
    {
        float pfa = configuration_->property(role_ + ".pfa", 0.0f);
        threshold_ = (pfa == 0.0f || doppler_step_ == 0) ? threshold : gnsscorr::exponential_quantile_threshold(pfa, vector_length_, doppler_max_, doppler_step_);
        acquisition_->set_threshold(threshold_);
    }

    void set_local_code() override
    {
        using gnsscorr::AcqSignal;
        std::vector<gr_complex> code(code_length_ + 8);
        float* dst = reinterpret_cast<float*>(code.data());
        unsigned int reps = sampled_ms_;
        if (SIG == AcqSignal::GPS_L1_CA)
            gc_gps_l1_ca_code_gen_complex_sampled(dst, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
        else if (SIG == AcqSignal::BEIDOU_B1I)
            gc_beidou_b1i_code_gen_complex_sampled(dst, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
        else if (SIG == AcqSignal::GLONASS_L1_CA)
            gc_glonass_l1_ca_code_gen_complex_sampled(dst, static_cast<int32_t>(fs_in_), 0, nullptr);  // one code for every slot (FDMA)
        else if (SIG == AcqSignal::BEIDOU_B3I)
            gc_beidou_b3i_code_gen_complex_sampled(dst, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
        else if (SIG == AcqSignal::GPS_L5I)
            gc_gps_l5i_code_gen_complex_sampled(dst, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), nullptr);
        else if (SIG == AcqSignal::GPS_L2_M)
            {
                gc_gps_l2c_m_code_gen_complex_sampled(dst, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), nullptr);
                reps = sampled_ms_ / 20;
            }
        else if (SIG == AcqSignal::GALILEO_E5A)
            {
                // galileo_e5a_pcps_acquisition.cc:238-266
                const char* sig = acquire_iq_ ? "5X" : acquire_pilot_ ? "5Q" : "5I";
                gc_galileo_e5_a_code_gen_complex_sampled(dst, sig, gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
            }
        else
            {
                // galileo_e1_pcps_ambiguous_acquisition.cc:240-284: the pilot if asked for, else whatever signal the synchro names
                const char sig[3] = {acquire_pilot_ ? '1' : gnss_synchro_->Signal[0], acquire_pilot_ ? 'C' : gnss_synchro_->Signal[1], 0};
                gnsscorr::e1_code_sampled(configuration_, channel_, gnss_synchro_, fs_in_, code.data(), sig);
                reps = sampled_ms_ / 4;
            }
        gnsscorr::tile_code(code.data(), code_length_, reps, code_.data());
        acquisition_->set_local_code(code_.data());
    }

    //! this block takes the resampler's latency into its sample stamps
    void set_resampler_latency(uint32_t latency_samples) override { acquisition_->set_resampler_latency(latency_samples); }

private:
    Acq_Conf acq_parameters_;
    unsigned int sampled_ms_ = 1;
    bool acquire_pilot_ = false;
    bool acquire_iq_ = false;
    std::vector<gr_complex> code_;
};

using GpsL1CaPcpsAcquisitionHip = PcpsAcquisitionHip<gnsscorr::AcqSignal::GPS_L1_CA>;
using GalileoE1PcpsAmbiguousAcquisitionHip = PcpsAcquisitionHip<gnsscorr::AcqSignal::GALILEO_E1>;
using BeidouB1iPcpsAcquisitionHip = PcpsAcquisitionHip<gnsscorr::AcqSignal::BEIDOU_B1I>;
using GpsL2MPcpsAcquisitionHip = PcpsAcquisitionHip<gnsscorr::AcqSignal::GPS_L2_M>;
using GpsL5iPcpsAcquisitionHip = PcpsAcquisitionHip<gnsscorr::AcqSignal::GPS_L5I>;
using GalileoE5aPcpsAcquisitionHip = PcpsAcquisitionHip<gnsscorr::AcqSignal::GALILEO_E5A>;
using BeidouB3iPcpsAcquisitionHip = PcpsAcquisitionHip<gnsscorr::AcqSignal::BEIDOU_B3I>;
//! the block applies the FDMA offset in set_local_code() once hip_pcps_acquisition::set_glonass_channel_map() holds the almanac
using GlonassL1CaPcpsAcquisitionHip = PcpsAcquisitionHip<gnsscorr::AcqSignal::GLONASS_L1_CA>;


/*! GalileoE1PcpsCccwsrAmbiguousAcquisition (galileo_e1_pcps_cccwsr_ambiguous_acquisition.cc:42-243) and
 *  GalileoE1Pcps8msAmbiguousAcquisition (galileo_e1_pcps_8ms_ambiguous_acquisition.cc:41-263) over hip_pcps_paired_acquisition.
 *  Keys of both: doppler_max, coherent_integration_time_ms (default 4; rounded down to a multiple of 4, :65-73 / :66-74),
 *  max_dwells, Acquisition<ch>.cboc, dump, dump_filename; code_length = round(fs / (1.023e6 / 4092)), samples_per_ms = code_length / 4,
 *  vector_length = code_length * (coherent_integration_time_ms / 4).  Threshold: the CCCWSR adapter installs the value it is given
 *  (its Pfa rule is "not implemented", :237-243); the 8 ms adapter looks up <role><ch>.pfa, then <role>.pfa, and applies the
 *  exponential-quantile rule (:136-160, :245-263).  The E1-B and E1-C replicas come from gc_galileo_e1_code_gen_complex_sampled;
 *  the CCCWSR adapter of the reference generates ONE code period whatever the coherent time and hands the block a buffer it reads
 *  vector_length samples of (:199-220) -- here the period is tiled over the coherent time, as its 8 ms sibling does (:224-228).
 *  Departure: with a doppler_step of 0 (set_threshold before set_doppler_step) the bin loop of the 8 ms adapter's rule would not
 *  end; the given threshold stays installed. */
template <hip_pcps_paired_acquisition::Kind KIND>
class GalileoE1PairedAcquisitionHip : public AcquisitionAdapterBase<hip_pcps_paired_acquisition>
{
public:
    GalileoE1PairedAcquisitionHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : AcquisitionAdapterBase<hip_pcps_paired_acquisition>(configuration, role, in_streams, out_streams, 4000000)
    {
        dump_ = configuration_->property(role + ".dump", false);
        doppler_max_ = configuration_->property(role + ".doppler_max", 5000);
        sampled_ms_ = configuration_->property(role + ".coherent_integration_time_ms", 4);
        if (sampled_ms_ % 4 != 0) sampled_ms_ = static_cast<int>(sampled_ms_ / 4) * 4;
        max_dwells_ = configuration_->property(role + ".max_dwells", 1);
        dump_filename_ = configuration_->property(role + ".dump_filename", std::string("../data/acquisition.dat"));
        code_length_ = static_cast<unsigned int>(std::round(static_cast<double>(fs_in_) / (1.023e6 / 4092.0)));
        vector_length_ = code_length_ * static_cast<int>(sampled_ms_ / 4);
        const int samples_per_ms = code_length_ / 4;
        acquisition_ = std::make_shared<hip_pcps_paired_acquisition>(KIND, sampled_ms_, max_dwells_, doppler_max_, fs_in_, samples_per_ms, code_length_, dump_, dump_filename_);
    }

    std::string implementation() override
    {
        return KIND == hip_pcps_paired_acquisition::CCCWSR ? "Galileo_E1_PCPS_CCCWSR_Ambiguous_Acquisition_HIP" : "Galileo_E1_PCPS_8ms_Ambiguous_Acquisition_HIP";
    }

    //! CCCWSR installs the threshold it is given; the 8 ms kind applies the Pfa rule (galileo_e1_pcps_8ms_ambiguous_acquisition.cc:245-263)
    void set_threshold(float threshold) override
    {
        threshold_ = threshold;
        if (KIND == hip_pcps_paired_acquisition::E1_8MS)
            {
                const float pfa = pfa_for_channel();
                if (pfa != 0.0f && doppler_step_ != 0) threshold_ = gnsscorr::exponential_quantile_threshold(pfa, vector_length_, doppler_max_, doppler_step_);
            }
        acquisition_->set_threshold(threshold_);
    }

    void set_local_code() override
    {
        std::vector<gr_complex> one(code_length_ + 8), data(vector_length_), pilot(vector_length_);
        // CCCWSR: E1-B and E1-C; 8 ms: the synchro's component
        gnsscorr::e1_code_sampled(configuration_, channel_, gnss_synchro_, fs_in_, one.data(), KIND == hip_pcps_paired_acquisition::CCCWSR ? "1B" : nullptr);
        gnsscorr::tile_code(one.data(), code_length_, sampled_ms_ / 4, data.data());
        if (KIND == hip_pcps_paired_acquisition::CCCWSR)
            {
                gnsscorr::e1_code_sampled(configuration_, channel_, gnss_synchro_, fs_in_, one.data(), "1C");
                gnsscorr::tile_code(one.data(), code_length_, sampled_ms_ / 4, pilot.data());
                acquisition_->set_local_code(data.data(), pilot.data());
            }
        else
            acquisition_->set_local_code(data.data());
    }

private:
    std::string dump_filename_;
    unsigned int sampled_ms_ = 4;
    unsigned int max_dwells_ = 1;
    bool dump_ = false;
};

using GalileoE1PcpsCccwsrAmbiguousAcquisitionHip = GalileoE1PairedAcquisitionHip<hip_pcps_paired_acquisition::CCCWSR>;
using GalileoE1Pcps8msAmbiguousAcquisitionHip = GalileoE1PairedAcquisitionHip<hip_pcps_paired_acquisition::E1_8MS>;

/*! GpsL1CaPcpsAcquisitionFineDoppler (gps_l1_ca_pcps_acquisition_fine_doppler.cc:44-189) over hip_pcps_acquisition_fine_doppler.  Keys:
 *  doppler_max (5000), coherent_integration_time_ms (1; read and, as in the reference, not used by the block), max_dwells (1), dump,
 *  dump_filename ("./acquisition.mat"), blocking_on_standby (false); doppler_step and threshold come through the interface.
 *  vector_length = round(fs / (1.023e6 / 1023)) = samples_per_ms; the local code is one sampled code period. */
class GpsL1CaPcpsAcquisitionFineDopplerHip : public AcquisitionAdapterBase<hip_pcps_acquisition_fine_doppler>
{
public:
    GpsL1CaPcpsAcquisitionFineDopplerHip(ConfigurationInterface* configuration, const std::string& role, unsigned int in_streams, unsigned int out_streams)
        : AcquisitionAdapterBase<hip_pcps_acquisition_fine_doppler>(configuration, role, in_streams, out_streams, 2048000)
    {
        dump_ = configuration->property(role + ".dump", false);
        dump_filename_ = configuration->property(role + ".dump_filename", std::string("./acquisition.mat"));
        doppler_max_ = configuration->property(role + ".doppler_max", 5000);
        sampled_ms_ = configuration->property(role + ".coherent_integration_time_ms", 1);
        max_dwells_ = configuration->property(role + ".max_dwells", 1);
        blocking_on_standby_ = configuration->property(role + ".blocking_on_standby", false);
        vector_length_ = static_cast<unsigned int>(std::round(static_cast<double>(fs_in_) / (1.023e6 / 1023.0)));
        acquisition_ = std::make_shared<hip_pcps_acquisition_fine_doppler>(max_dwells_, doppler_max_, fs_in_, static_cast<int32_t>(vector_length_), blocking_on_standby_, dump_,
            dump_filename_);
    }

    std::string implementation() override { return "GPS_L1_CA_PCPS_Acquisition_Fine_Doppler_HIP"; }

    void set_threshold(float threshold) override
    {
        threshold_ = threshold;
        acquisition_->set_threshold(threshold_);
    }

    void set_local_code() override
    {
        std::vector<gr_complex> code(vector_length_ + 8);
        gc_gps_l1_ca_code_gen_complex_sampled(reinterpret_cast<float*>(code.data()), gnss_synchro_->PRN, static_cast<int32_t>(fs_in_), 0, nullptr);
        acquisition_->set_local_code(code.data());
    }

    //! the block's mag() is its statistic, cut to an integer
    signed int mag() override { return static_cast<signed int>(acquisition_->mag()); }

    unsigned int doppler_max() const { return doppler_max_; }
    unsigned int sampled_ms() const { return sampled_ms_; }
    unsigned int max_dwells() const { return max_dwells_; }
    bool blocking_on_standby() const { return blocking_on_standby_; }
    bool dump() const { return dump_; }
    const std::string& dump_filename() const { return dump_filename_; }

private:
    std::string dump_filename_;
    unsigned int sampled_ms_ = 1;
    unsigned int max_dwells_ = 1;
    bool dump_ = false, blocking_on_standby_ = false;
};

#endif  // GNSSCORR_PCPS_ACQUISITION_ADAPTERS_H_
