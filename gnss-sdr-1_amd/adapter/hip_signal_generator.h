/*!
 * \file hip_signal_generator.h
 * \brief The signal source of a receiver without a capture file, on the GPU: a synthetic multi-satellite scene written into a ring.
 *
 * The reference's Signal_Generator source (src/algorithms/signal_generator/adapters/signal_generator.cc, block
 * gnuradio_blocks/signal_generator_c.cc) feeds its own acquisition tests.  This class reads that adapter's configuration keys --
 *   SignalSource.fs_hz            [Hz]                                            (default 4000000)
 *   SignalSource.num_satellites                                                   (default 1)
 *   SignalSource.system_i         "G" | "R" | "E"                                 (default "G")
 *   SignalSource.signal_i         "1C" | "1G" | "1B" | "5X"                       (default "1C")
 *   SignalSource.PRN_i                                                            (default 1)
 *   SignalSource.CN0_dB_i         [dB-Hz]                                         (default 10)
 *   SignalSource.doppler_Hz_i     [Hz]                                            (default 0)
 *   SignalSource.delay_chips_i    [chips]                                         (default 0)
 *   SignalSource.delay_sec_i      [secondary-code chips]                          (default 0)
 *   SignalSource.data_flag, SignalSource.noise_flag                               (default false)
 *   SignalSource.BW_BB            baseband bandwidth as a fraction of fs / 2      (default 1.0)
 *   <role>.item_type              "gr_complex", the only type the reference's adapter makes a block for
 * -- and four of this library under the role:
 *   seed                          64-bit seed of the noise and the data symbols   (default 0)
 *   intermediate_freq_hz          GLONASS: the frequency of channel 0 in the stream (default 4000000, the block's hard-coded
 *                                 value, of which its source says "must be set by the user")
 *   output_item_type              "gr_complex" | "cshort" | "cbyte": the ring's format (default: item_type)
 *   output_scale                  factor in front of the clamp of a cshort / cbyte ring (default 1; 127 for cbyte)
 * -- owns the ring and the device generator (gc_signal_generator) that writes it, and work(n_vectors) appends n_vectors vectors of
 * vector_length() samples, the block's output item, computed by the adapter's rule (signal_generator.cc:86-117).
 *
 * Not mirrored (gnsscorr.h, "Signal generator"): the block's unseeded std::default_random_engine -- noise and data here are
 * functions of `seed` and the sample number -- and the PRN / PRN - 1 index slip of its E5a initialisation.  Data symbols change at
 * the satellite's own code-period boundary (the block changes them delay_chips into its vector), and a Galileo E1 table is read by
 * the exact sampling rule where the block's float32 quotient slips an entry at isolated samples.
 */
#ifndef GNSSCORR_HIP_SIGNAL_GENERATOR_H_
#define GNSSCORR_HIP_SIGNAL_GENERATOR_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

class hip_signal_generator
{
public:
    /*! ring_capacity / max_window: size of the ring and its longest window, in samples (gc_stream_create) */
    hip_signal_generator(gc_ctx* ctx, ConfigurationInterface* configuration, const std::string& role, uint64_t ring_capacity, uint32_t max_window)
    {
        d_item_type = configuration->property(role + ".item_type", std::string("gr_complex"));
        d_fs = configuration->property("SignalSource.fs_hz", 4e6);
        const bool data_flag = configuration->property("SignalSource.data_flag", false);
        const bool noise_flag = configuration->property("SignalSource.noise_flag", false);
        const double bw_bb = configuration->property("SignalSource.BW_BB", 1.0);
        const uint32_t num_satellites = configuration->property("SignalSource.num_satellites", static_cast<uint32_t>(1));
        const int64_t seed = configuration->property(role + ".seed", static_cast<int64_t>(0));
        const double intermediate_freq = configuration->property(role + ".intermediate_freq_hz", 4e6);
        const std::string out_item_type = configuration->property(role + ".output_item_type", d_item_type);
        if (d_item_type != "gr_complex" || !gnsscorr_iq_format(out_item_type, &d_out_format) || num_satellites < 1 || num_satellites > GC_SIGGEN_MAX_SATS)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        d_out_scale = configuration->property(role + ".output_scale", d_out_format == GC_IQ_I8 ? 127.0f : 1.0f);
        d_sats.resize(num_satellites);
        d_tables.resize(num_satellites);
        d_secondaries.resize(num_satellites);
        double sigma = 0.0;
        for (uint32_t i = 0; i < num_satellites; i++)
            {
                const std::string sat = std::to_string(i);
                d_signal.push_back(configuration->property("SignalSource.signal_" + sat, std::string("1C")));
                d_system.push_back(configuration->property("SignalSource.system_" + sat, std::string("G")));
                const uint32_t prn = configuration->property("SignalSource.PRN_" + sat, static_cast<uint32_t>(1));
                const double cn0 = configuration->property("SignalSource.CN0_dB_" + sat, 10.0);
                const double doppler = configuration->property("SignalSource.doppler_Hz_" + sat, 0.0);
                const uint32_t delay_chips = configuration->property("SignalSource.delay_chips_" + sat, static_cast<uint32_t>(0));
                const uint32_t delay_sec = configuration->property("SignalSource.delay_sec_" + sat, static_cast<uint32_t>(0));
                d_tables[i].assign(2 * static_cast<size_t>(GC_SIGGEN_MAX_TABLE), 0.0f);
                d_secondaries[i].assign(2 * static_cast<size_t>(GC_SIGGEN_MAX_SECONDARY), 0);
                d_status = gc_siggen_reference_satellite(d_system[i].c_str(), d_signal[i].c_str(), prn, cn0, doppler, delay_chips, delay_sec, d_fs, bw_bb,
                    data_flag ? 1 : 0, noise_flag ? 1 : 0, intermediate_freq, &d_sats[i], d_tables[i].data(), GC_SIGGEN_MAX_TABLE, d_secondaries[i].data(), &sigma);
                if (d_status != GC_OK) return;
            }
        // the block's output item (signal_generator.cc:86-117): 100 ms with Galileo E1, one code period otherwise
        const auto present = [&](const char* s) { return std::find(d_system.begin(), d_system.end(), std::string(s)) != d_system.end(); };
        const float fs_f = static_cast<float>(static_cast<unsigned int>(d_fs));
        if (present("E"))
            d_vector_length = d_signal[0].at(0) == '5' ? static_cast<uint32_t>(std::round(fs_f / (10.23e6 / 10230.0)))
                                                       : static_cast<uint32_t>(std::round(fs_f / (1.023e6 / 4092.0))) * 25u;
        else if (present("G"))
            d_vector_length = static_cast<uint32_t>(std::round(fs_f / (1.023e6 / 1023.0)));
        else if (present("R"))
            d_vector_length = static_cast<uint32_t>(std::round(fs_f / (0.511e6 / 511.0)));
        if (d_vector_length == 0)
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        gc_siggen_conf c;
        c.fs_hz = d_fs;
        c.noise_sigma = sigma;
        c.seed = static_cast<uint64_t>(seed);
        c.t0 = 0;
        c.n_sats = num_satellites;
        c.table_placement = GC_SIGGEN_TABLES_AUTO;
        c.sats = d_sats.data();
        d_status = gc_stream_create(ctx, d_out_format, std::max<uint64_t>(ring_capacity, 2ull * max_window), max_window, &d_ring);
        if (d_status == GC_OK && d_out_format != GC_IQ_F32) d_status = gc_stream_accept_quantised_output(d_ring);
        if (d_status == GC_OK) d_status = gc_signal_generator_create(ctx, &c, d_ring, &d_gen);
        if (d_status == GC_OK && d_out_format != GC_IQ_F32) d_status = gc_signal_generator_set_output_scale(d_gen, d_out_scale);
    }
    ~hip_signal_generator()
    {
        if (d_gen) gc_signal_generator_destroy(d_gen);
        if (d_ring) gc_stream_destroy(d_ring);
    }
    hip_signal_generator(const hip_signal_generator&) = delete;
    hip_signal_generator& operator=(const hip_signal_generator&) = delete;

    //! appends n_vectors output items of vector_length() samples (asynchronous); first_index: the stream index of the first sample
    gc_status work(uint32_t n_vectors, uint64_t* first_index = nullptr)
    {
        if (d_gen == nullptr) return d_status;
        d_status = gc_signal_generator_generate(d_gen, static_cast<uint64_t>(n_vectors) * d_vector_length, first_index);
        return d_status;
    }
    //! the ring: pass it to the acquisition bank and the tracking group together with fs_hz()
    gc_stream* ring() const { return d_ring; }
    double fs_hz() const { return d_fs; }
    //! samples per output item of the reference's block
    uint32_t vector_length() const { return d_vector_length; }
    //! gc_iq_format of the ring (output_item_type) and the factor in front of its clamp (1 for gr_complex)
    int output_format() const { return d_out_format; }
    float output_scale() const { return d_out_format == GC_IQ_F32 ? 1.0f : d_out_scale; }
    //! the satellites as the generator was given them
    const std::vector<gc_siggen_sat>& satellites() const { return d_sats; }
    //! samples generated so far (the ring's head)
    uint64_t head() const
    {
        uint64_t h = 0;
        if (d_gen) gc_signal_generator_info(d_gen, &h);
        return h;
    }
    gc_status last_status() const { return d_status; }

private:
    double d_fs = 0.0;
    std::string d_item_type;
    int d_out_format = GC_IQ_F32;
    float d_out_scale = 1.0f;
    uint32_t d_vector_length = 0;
    std::vector<std::string> d_system, d_signal;
    std::vector<gc_siggen_sat> d_sats;
    std::vector<std::vector<float>> d_tables;
    std::vector<std::vector<int8_t>> d_secondaries;
    gc_stream* d_ring = nullptr;
    gc_signal_generator* d_gen = nullptr;
    gc_status d_status = GC_OK;
};

#endif  // GNSSCORR_HIP_SIGNAL_GENERATOR_H_
