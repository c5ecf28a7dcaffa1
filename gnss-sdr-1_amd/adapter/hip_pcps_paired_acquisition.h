/*!
 * \file hip_pcps_paired_acquisition.h
 * \brief Image of the reference's two-hypothesis PCPS blocks, searched by a paired MAX engine of libgnsscorr.so (gc_acq_create_paired):
 *   pcps_cccwsr_acquisition_cc        (src/algorithms/acquisition/gnuradio_blocks/pcps_cccwsr_acquisition_cc.{h,cc})
 *   galileo_pcps_8ms_acquisition_cc   (src/algorithms/acquisition/gnuradio_blocks/galileo_pcps_8ms_acquisition_cc.{h,cc})
 * Both correlate every Doppler bin's spectrum with two replicas and keep the larger |.|^2: CCCWSR forms d + jp and d - jp of the
 * data and pilot correlations (:342-351), which by linearity are the correlations with cd - j cp and cd + j cp
 * (gc_cccwsr_replicas); the 8 ms block searches code A and code B = A with its second code period negated (:150-165,
 * gc_e1_8ms_replicas).  The engine combines the two on the device and writes max(a, b) once per cell.
 *
 * Contracts kept:
 *   - the Doppler bins run from -doppler_max to +doppler_max INCLUSIVE (cccwsr :195-202, 8ms :182-189), Doppler of bin i is
 *     -doppler_max + doppler_step * i;
 *   - statistic = mag / input_power with mag = max |.|^2 / N^4 (cccwsr :355-359, :399; 8ms :317-333, :374): the engine runs one CFAR
 *     dwell per call (max_dwells = 1, gc_acq_reset between dwells) and the best dwell is kept here.  CCCWSR keeps d_mag and the
 *     synchro fields across the dwells of a search (:373-380, reset in set_state / state 0); the 8 ms block restarts d_mag with
 *     every dwell (:272-273);
 *   - positive at statistic > threshold, negative when the dwell count reaches max_dwells (cccwsr :402-409, 8ms :376-383); the
 *     "events" port carries 1 (ACQ_SUCCESS) or 2 (ACQ_FAIL) from states 2 and 3;
 *   - general_work(noutput, ninput_items, input_items, ..) becomes work(in, ninput_items[0]) on items of fft_size() samples
 *     (the adapter's stream_to_vector), consume_each(n) the return value.
 * Documented departure: the reference takes the maxima of the two hypotheses' rows separately and prefers the first (plus / A) on
 * a tie (cccwsr :361-370, 8ms :336-345); the engine takes the row maximum of the per-sample maximum.  The two differ only if both
 * hypotheses reach the identical float maximum at different indices.  `dump` writes, per Doppler bin, the combined |.|^2 row
 * (fft_size float32) under the reference's file name test_statistics_<System>_<Signal>_sat_<PRN>_doppler_<Hz>.dat in the directory
 * of dump_filename; the reference writes the last inverse transform's complex output there (cccwsr :383-394).
 */
#ifndef GNSSCORR_HIP_PCPS_PAIRED_ACQUISITION_H_
#define GNSSCORR_HIP_PCPS_PAIRED_ACQUISITION_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include "hip_multicorrelator_real_codes.h"  // gnsscorr::shared_context()
#include <cmath>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

class hip_pcps_paired_acquisition
{
public:
    enum Kind
    {
        CCCWSR,  //!< pcps_cccwsr_acquisition_cc: set_local_code(data, pilot)
        E1_8MS   //!< galileo_pcps_8ms_acquisition_cc: set_local_code(code)
    };

    hip_pcps_paired_acquisition(Kind kind, uint32_t sampled_ms, uint32_t max_dwells, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms,
        int32_t samples_per_code, bool dump, const std::string& dump_filename)
        : d_kind(kind), d_fs_in(fs_in), d_samples_per_ms(samples_per_ms), d_samples_per_code(samples_per_code), d_sampled_ms(sampled_ms), d_max_dwells(max_dwells), d_doppler_max(doppler_max), d_dump(dump), d_dump_filename(dump_filename)
    {
        d_fft_size = d_sampled_ms * d_samples_per_ms;
        d_code_a.assign(d_fft_size, gr_complex(0.0f, 0.0f));
        d_code_b.assign(d_fft_size, gr_complex(0.0f, 0.0f));
    }

    ~hip_pcps_paired_acquisition()
    {
        if (d_acq != nullptr) gc_acq_destroy(d_acq);
    }

    hip_pcps_paired_acquisition(const hip_pcps_paired_acquisition&) = delete;
    hip_pcps_paired_acquisition& operator=(const hip_pcps_paired_acquisition&) = delete;

    inline void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    inline uint32_t mag() const { return d_mag; }
    inline void set_active(bool active) { d_active = active; }
    inline void set_channel(uint32_t channel) { d_channel = channel; }
    inline void set_threshold(float threshold) { d_threshold = threshold; }
    inline void set_doppler_max(uint32_t doppler_max) { d_doppler_max = doppler_max; }
    inline void set_doppler_step(uint32_t doppler_step) { d_doppler_step = doppler_step; }

    /*! pcps_cccwsr_acquisition_cc::set_local_code (:161-179): fft_size samples of the data and of the pilot code */
    void set_local_code(std::complex<float>* code_data, std::complex<float>* code_pilot)
    {
        d_status = gc_cccwsr_replicas(reinterpret_cast<const float*>(code_data), reinterpret_cast<const float*>(code_pilot), d_fft_size,
            reinterpret_cast<float*>(d_code_a.data()), reinterpret_cast<float*>(d_code_b.data()));
        install_codes();
    }

    /*! galileo_pcps_8ms_acquisition_cc::set_local_code (:147-166): fft_size samples, at least two code periods */
    void set_local_code(std::complex<float>* code)
    {
        d_status = gc_e1_8ms_replicas(reinterpret_cast<const float*>(code), d_fft_size, static_cast<uint32_t>(d_samples_per_code),
            reinterpret_cast<float*>(d_code_a.data()), reinterpret_cast<float*>(d_code_b.data()));
        install_codes();
    }

    /*! init (cccwsr :182-216, 8ms :169-202): clears the synchro fields, counts the bins, (re)creates the engine whose wipe-off
     *  table is the blocks' volk_gnsssdr_s32f_sincos_32fc grid */
    void init()
    {
        d_gnss_synchro->Flag_valid_acquisition = false;
        d_gnss_synchro->Flag_valid_symbol_output = false;
        d_gnss_synchro->Flag_valid_pseudorange = false;
        d_gnss_synchro->Flag_valid_word = false;
        d_gnss_synchro->Acq_doppler_step = 0U;
        d_gnss_synchro->Acq_delay_samples = 0.0;
        d_gnss_synchro->Acq_doppler_hz = 0.0;
        d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
        d_mag = 0.0;
        d_input_power = 0.0;
        // Count the number of bins: both ends of the range
        d_num_doppler_bins = 0;
        for (auto doppler = static_cast<int32_t>(-d_doppler_max); doppler <= static_cast<int32_t>(d_doppler_max); doppler += d_doppler_step) d_num_doppler_bins++;
        if (d_acq != nullptr)
            {
                gc_acq_destroy(d_acq);
                d_acq = nullptr;
            }
        gc_acq_conf c;
        std::memset(&c, 0, sizeof c);
        c.fs_in = d_fs_in;
        c.sampled_ms = d_sampled_ms;
        c.ms_per_code = d_sampled_ms;  // the blocks transform exactly the block they consume
        c.samples_per_ms = static_cast<float>(d_samples_per_ms);
        c.samples_per_code = static_cast<float>(d_samples_per_code);
        c.samples_per_chip = static_cast<uint32_t>(std::ceil(static_cast<double>(d_fs_in) / 1.023e6));
        c.doppler_max = d_doppler_max;
        c.doppler_step = d_doppler_step;
        c.max_dwells = 1;
        c.use_CFAR_algorithm_flag = 1;
        c.num_doppler_bins_override = d_num_doppler_bins;
        gc_ctx* ctx = gnsscorr::shared_context();
        d_status = ctx ? gc_acq_create_paired(ctx, &c, 1, GC_ACQ_COMBINE_MAX, &d_acq) : GC_ERR_NO_DEVICE;
        if (d_status == GC_OK && d_have_code) install_codes();
    }

    void set_state(int32_t state)
    {
        d_state = state;
        if (d_state == 1) restart();
    }

    /*! general_work (cccwsr :243-468, 8ms :229-442) on items of fft_size() samples.  Returns the number of items consumed. */
    int work(const gr_complex* in, int ninput_items)
    {
        switch (d_state)
            {
            case 0:
                if (d_active)
                    {
                        restart();
                        d_state = 1;
                    }
                d_sample_counter += static_cast<uint64_t>(d_fft_size) * static_cast<uint64_t>(ninput_items);
                return ninput_items;
            case 1:
                dwell(in);
                return 1;
            case 2:
            case 3:
                d_active = false;
                d_events.push_back(d_state == 2 ? 1 : 2);
                d_state = 0;
                d_sample_counter += static_cast<uint64_t>(d_fft_size) * static_cast<uint64_t>(ninput_items);
                return ninput_items;
            }
        return 0;
    }

    //! messages published on the "events" port: 1 = ACQ_SUCCESS, 2 = ACQ_FAIL
    const std::vector<int>& events() const { return d_events; }
    void clear_events() { d_events.clear(); }
    float test_statistics() const { return d_test_statistics; }
    float input_power() const { return d_input_power; }
    const gc_acq_result& last_result() const { return d_last; }
    uint32_t fft_size() const { return d_fft_size; }
    uint32_t num_doppler_bins() const { return d_num_doppler_bins; }
    uint32_t dwell_count() const { return d_well_count; }
    int32_t state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    gc_status last_status() const { return d_status; }

private:
    void install_codes()
    {
        d_have_code = (d_status == GC_OK);
        if (d_acq != nullptr && d_status == GC_OK)
            d_status = gc_acq_set_local_code_pair(d_acq, 0, reinterpret_cast<const float*>(d_code_a.data()), reinterpret_cast<const float*>(d_code_b.data()));
    }

    // "restart acquisition variables" (set_state(1) and state 0 of both blocks)
    void restart()
    {
        d_gnss_synchro->Acq_delay_samples = 0.0;
        d_gnss_synchro->Acq_doppler_hz = 0.0;
        d_gnss_synchro->Acq_samplestamp_samples = 0ULL;
        d_gnss_synchro->Acq_doppler_step = 0U;
        d_well_count = 0;
        d_mag = 0.0;
        d_input_power = 0.0;
        d_test_statistics = 0.0;
    }

    // state 1: one dwell on one item
    void dwell(const gr_complex* in)
    {
        const float fft_normalization_factor = static_cast<float>(d_fft_size) * static_cast<float>(d_fft_size);
        if (d_kind == E1_8MS)
            {
                d_input_power = 0.0;  // 8ms :272-273
                d_mag = 0.0;
            }
        d_sample_counter += static_cast<uint64_t>(d_fft_size);
        d_well_count++;
        gc_acq_result r;
        std::memset(&r, 0, sizeof r);
        d_status = d_acq ? gc_acq_reset(d_acq) : GC_ERR_STATE;
        if (d_status == GC_OK) d_status = gc_acq_dwell(d_acq, reinterpret_cast<const float*>(in), &r);
        d_last = r;
        if (d_status == GC_OK)
            {
                d_input_power = r.input_power;
                // the largest of the bins' maxima, first bin on a tie, as the `d_mag < magt` scan of the Doppler loop leaves it
                const float magt = r.mag / (fft_normalization_factor * fft_normalization_factor);
                if (d_mag < magt)
                    {
                        d_mag = magt;
                        d_gnss_synchro->Acq_delay_samples = r.acq_delay_samples;
                        d_gnss_synchro->Acq_doppler_hz = r.acq_doppler_hz;
                        d_gnss_synchro->Acq_samplestamp_samples = d_sample_counter;
                        d_gnss_synchro->Acq_doppler_step = d_doppler_step;
                    }
                if (d_dump) dump_rows();
                d_test_statistics = d_mag / d_input_power;
            }
        if (d_status == GC_OK && d_test_statistics > d_threshold)
            d_state = 2;  // Positive acquisition
        else if (d_well_count == d_max_dwells)
            d_state = 3;  // Negative acquisition
    }

    void dump_rows()
    {
        std::vector<float> grid(static_cast<size_t>(d_num_doppler_bins) * d_fft_size);
        if (gc_acq_get_grid(d_acq, 0, grid.data()) != GC_OK) return;
        const size_t slash = d_dump_filename.find_last_of('/');
        const std::string dir = slash == std::string::npos ? std::string(".") : d_dump_filename.substr(0, slash);
        for (uint32_t b = 0; b < d_num_doppler_bins; b++)
            {
                const int32_t doppler = -static_cast<int32_t>(d_doppler_max) + static_cast<int32_t>(d_doppler_step * b);
                const std::string name = dir + "/test_statistics_" + std::string(1, d_gnss_synchro->System) + "_" + std::string(1, d_gnss_synchro->Signal[0]) +
                                         std::string(1, d_gnss_synchro->Signal[1]) + "_sat_" + std::to_string(d_gnss_synchro->PRN) + "_doppler_" + std::to_string(doppler) + ".dat";
                std::ofstream f(name, std::ios::out | std::ios::binary);
                f.write(reinterpret_cast<const char*>(&grid[static_cast<size_t>(b) * d_fft_size]), static_cast<std::streamsize>(sizeof(float) * d_fft_size));
            }
    }

    Kind d_kind;
    int64_t d_fs_in;
    int32_t d_samples_per_ms, d_samples_per_code;
    uint32_t d_sampled_ms, d_max_dwells, d_doppler_max;
    bool d_dump;
    std::string d_dump_filename;
    uint32_t d_fft_size = 0U, d_num_doppler_bins = 0U, d_doppler_step = 0U, d_channel = 0U, d_well_count = 0U;
    uint64_t d_sample_counter = 0ULL;
    int32_t d_state = 0;
    bool d_active = false, d_have_code = false;
    float d_threshold = 0.0f, d_mag = 0.0f, d_input_power = 0.0f, d_test_statistics = 0.0f;
    gc_acq* d_acq = nullptr;
    gc_status d_status = GC_OK;
    gc_acq_result d_last{};
    Gnss_Synchro* d_gnss_synchro = nullptr;
    std::vector<gr_complex> d_code_a, d_code_b;
    std::vector<int> d_events;
};

#endif  // GNSSCORR_HIP_PCPS_PAIRED_ACQUISITION_H_
