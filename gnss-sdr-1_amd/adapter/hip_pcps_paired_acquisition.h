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
 * Documented departures:
 *   - the reference takes the maxima of the two hypotheses' rows separately and prefers the first (plus / A) on a tie (cccwsr
 *     :361-370, 8ms :336-345); the engine takes the row maximum of the per-sample maximum.  The two differ only if both hypotheses
 *     reach the identical float maximum at different indices;
 *   - `dump` writes, per Doppler bin, the combined |.|^2 row (fft_size float32) under the reference's file name
 *     test_statistics_<System>_<Signal>_sat_<PRN>_doppler_<Hz>.dat in the directory of dump_filename; the reference writes the last
 *     inverse transform's complex output there (cccwsr :383-394);
 *   - a doppler_step of 0 (init() before set_doppler_step) has no bins; the blocks' loop would not end.  init() leaves no engine,
 *     last_status() is GC_ERR_INVALID and the search fails after max_dwells items.
 * The host-side pieces -- bin count, the step-0 refusals of block and adapter -- are checked without a GPU by
 * `paired_acquisition_selftest --host`.
 */
#ifndef GNSSCORR_HIP_PCPS_PAIRED_ACQUISITION_H_
#define GNSSCORR_HIP_PCPS_PAIRED_ACQUISITION_H_

#include "acquisition_block_base.h"
#include <cmath>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

class hip_pcps_paired_acquisition : public hip_acquisition_item_block
{
public:
    enum Kind
    {
        CCCWSR,  //!< pcps_cccwsr_acquisition_cc: set_local_code(data, pilot)
        E1_8MS   //!< galileo_pcps_8ms_acquisition_cc: set_local_code(code)
    };

    // general_work (cccwsr :243-468, 8ms :229-442): search state 1, positive 2, negative 3; set_state(1) restarts and leaves d_active alone
    hip_pcps_paired_acquisition(Kind kind, uint32_t sampled_ms, uint32_t max_dwells, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms,
        int32_t samples_per_code, bool dump, const std::string& dump_filename)
        : hip_acquisition_item_block(Policy{1, 1, 2, 3, false}, sampled_ms, max_dwells, doppler_max, fs_in, samples_per_ms, samples_per_code, dump, dump_filename,
              sampled_ms * samples_per_ms, sampled_ms * samples_per_ms),
          d_kind(kind)
    {
        d_code_a.assign(d_fft_size, gr_complex(0.0f, 0.0f));
        d_code_b.assign(d_fft_size, gr_complex(0.0f, 0.0f));
    }

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

private:
    void install_codes()
    {
        d_have_code = (d_status == GC_OK);
        if (d_acq != nullptr && d_status == GC_OK) d_status = load_code();
    }

    // init (cccwsr :182-216, 8ms :169-202): counts the bins, both ends of the range, and creates the engine whose wipe-off table is the
    // blocks' volk_gnsssdr_s32f_sincos_32fc grid.  A step of 0 has no bins: GC_ERR_INVALID and no engine
    gc_status create_engine() override
    {
        d_num_doppler_bins = gnsscorr::inclusive_doppler_bins(d_doppler_max, d_doppler_step);
        if (d_num_doppler_bins == 0) return GC_ERR_INVALID;
        gc_acq_conf c = conf(1.023e6, 1);
        c.use_CFAR_algorithm_flag = 1;
        c.num_doppler_bins_override = d_num_doppler_bins;
        return make_engine([&](gc_ctx* ctx, gc_acq** acq) { return gc_acq_create_paired(ctx, &c, 1, GC_ACQ_COMBINE_MAX, acq); });
    }

    gc_status load_code() override
    {
        return gc_acq_set_local_code_pair(d_acq.get(), 0, reinterpret_cast<const float*>(d_code_a.data()), reinterpret_cast<const float*>(d_code_b.data()));
    }

    // state 1: one dwell on one item, whatever n_items says; the counter and the dwell count advance BEFORE the dwell.  A restart
    // leaves the engine alone: gc_acq_reset runs inside every dwell.  On an engine error the search stays in state 1 until the dwell
    // count reaches max_dwells, then fails
    int search(const gr_complex* in, gc_stream*, uint64_t, int) override
    {
        const float fft_normalization_factor = static_cast<float>(d_fft_size) * static_cast<float>(d_fft_size);
        if (d_kind == E1_8MS)
            {
                d_input_power = 0.0;  // 8ms :272-273
                d_mag = 0.0;
            }
        count_items(1);
        d_dwell_count++;
        gc_acq_result r;
        std::memset(&r, 0, sizeof r);
        d_status = d_acq ? gc_acq_reset(d_acq.get()) : GC_ERR_STATE;
        if (d_status == GC_OK) d_status = gc_acq_dwell(d_acq.get(), reinterpret_cast<const float*>(in), &r);
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
        else if (d_dwell_count == d_max_dwells)
            d_state = 3;  // Negative acquisition
        return 1;
    }

    void dump_rows()
    {
        std::vector<float> grid(static_cast<size_t>(d_num_doppler_bins) * d_fft_size);
        if (gc_acq_get_grid(d_acq.get(), 0, grid.data()) != GC_OK) return;
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
    std::vector<gr_complex> d_code_a, d_code_b;
};


#endif  // GNSSCORR_HIP_PCPS_PAIRED_ACQUISITION_H_
