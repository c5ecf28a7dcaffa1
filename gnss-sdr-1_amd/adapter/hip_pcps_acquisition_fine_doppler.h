/*!
 * \file hip_pcps_acquisition_fine_doppler.h
 * \brief Image of pcps_acquisition_fine_doppler_cc (src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition_fine_doppler_cc.{h,cc})
 * over a plain engine of libgnsscorr.so (gc_acq_create) for the grid and a fine Doppler stage (gc_fine_doppler_create) for
 * estimate_Doppler.  The AcquisitionInterface adapter in front of it is GpsL1CaPcpsAcquisitionFineDopplerHip
 * (pcps_acquisition_adapters.h).
 *
 * Contracts kept:
 *   - d_fft_size = samples_per_ms, whatever coherent_integration_time_ms says (:66); the grid has floor(2 * doppler_max / doppler_step)
 *     bins from -doppler_max on, which EXCLUDES +doppler_max (:158, :254) -- num_doppler_bins_override of the engine;
 *   - state 1 (:550-561): every d_fft_size samples are one dwell whose |.|^2 is added to the grid, unnormalised, and are kept in the
 *     10 ms buffer; max_dwells of them, then state 2;
 *   - state 2, compute_CAF (:266-335), on the host from gc_acq_get_grid, once per search: the first maximum with the bins ascending,
 *     a range of +-ceil(chip period * fs) samples around it in its row zeroed -- wrapped the block's way, an `else if` (:300-307), and
 *     from index 1 up to but EXCLUDING index 2 (:309-319) -- and the statistic first peak / second peak of that row; the synchro
 *     fields are written whatever the decision;
 *   - state 3 (:575-597): the buffer is filled up to 10 ms from the stream, then estimate_Doppler (:400-479) on the 10 ms that begin at
 *     the first dwell: GC_FINE_ALIGN_REFERENCE, the block's own rotate; 4 and 5 publish 1 (ACQ_SUCCESS) / 2 (ACQ_FAIL) on "events";
 *   - the sample counter advances by what every state consumes, nothing in states 2; blocking_on_standby (:544, :616, :640).
 *   - general_work(noutput_items, .., input_items, ..) becomes work(in, noutput_items), which returns the samples consumed.
 * Documented departures:
 *   - the block accepts the maximum of the WHOLE fine spectrum when it lies within 1 kHz of the grid's Doppler and keeps the grid's
 *     value otherwise; the stage computes the bins within 1 kHz only and reports their maximum.  The grid's value stays when that
 *     maximum is the window's first or last bin (GC_FINE_EDGE): a spectrum that still rises at the window's end has its maximum outside;
 *   - the block regenerates the GPS L1 C/A code of Gnss_Synchro::PRN for the wipe-off (:415); here the code given to set_local_code
 *     is used, which is that code in GpsL1CaPcpsAcquisitionFineDopplerHip;
 *   - max_dwells above 10 overruns nothing: the block's buffer holds 50 ms and so does this one, dwells beyond it are not kept;
 *   - `dump` is accepted and ignored (gc_acq_get_grid gives the grid).
 * The host-side pieces -- bin count, keys, compute_CAF with its wrap cases -- are checked without a GPU by `fine_doppler_selftest --host`.
 */
#ifndef GNSSCORR_HIP_PCPS_ACQUISITION_FINE_DOPPLER_H_
#define GNSSCORR_HIP_PCPS_ACQUISITION_FINE_DOPPLER_H_

#include "acquisition_block_base.h"  // engine owners, conf filler, synchro clearing
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gnsscorr
{
//! set_doppler_step (:158): +doppler_max is not searched
inline uint32_t fine_doppler_bins(uint32_t doppler_max, uint32_t doppler_step)
{
    if (doppler_step == 0) return 0;
    return static_cast<uint32_t>(std::floor(std::abs(2 * static_cast<int>(doppler_max)) / static_cast<double>(doppler_step)));
}

//! ceil(GPS_L1_CA_CHIP_PERIOD * float(fs)) (:295)
inline uint32_t fine_doppler_samples_per_chip(int64_t fs_in)
{
    return static_cast<uint32_t>(std::ceil((1.0 / 1.023e6) * static_cast<float>(fs_in)));
}

struct FineDopplerCaf
{
    int index_doppler = 0;
    uint32_t index_time = 0;
    float first_peak = 0.0f, second_peak = 0.0f, test_statistics = 0.0f;
};

/*! compute_CAF (:266-335) on grid[n_bins][fft_size]; the exclusion range is zeroed IN the grid, as the block does */
inline FineDopplerCaf fine_doppler_caf(float* grid, int n_bins, uint32_t fft_size, uint32_t samples_per_chip)
{
    FineDopplerCaf r;
    for (int i = 0; i < n_bins; i++)
        {
            const float* row = grid + static_cast<size_t>(i) * fft_size;
            uint32_t t = 0;
            for (uint32_t j = 1; j < fft_size; j++)
                if (row[j] > row[t]) t = j;
            if (row[t] > r.first_peak)
                {
                    r.first_peak = row[t];
                    r.index_doppler = i;
                    r.index_time = t;
                }
        }
    int32_t ex1 = static_cast<int32_t>(r.index_time) - static_cast<int32_t>(samples_per_chip);
    int32_t ex2 = static_cast<int32_t>(r.index_time) + static_cast<int32_t>(samples_per_chip);
    if (ex1 < 0)
        ex1 = static_cast<int32_t>(fft_size) + ex1;
    else if (ex2 >= static_cast<int32_t>(fft_size))
        ex2 = ex2 - static_cast<int32_t>(fft_size);
    float* row = grid + static_cast<size_t>(r.index_doppler) * fft_size;
    int32_t idx = ex1;
    uint32_t guard = 0;  // a transform shorter than the range would never meet index 2
    do
        {
            if (idx >= 0 && idx < static_cast<int32_t>(fft_size)) row[idx] = 0.0f;
            idx++;
            if (idx == static_cast<int32_t>(fft_size)) idx = 0;
        }
    while (idx != ex2 && ++guard < fft_size);
    uint32_t t = 0;
    for (uint32_t j = 1; j < fft_size; j++)
        if (row[j] > row[t]) t = j;
    r.second_peak = row[t];
    r.test_statistics = r.first_peak / r.second_peak;
    return r;
}
}  // namespace gnsscorr

class hip_pcps_acquisition_fine_doppler
{
public:
    static constexpr uint32_t kPrnReplicas = 10, kZeroPaddingFactor = 8, kBufferMs = 50;

    hip_pcps_acquisition_fine_doppler(uint32_t max_dwells, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms, bool blocking_on_standby, bool dump,
        const std::string& dump_filename)
        : d_fs_in(fs_in), d_samples_per_ms(samples_per_ms), d_max_dwells(max_dwells), d_config_doppler_max(doppler_max), d_blocking_on_standby(blocking_on_standby), d_dump(dump), d_dump_filename(dump_filename)
    {
        d_fft_size = static_cast<uint32_t>(d_samples_per_ms);
        d_code.assign(d_fft_size, gr_complex(0.0f, 0.0f));
        d_10_ms_buffer.assign(static_cast<size_t>(kBufferMs) * d_fft_size, gr_complex(0.0f, 0.0f));
    }

    inline void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    inline uint32_t mag() const { return static_cast<uint32_t>(d_test_statistics); }
    inline void set_active(bool active) { d_active = active; }
    inline void set_channel(uint32_t channel) { d_channel = channel; }
    inline void set_doppler_max(uint32_t doppler_max) { d_config_doppler_max = doppler_max; }
    inline void set_threshold(float threshold) { d_threshold = threshold; }

    /*! set_doppler_step (:153-172): sizes the grid */
    void set_doppler_step(uint32_t doppler_step)
    {
        d_doppler_step = doppler_step;
        d_num_doppler_points = gnsscorr::fine_doppler_bins(d_config_doppler_max, d_doppler_step);
    }

    /*! set_local_code (:199-205): d_fft_size samples */
    void set_local_code(std::complex<float>* code)
    {
        std::memcpy(d_code.data(), code, sizeof(gr_complex) * d_code.size());
        d_have_code = true;
        install_code();
    }

    /*! init (:208-219), and the engines: the block builds its grid in set_doppler_step and its transforms in the constructor */
    void init()
    {
        gnsscorr::clear_synchro_for_init(*d_gnss_synchro);
        d_state = 0;
        d_fine.reset();
        gc_acq_conf c = gnsscorr::acq_conf(d_fs_in, 1, 1, static_cast<float>(d_samples_per_ms), static_cast<float>(d_samples_per_ms), 1.023e6, d_config_doppler_max, d_doppler_step,
            std::max(1u, d_max_dwells));
        c.samples_per_chip = gnsscorr::fine_doppler_samples_per_chip(d_fs_in);  // the block's own rounding (:295), through float
        c.num_doppler_bins_override = d_num_doppler_points;
        // without a device GC_ERR_NO_DEVICE, whatever the grid; with one, a grid of no bins is GC_ERR_INVALID
        d_status = gnsscorr::create_engine(d_acq, [&](gc_ctx* ctx, gc_acq** acq) { return d_num_doppler_points > 0 ? gc_acq_create(ctx, &c, 1, acq) : GC_ERR_INVALID; });
        if (d_status != GC_OK) return;
        gc_fine_doppler_conf f;
        std::memset(&f, 0, sizeof f);
        f.fs_in = d_fs_in;
        f.samples_per_code = d_fft_size;
        f.prn_replicas = kPrnReplicas;
        f.zero_padding_factor = kZeroPaddingFactor;
        f.window_hz = 1000.0f;
        f.alignment = GC_FINE_ALIGN_REFERENCE;
        d_status = gnsscorr::create_engine(d_fine, [&](gc_ctx* ctx, gc_fine_doppler** fine) { return gc_fine_doppler_create(ctx, &f, 1, fine); });
        if (d_status == GC_OK) install_code();
    }

    /*! set_state (:490-513) */
    void set_state(int32_t state)
    {
        d_state = state;
        if (d_state == 1)
            {
                gnsscorr::clear_synchro_for_restart(*d_gnss_synchro);
                d_test_statistics = 0.0f;
                d_active = true;
                reset_grid();
            }
    }

    /*! general_work (:516-656): `in` holds noutput_items samples (at least item_length() of them in states 0 and 1, the block's
     *  forecast).  Returns the samples consumed. */
    int work(const gr_complex* in, int noutput_items)
    {
        const int fft = static_cast<int>(d_fft_size);
        switch (d_state)
            {
            case 0:
                if (d_active)
                    {
                        reset_grid();
                        d_n_samples_in_buffer = 0;
                        d_state = 1;
                    }
                return standby(fft);
            case 1:
                {
                    if (noutput_items < fft) return 0;
                    gc_acq_result r;
                    d_status = d_acq != nullptr ? gc_acq_dwell(d_acq.get(), reinterpret_cast<const float*>(in), &r) : GC_ERR_STATE;
                    if (d_n_samples_in_buffer + d_fft_size <= d_10_ms_buffer.size()) std::memcpy(&d_10_ms_buffer[d_n_samples_in_buffer], in, sizeof(gr_complex) * d_fft_size);
                    d_n_samples_in_buffer += d_fft_size;
                    d_well_count++;
                    if (d_well_count >= d_max_dwells) d_state = 2;
                    // a broken engine fails the search, so that it cannot hold a channel for ever
                    if (d_status != GC_OK) d_state = 5;
                    d_sample_counter += d_fft_size;
                    return fft;
                }
            case 2:
                {
                    d_grid.resize(static_cast<size_t>(d_num_doppler_points) * d_fft_size);
                    d_status = gc_acq_get_grid(d_acq.get(), 0, d_grid.data());
                    if (d_status != GC_OK)
                        {
                            d_state = 5;
                            return 0;
                        }
                    d_caf = gnsscorr::fine_doppler_caf(d_grid.data(), static_cast<int>(d_num_doppler_points), d_fft_size, gnsscorr::fine_doppler_samples_per_chip(d_fs_in));
                    d_test_statistics = d_caf.test_statistics;
                    d_gnss_synchro->Acq_delay_samples = static_cast<double>(d_caf.index_time);
                    d_gnss_synchro->Acq_doppler_hz = static_cast<double>(d_caf.index_doppler * static_cast<int>(d_doppler_step) - static_cast<int>(d_config_doppler_max));
                    d_gnss_synchro->Acq_samplestamp_samples = d_sample_counter;
                    d_gnss_synchro->Acq_doppler_step = d_doppler_step;
                    if (d_test_statistics > d_threshold)
                        d_state = 3;
                    else
                        {
                            d_state = 5;
                            d_n_samples_in_buffer = 0;
                        }
                    return 0;
                }
            case 3:
                {
                    const int64_t samples_remaining = static_cast<int64_t>(kPrnReplicas) * d_samples_per_ms - static_cast<int64_t>(d_n_samples_in_buffer);
                    if (samples_remaining > noutput_items)
                        {
                            std::memcpy(&d_10_ms_buffer[d_n_samples_in_buffer], in, sizeof(gr_complex) * static_cast<size_t>(noutput_items));
                            d_n_samples_in_buffer += static_cast<size_t>(noutput_items);
                            d_sample_counter += static_cast<uint64_t>(noutput_items);
                            return noutput_items;
                        }
                    int consumed = 0;
                    if (samples_remaining > 0)
                        {
                            std::memcpy(&d_10_ms_buffer[d_n_samples_in_buffer], in, sizeof(gr_complex) * static_cast<size_t>(samples_remaining));
                            d_sample_counter += static_cast<uint64_t>(samples_remaining);
                            consumed = static_cast<int>(samples_remaining);
                        }
                    estimate_Doppler();
                    d_n_samples_in_buffer = 0;
                    d_state = 4;
                    return consumed;
                }
            case 4:
            case 5:
                d_positive_acq = d_state == 4 ? 1 : 0;
                d_active = false;
                d_events.push_back(d_state == 4 ? 1 : 2);
                d_state = 0;
                return standby(noutput_items);
            default:
                d_state = 0;
                return standby(noutput_items);
            }
    }

    //! messages published on the "events" port: 1 = ACQ_SUCCESS, 2 = ACQ_FAIL
    const std::vector<int>& events() const { return d_events; }
    void clear_events() { d_events.clear(); }
    float test_statistics() const { return d_test_statistics; }
    float threshold() const { return d_threshold; }
    uint32_t fft_size() const { return d_fft_size; }
    uint32_t item_length() const { return d_fft_size; }
    uint32_t num_doppler_bins() const { return d_num_doppler_points; }
    uint32_t well_count() const { return d_well_count; }
    int32_t state() const { return d_state; }
    int32_t positive_acq() const { return d_positive_acq; }
    uint64_t sample_counter() const { return d_sample_counter; }
    gc_status last_status() const { return d_status; }
    const gnsscorr::FineDopplerCaf& caf() const { return d_caf; }
    //! the fine stage's record of the last positive search (status 0: it did not run)
    const gc_fine_doppler_result& fine_result() const { return d_fine_result; }
    gc_acq* engine() { return d_acq.get(); }
    gc_fine_doppler* fine_engine() { return d_fine.get(); }

private:
    int standby(int n)
    {
        if (d_blocking_on_standby) return 0;
        d_sample_counter += static_cast<uint64_t>(n);
        return n;
    }

    void install_code()
    {
        if (!d_have_code) return;
        if (d_acq != nullptr) d_status = gc_acq_set_local_code(d_acq.get(), 0, reinterpret_cast<const float*>(d_code.data()));
        if (d_fine != nullptr && d_status == GC_OK) d_status = gc_fine_doppler_set_code(d_fine.get(), 0, reinterpret_cast<const float*>(d_code.data()));
    }

    // reset_grid (:232-243): the engine's grid reads as zero after gc_acq_reset
    void reset_grid()
    {
        d_well_count = 0;
        if (d_acq != nullptr) d_status = gc_acq_reset(d_acq.get());
    }

    // estimate_Doppler (:400-479) on the buffer's first 10 ms
    void estimate_Doppler()
    {
        std::memset(&d_fine_result, 0, sizeof d_fine_result);
        if (d_fine == nullptr) return;
        gc_fine_doppler_request q;
        q.slot = 0;
        q.delay_samples = static_cast<uint32_t>(static_cast<int>(d_gnss_synchro->Acq_delay_samples));
        q.coarse_doppler_hz = d_gnss_synchro->Acq_doppler_hz;
        d_status = gc_fine_doppler_estimate(d_fine.get(), reinterpret_cast<const float*>(d_10_ms_buffer.data()), &q, 1, &d_fine_result);
        if (d_status == GC_OK && d_fine_result.status == GC_FINE_REFINED) d_gnss_synchro->Acq_doppler_hz = d_fine_result.doppler_hz;
    }

    int64_t d_fs_in;
    int32_t d_samples_per_ms;
    uint32_t d_max_dwells, d_config_doppler_max;
    bool d_blocking_on_standby, d_dump;
    std::string d_dump_filename;
    uint32_t d_fft_size = 0U, d_num_doppler_points = 0U, d_doppler_step = 0U, d_channel = 0U, d_well_count = 0U;
    size_t d_n_samples_in_buffer = 0;
    uint64_t d_sample_counter = 0ULL;
    int32_t d_state = 0, d_positive_acq = 0;
    bool d_active = false, d_have_code = false;
    float d_threshold = 0.0f, d_test_statistics = 0.0f;
    gnsscorr::AcqEngine d_acq;
    gnsscorr::FineDopplerEngine d_fine;
    gc_status d_status = GC_OK;
    gnsscorr::FineDopplerCaf d_caf;
    gc_fine_doppler_result d_fine_result{};
    Gnss_Synchro* d_gnss_synchro = nullptr;
    std::vector<gr_complex> d_code, d_10_ms_buffer;
    std::vector<float> d_grid;
    std::vector<int> d_events;
};

#endif  // GNSSCORR_HIP_PCPS_ACQUISITION_FINE_DOPPLER_H_
