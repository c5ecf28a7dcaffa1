/*!
 * \file acquisition_block_base.h
 * \brief What the images of the reference's acquisition blocks share: the inclusive Doppler-bin count, owners of the library's
 * engines, the common part of gc_acq_conf, the clearing of Gnss_Synchro, and hip_acquisition_item_block -- the members, accessors
 * and state machine of the blocks that consume whole items (Tong, QuickSync, paired, E5a CAF).
 *
 * The item blocks of the reference are one machine with different numbers:
 *   state 0                 if active: "restart acquisition variables", go to the search state; count the items, consume them all;
 *   search state(s)         the block's own step (search()): it runs the dwell or dwells, sets the next state, returns the items consumed;
 *   positive / negative     clear d_active, publish 1 (ACQ_SUCCESS) / 2 (ACQ_FAIL) on "events", go to 0; count the items, consume them all.
 * What differs between them -- the state numbers, whether set_state(1) also activates, what a restart resets besides the common
 * fields, and everything inside the search step -- is a parameter (Policy) or an override, each with its reference line in the
 * block's own header.  The fine-Doppler block counts samples and has a machine of its own; it uses the helpers only.
 */
#ifndef GNSSCORR_ACQUISITION_BLOCK_BASE_H_
#define GNSSCORR_ACQUISITION_BLOCK_BASE_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include "hip_multicorrelator_real_codes.h"  // gnsscorr::shared_context()
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace gnsscorr
{
//! The blocks' "count the number of bins" loop: -doppler_max, -doppler_max + step, .. while <= +doppler_max, both ends counted.  64-bit
//! arithmetic, as the Tong and CAF copies had it: the 32-bit copies (paired, QuickSync, the adapters' threshold rule) wrapped once
//! doppler_max + doppler_step passed 2^31 and then counted garbage or did not end.  A step of 0 has no bins.
inline uint32_t inclusive_doppler_bins(uint32_t doppler_max, uint32_t doppler_step)
{
    if (doppler_step == 0) return 0;
    uint32_t n = 0;
    for (int64_t doppler = -static_cast<int64_t>(doppler_max); doppler <= static_cast<int64_t>(doppler_max); doppler += doppler_step) n++;
    return n;
}

struct AcqEngineDeleter
{
    void operator()(gc_acq* acq) const { gc_acq_destroy(acq); }
    void operator()(gc_fine_doppler* fine) const { gc_fine_doppler_destroy(fine); }
};
using AcqEngine = std::unique_ptr<gc_acq, AcqEngineDeleter>;
using FineDopplerEngine = std::unique_ptr<gc_fine_doppler, AcqEngineDeleter>;

//! Replaces the engine in `owner` by what create(ctx, &handle) makes on the shared context; GC_ERR_NO_DEVICE without one
template <class Handle, class Create>
inline gc_status create_engine(std::unique_ptr<Handle, AcqEngineDeleter>& owner, Create create)
{
    owner.reset();
    gc_ctx* ctx = shared_context();
    if (ctx == nullptr) return GC_ERR_NO_DEVICE;
    Handle* handle = nullptr;
    const gc_status status = create(ctx, &handle);
    owner.reset(handle);
    return status;
}

//! A zeroed gc_acq_conf with the fields every block sets; samples_per_chip = ceil(fs_in / chip_rate_hz)
inline gc_acq_conf acq_conf(int64_t fs_in, uint32_t sampled_ms, uint32_t ms_per_code, float samples_per_ms, float samples_per_code, double chip_rate_hz, uint32_t doppler_max,
    uint32_t doppler_step, uint32_t max_dwells)
{
    gc_acq_conf c;
    std::memset(&c, 0, sizeof c);
    c.fs_in = fs_in;
    c.sampled_ms = sampled_ms;
    c.ms_per_code = ms_per_code;
    c.samples_per_ms = samples_per_ms;
    c.samples_per_code = samples_per_code;
    c.samples_per_chip = static_cast<uint32_t>(std::ceil(static_cast<double>(fs_in) / chip_rate_hz));
    c.doppler_max = doppler_max;
    c.doppler_step = doppler_step;
    c.max_dwells = max_dwells;
    return c;
}

//! the fields "restart acquisition variables" clears in every block
inline void clear_synchro_for_restart(Gnss_Synchro& s)
{
    s.Acq_delay_samples = 0.0;
    s.Acq_doppler_hz = 0.0;
    s.Acq_samplestamp_samples = 0ULL;
    s.Acq_doppler_step = 0U;
}

//! the fields init() clears in every block
inline void clear_synchro_for_init(Gnss_Synchro& s)
{
    s.Flag_valid_acquisition = false;
    s.Flag_valid_symbol_output = false;
    s.Flag_valid_pseudorange = false;
    s.Flag_valid_word = false;
    clear_synchro_for_restart(s);
}
}  // namespace gnsscorr

class hip_acquisition_item_block
{
public:
    //! the block's state numbering, and whether set_state(1) sets d_active besides restarting
    struct Policy
    {
        int32_t search_first, search_last, positive, negative;
        bool set_state_activates;
    };

    virtual ~hip_acquisition_item_block() = default;

    inline void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_gnss_synchro = p_gnss_synchro; }
    inline uint32_t mag() const { return d_mag; }
    inline void set_active(bool active) { d_active = active; }
    inline void set_channel(uint32_t channel) { d_channel = channel; }
    inline void set_doppler_max(uint32_t doppler_max) { d_doppler_max = doppler_max; }
    inline void set_doppler_step(uint32_t doppler_step) { d_doppler_step = doppler_step; }
    virtual void set_threshold(float threshold) { d_threshold = threshold; }

    /*! init of every block: clears the synchro fields, (re)creates the engine and re-installs the code if there is one */
    void init()
    {
        gnsscorr::clear_synchro_for_init(*d_gnss_synchro);
        d_mag = 0.0;
        d_input_power = 0.0;
        d_acq.reset();
        d_status = create_engine();
        if (d_status == GC_OK && d_have_code) d_status = load_code();
    }

    void set_state(int32_t state)
    {
        d_state = state;
        if (d_state == 1)
            {
                restart();
                if (d_policy.set_state_activates) d_active = true;
            }
    }

    /*! general_work on host items of item_length() samples.  Returns the number of items consumed. */
    int work(const gr_complex* in, int ninput_items) { return step(in, nullptr, 0, ninput_items); }

    //! messages published on the "events" port: 1 = ACQ_SUCCESS, 2 = ACQ_FAIL
    const std::vector<int>& events() const { return d_events; }
    void clear_events() { d_events.clear(); }
    float test_statistics() const { return d_test_statistics; }
    float input_power() const { return d_input_power; }
    float threshold() const { return d_threshold; }
    const gc_acq_result& last_result() const { return d_last; }
    uint32_t fft_size() const { return d_fft_size; }
    uint32_t item_length() const { return d_item_length; }
    uint32_t num_doppler_bins() const { return d_num_doppler_bins; }
    uint32_t dwell_count() const { return d_dwell_count; }
    int32_t state() const { return d_state; }
    uint64_t sample_counter() const { return d_sample_counter; }
    gc_status last_status() const { return d_status; }
    gc_acq* engine() { return d_acq.get(); }

protected:
    hip_acquisition_item_block(const Policy& policy, uint32_t sampled_ms, uint32_t max_dwells, uint32_t doppler_max, int64_t fs_in, int32_t samples_per_ms, int32_t samples_per_code,
        bool dump, const std::string& dump_filename, uint32_t fft_size, uint32_t item_length, uint32_t doppler_step = 0U)
        : d_policy(policy), d_fs_in(fs_in), d_samples_per_ms(samples_per_ms), d_samples_per_code(samples_per_code), d_sampled_ms(sampled_ms), d_max_dwells(max_dwells), d_doppler_max(doppler_max), d_dump(dump), d_dump_filename(dump_filename), d_fft_size(fft_size), d_item_length(item_length), d_doppler_step(doppler_step)
    {
    }

    //! counts the bins and creates the engine in d_acq (make_engine() below); the status becomes last_status()
    virtual gc_status create_engine() = 0;
    //! installs the stored code in the engine
    virtual gc_status load_code() = 0;
    //! what "restart acquisition variables" resets besides the fields restart() clears
    virtual void on_restart() {}
    /*! the search state(s) on n_items items at `in`, or in `ring` from absolute sample first_index on when ring is not NULL: runs the
     *  dwell or dwells, counts them and their samples, sets the next state.  Returns the items consumed. */
    virtual int search(const gr_complex* in, gc_stream* ring, uint64_t first_index, int n_items) = 0;

    template <class Create>
    gc_status make_engine(Create create)
    {
        return gnsscorr::create_engine(d_acq, create);
    }

    //! the fields every block fills, with ms_per_code = sampled_ms: the blocks transform exactly the block they consume
    gc_acq_conf conf(double chip_rate_hz, uint32_t max_dwells) const
    {
        return gnsscorr::acq_conf(d_fs_in, d_sampled_ms, d_sampled_ms, static_cast<float>(d_samples_per_ms), static_cast<float>(d_samples_per_code), chip_rate_hz, d_doppler_max,
            d_doppler_step, max_dwells);
    }

    void reset_engine()
    {
        if (d_acq != nullptr) d_status = gc_acq_reset(d_acq.get());
    }

    void count_items(int n_items) { d_sample_counter += static_cast<uint64_t>(d_item_length) * static_cast<uint64_t>(n_items); }

    int step(const gr_complex* in, gc_stream* ring, uint64_t first_index, int n_items)
    {
        if (d_state == 0)
            {
                if (d_active)
                    {
                        restart();
                        d_state = d_policy.search_first;
                    }
                count_items(n_items);
                return n_items;
            }
        if (d_state >= d_policy.search_first && d_state <= d_policy.search_last) return search(in, ring, first_index, n_items);
        if (d_state == d_policy.positive || d_state == d_policy.negative)
            {
                d_active = false;
                d_events.push_back(d_state == d_policy.positive ? 1 : 2);
                d_state = 0;
                count_items(n_items);
                return n_items;
            }
        return 0;
    }

    const Policy d_policy;
    int64_t d_fs_in;
    int32_t d_samples_per_ms, d_samples_per_code;
    uint32_t d_sampled_ms, d_max_dwells, d_doppler_max;
    bool d_dump;
    std::string d_dump_filename;
    uint32_t d_fft_size, d_item_length, d_doppler_step;
    uint32_t d_num_doppler_bins = 0U, d_channel = 0U, d_dwell_count = 0U;
    uint64_t d_sample_counter = 0ULL;
    int32_t d_state = 0;
    bool d_active = false, d_have_code = false;
    float d_threshold = 0.0f, d_mag = 0.0f, d_input_power = 0.0f, d_test_statistics = 0.0f;
    gnsscorr::AcqEngine d_acq;
    gc_status d_status = GC_OK;
    gc_acq_result d_last{};
    Gnss_Synchro* d_gnss_synchro = nullptr;
    std::vector<int> d_events;

private:
    // "restart acquisition variables" (set_state(1) and state 0 of every block)
    void restart()
    {
        gnsscorr::clear_synchro_for_restart(*d_gnss_synchro);
        d_dwell_count = 0;
        d_mag = 0.0;
        d_input_power = 0.0;
        d_test_statistics = 0.0;
        on_restart();
    }
};

#endif  // GNSSCORR_ACQUISITION_BLOCK_BASE_H_
