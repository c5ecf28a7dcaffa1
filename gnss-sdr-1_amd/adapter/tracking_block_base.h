/*!
 * \file tracking_block_base.h
 * \brief What the tracking blocks and groups on the DEVICE loop (gc_trk_loop) share.  A block is one channel with a ring of its own:
 * work() pushes the new input items into the ring, runs every code period that is complete in it in one launch and turns the
 * records into Gnss_Synchro items (hip_device_loop_block).  A group is N channel slots on a ring somebody else fills: run() does the
 * same for all active slots in one launch (hip_loop_group_base).  The arithmetic of both -- how many items still go into the ring,
 * how many periods a launch asks for, how a channel's records are walked -- is three free functions without a library call.
 *
 * The veml loop (gc_trk_loop_start) and the GLONASS loop (gc_trk_loop_start_glonass) differ in how a launch reports the end of its
 * input, in the item of the pull-in alignment and in who puts an engine slot back in standby; that is the Policy.  What a start
 * does and what a record becomes are the hooks of the concrete class.
 */
#ifndef GNSSCORR_TRACKING_BLOCK_BASE_H_
#define GNSSCORR_TRACKING_BLOCK_BASE_H_

#include "gnss_sdr_types.h"
#include "gnsscorr.h"
#include <algorithm>
#include <mutex>
#include <vector>

namespace gnsscorr
{
struct TrkLoopPolicy
{
    /*! GLONASS: the first record with valid == 0 is the end of the input.  veml: pull-in and integrating periods have valid == 0 too
     *  and are consumed without an item; the input ends at a record that did not advance (state >= 2, sample_counter unchanged) */
    bool invalid_record_ends_input;
    //! GLONASS: the alignment writes an item of its own, first after a start
    bool pull_in_item;
    //! GLONASS: gc_trk_loop_stop on loss of lock, and in a block's stop_tracking.  The veml block never stops its slot, the veml group
    //! only in stop_tracking and before a restart (as every group does)
    bool stops_engine_slot;
};
constexpr TrkLoopPolicy kVemlLoopPolicy = {false, false, false};
constexpr TrkLoopPolicy kGlonassLoopPolicy = {true, true, true};

/*! Ring feed plan of a block: of the ninput_items the scheduler shows, `have` are in the ring already (pushed, not yet consumed: it
 *  shows again what was not consumed last time).  Returns how many of the others go in now: what the ring has room for. */
inline uint64_t ring_feed_fresh(int ninput_items, uint64_t have, uint64_t ring_capacity)
{
    const uint64_t fresh = static_cast<uint64_t>(ninput_items) > have ? static_cast<uint64_t>(ninput_items) - have : 0;
    return std::min(fresh, ring_capacity - have);
}

//! Launch size of a block: every period that may be complete in the ring, as far as the output (out_room items left) and the record buffer go
inline int block_launch_periods(int out_room, size_t n_records, uint64_t pushed, uint64_t sample_counter, uint32_t vector_length)
{
    return std::min<int>(std::min<int>(out_room, static_cast<int>(n_records)), static_cast<int>((pushed - sample_counter) / vector_length) + 1);
}

//! Launch size of a group: the most periods any active slot may have complete below the ring's head (a mixed group sizes the launch
//! for its shortest code period); 0: nothing to run
template <class VectorLengthOf>
inline int group_launch_periods(uint64_t head, const std::vector<char>& active, const std::vector<uint64_t>& position, VectorLengthOf vector_length_of)
{
    int n_periods = 0;
    for (size_t ch = 0; ch < active.size(); ch++)
        if (active[ch] && head > position[ch]) n_periods = std::max<int>(n_periods, static_cast<int>((head - position[ch]) / vector_length_of(static_cast<int>(ch))) + 1);
    return n_periods;
}

struct RecordWalk
{
    uint64_t position;           //!< stream sample up to which the channel has consumed
    const gc_loop_record* last;  //!< the last record consumed (its state is the channel's), NULL: none
    bool lost;                   //!< that record reported loss of lock (state 0): event 3, nothing behind it was read
};

/*! The n records of one channel from one launch, the channel being at `position`: stops at the end of the input (the launch marks the
 *  periods that were not complete), calls emit(record) for every valid period -- under invalid_record_ends_input that is every
 *  record before the end -- and stops behind the record that lost lock, whose item is still handed out. */
template <class Emit>
inline RecordWalk walk_records(const TrkLoopPolicy& policy, const gc_loop_record* records, int n, uint64_t position, Emit emit)
{
    RecordWalk w = {position, nullptr, false};
    for (int k = 0; k < n && !w.lost; k++)
        {
            const gc_loop_record& r = records[k];
            if (policy.invalid_record_ends_input ? r.valid == 0 : (r.sample_counter == w.position && r.valid == 0 && r.state >= 2)) break;
            w.position = r.sample_counter;
            w.last = &r;
            if (r.valid) emit(r);
            w.lost = r.state == 0;
        }
    return w;
}
}  // namespace gnsscorr

class hip_device_loop_block
{
public:
    virtual ~hip_device_loop_block()
    {
        if (d_loop) gc_trk_loop_destroy(d_loop);
        if (d_ring) gc_stream_destroy(d_ring);
        if (d_ctx) gc_ctx_destroy(d_ctx);
    }
    hip_device_loop_block(const hip_device_loop_block&) = delete;
    hip_device_loop_block& operator=(const hip_device_loop_block&) = delete;

    void set_channel(uint32_t channel) { d_channel = channel; }
    void set_gnss_synchro(Gnss_Synchro* p_gnss_synchro) { d_acquisition_gnss_synchro = p_gnss_synchro; }

    //! start_tracking of the reference block, on the device; a failure is sticky (last_status())
    void start_tracking()
    {
        std::lock_guard<std::mutex> l(d_setlock);
        if (d_status != GC_OK) return;
        d_status = start_channel(d_sample_counter, d_policy.pull_in_item ? &d_pull_in_item : nullptr);
        d_state = d_status == GC_OK ? 1 : 0;
        d_pull_in = d_policy.pull_in_item && d_status == GC_OK;
    }

    void stop_tracking()
    {
        std::lock_guard<std::mutex> l(d_setlock);
        if (d_policy.stops_engine_slot && d_state != 0 && d_loop) gc_trk_loop_stop(d_loop, 0);
        d_state = 0;
    }

    //! forecast: like the reference blocks, two code periods
    int required_input_items() const { return static_cast<int>(d_vector_length) * 2; }

    /*! general_work: `in` points at the first unconsumed item, ninput_items are available, at most max_out Gnss_Synchro fit in
     *  `out`.  Returns the items consumed; *produced = Gnss_Synchro written: the pull-in item if there is one, then one per valid period. */
    int work(const gr_complex* in, int ninput_items, Gnss_Synchro* out, int max_out, int* produced)
    {
        std::lock_guard<std::mutex> l(d_setlock);
        *produced = 0;
        if (d_state == 0 || d_status != GC_OK)
            {
                // standby: the items pass by (they are not needed in HBM), the counters move on
                d_sample_counter += static_cast<uint64_t>(ninput_items);
                d_pushed = std::max(d_pushed, d_sample_counter);
                return ninput_items;
            }
        // 1. the items that are not in the ring yet
        const uint64_t have = d_pushed - d_sample_counter;
        const uint64_t fresh = gnsscorr::ring_feed_fresh(ninput_items, have, static_cast<uint64_t>(d_vector_length) * d_ring_periods);
        if (fresh > 0)
            {
                // items went by in standby: the ring's numbering continues at the stream position (zeros fill the gap)
                if (d_ring_head != d_pushed) d_status = skip_to(d_pushed);
                if (d_status == GC_OK) d_status = gc_stream_push(d_ring, in + have, fresh, nullptr);
                if (d_status != GC_OK) return 0;
                d_pushed += fresh;
                d_ring_head = d_pushed;
            }
        if (d_pull_in && max_out > 0)
            {
                out[(*produced)++] = d_pull_in_item;
                d_pull_in = false;
            }
        // 2. every complete code period in one launch
        const int n_periods = gnsscorr::block_launch_periods(max_out - *produced, d_records.size(), d_pushed, d_sample_counter, d_vector_length);
        if (n_periods <= 0) return 0;
        d_status = gc_trk_loop_run(d_loop, n_periods, d_records.data());
        if (d_status != GC_OK) return 0;
        // 3. records -> Gnss_Synchro; the launch stops at the first period that is not complete
        const gnsscorr::RecordWalk w = gnsscorr::walk_records(d_policy, d_records.data(), n_periods, d_sample_counter, [&](const gc_loop_record& r) { out[(*produced)++] = to_synchro(r); });
        if (w.last)
            {
                d_state = w.last->state;
                d_last = *w.last;
            }
        if (w.lost)
            {
                d_events.push_back(3);  // loss of lock
                if (d_policy.stops_engine_slot) gc_trk_loop_stop(d_loop, 0);
            }
        const int consumed = static_cast<int>(w.position - d_sample_counter);
        d_sample_counter = w.position;
        return consumed;
    }

    bool tracking_enabled() const { return d_state != 0; }
    int32_t state() const { return d_state; }
    double carrier_doppler_hz() const { return d_last.carrier_doppler_hz; }
    double code_freq_chips() const { return d_last.code_freq_chips; }
    double cn0_db_hz() const { return d_last.cn0_db_hz; }
    double carrier_lock_test() const { return d_last.carrier_lock_test; }
    uint64_t sample_counter() const { return d_sample_counter; }
    const gc_loop_record& last_record() const { return d_last; }
    const std::vector<int>& events() const { return d_events; }
    gc_status last_status() const { return d_status; }

protected:
    /*! ring_periods: code periods of vector_length items the HBM ring holds (a work() call may bring at most that many);
     *  precondition: what the concrete constructor found wrong before anything is created (it becomes last_status()) */
    hip_device_loop_block(const gnsscorr::TrkLoopPolicy& policy, uint32_t vector_length, int max_code_length, int device, int ring_periods, gc_status precondition = GC_OK)
        : d_policy(policy), d_vector_length(vector_length), d_ring_periods(ring_periods), d_status(precondition)
    {
        if (d_status == GC_OK) d_status = gc_ctx_create(device, &d_ctx);
        if (d_status == GC_OK) d_status = gc_stream_create(d_ctx, GC_IQ_F32, static_cast<uint64_t>(vector_length) * ring_periods, 2 * vector_length, &d_ring);
        if (d_status == GC_OK) d_status = gc_trk_loop_create(d_ctx, 1, max_code_length, &d_loop);
        if (d_status == GC_OK) d_status = gc_trk_loop_set_input_stream(d_loop, 0, d_ring);
        d_records.resize(ring_periods + 2);
    }

    //! starts slot 0 of d_loop on *d_acquisition_gnss_synchro at stream sample `sample_counter`; *pull_in (not NULL with
    //! Policy::pull_in_item) receives the item of the alignment
    virtual gc_status start_channel(uint64_t sample_counter, Gnss_Synchro* pull_in) = 0;
    //! what a valid period hands to the telemetry decoder
    virtual Gnss_Synchro to_synchro(const gc_loop_record& r) const = 0;

    const gnsscorr::TrkLoopPolicy d_policy;
    const uint32_t d_vector_length;
    const int d_ring_periods;
    std::mutex d_setlock;
    gc_ctx* d_ctx = nullptr;
    gc_stream* d_ring = nullptr;
    gc_trk_loop* d_loop = nullptr;
    gc_status d_status;
    Gnss_Synchro* d_acquisition_gnss_synchro = nullptr;
    uint32_t d_channel = 0;
    int32_t d_state = 0;

private:
    //! appends zeros until the ring's head is at absolute sample `index`
    gc_status skip_to(uint64_t index)
    {
        std::vector<gr_complex> zeros(std::min<uint64_t>(index - d_ring_head, 1u << 16));
        while (d_ring_head < index)
            {
                const uint64_t n = std::min<uint64_t>(index - d_ring_head, zeros.size());
                gc_status s = gc_stream_push(d_ring, zeros.data(), n, nullptr);
                if (s != GC_OK) return s;
                d_ring_head += n;
            }
        return GC_OK;
    }

    Gnss_Synchro d_pull_in_item{};
    bool d_pull_in = false;
    uint64_t d_sample_counter = 0;  // absolute index of the first unconsumed item (the block's d_sample_counter)
    uint64_t d_pushed = 0;          // absolute index one past the last item seen
    uint64_t d_ring_head = 0;       // absolute index one past the last item in the ring
    std::vector<gc_loop_record> d_records;
    gc_loop_record d_last{};
    std::vector<int> d_events;
};

class hip_loop_group_base
{
public:
    virtual ~hip_loop_group_base()
    {
        if (d_loop) gc_trk_loop_destroy(d_loop);
    }
    hip_loop_group_base(const hip_loop_group_base&) = delete;
    hip_loop_group_base& operator=(const hip_loop_group_base&) = delete;

    /*! Channel slot `ch` starts tracking the satellite of `acq` (PRN, Acq_delay_samples, Acq_doppler_hz, Acq_samplestamp_samples) at
     *  stream sample `start_index` -- any resident sample; the pull-in aligns the first code period after it.  A slot that was running
     *  is stopped first: a restart that fails leaves it inactive. */
    gc_status start_tracking(int ch, const Gnss_Synchro& acq, uint64_t start_index)
    {
        std::lock_guard<std::mutex> l(d_mutex);
        if (d_loop == nullptr) return d_status;  // construction failed
        if (ch < 0 || ch >= d_n) return GC_ERR_INVALID;
        if (d_active[ch]) gc_trk_loop_stop(d_loop, ch);
        d_active[ch] = 0;
        const gc_status st = start_slot(ch, acq, start_index, d_policy.pull_in_item ? &d_pull_in_item[ch] : nullptr);
        if (st != GC_OK) return st;
        d_acq[ch] = acq;
        d_active[ch] = 1;
        d_pull_in[ch] = d_policy.pull_in_item;
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

    /*! Every complete code period of every active slot, one launch; out[ch] receives the slot's Gnss_Synchro items (appended): the
     *  pull-in item if there is one (also when no launch follows), then one per valid period.  Returns the number of items produced
     *  over all slots, or -1 (last_status()). */
    int run(std::vector<std::vector<Gnss_Synchro>>& out)
    {
        std::lock_guard<std::mutex> l(d_mutex);
        if (d_loop == nullptr) return -1;  // construction failed; a failed run() is NOT sticky: the next call tries again
        out.resize(d_n);
        uint64_t head = 0;
        gc_stream_info(d_ring, nullptr, &head, nullptr);
        int produced = 0;
        for (int ch = 0; ch < d_n; ch++)
            if (d_active[ch] && d_pull_in[ch])
                {
                    out[ch].push_back(d_pull_in_item[ch]);
                    d_pull_in[ch] = 0;
                    produced++;
                }
        const int n_periods = gnsscorr::group_launch_periods(head, d_active, d_position, [this](int ch) { return vector_length_of(ch); });
        if (n_periods == 0) return produced;
        d_records.resize(static_cast<size_t>(d_n) * n_periods);
        d_status = gc_trk_loop_run(d_loop, n_periods, d_records.data());
        // e.g. a slot that was not serviced in time fell behind the ring (GC_ERR_STATE): the caller parks that slot (stop_tracking / a
        // new start_tracking) and goes on; the other slots are unaffected
        if (d_status != GC_OK) return -1;
        for (int ch = 0; ch < d_n; ch++)
            {
                if (!d_active[ch]) continue;
                const gnsscorr::RecordWalk w = gnsscorr::walk_records(d_policy, &d_records[static_cast<size_t>(ch) * n_periods], n_periods, d_position[ch], [&](const gc_loop_record& r) {
                    out[ch].push_back(to_synchro(ch, r));
                    produced++;
                });
                if (w.lost)
                    {
                        d_events[ch].push_back(3);  // loss of lock: the slot is free for the next acquisition
                        d_active[ch] = 0;
                        if (d_policy.stops_engine_slot) gc_trk_loop_stop(d_loop, ch);
                    }
                d_position[ch] = w.position;
            }
        return produced;
    }

    int n_channels() const { return d_n; }
    bool active(int ch) const { return d_active[ch] != 0; }
    //! stream sample up to which slot `ch` has consumed (a producer may evict everything before the minimum over the slots)
    uint64_t position(int ch) const { return d_position[ch]; }
    const std::vector<int>& events(int ch) const { return d_events[ch]; }
    gc_status last_status() const { return d_status; }

protected:
    hip_loop_group_base(const gnsscorr::TrkLoopPolicy& policy, gc_stream* ring) : d_policy(policy), d_ring(ring) {}

    //! the engine of d_n slots on the ring (a mixed engine when the slots are not all one signal) and the slot bookkeeping
    void create_loop(gc_ctx* ctx, int max_code_length, int iq_format, bool mixed)
    {
        d_status = gc_trk_loop_create(ctx, d_n, max_code_length, &d_loop);
        if (d_status == GC_OK && mixed) d_status = gc_trk_loop_set_mixed(d_loop, 1);
        if (d_status == GC_OK) d_status = gc_trk_loop_set_input_format(d_loop, iq_format);
        for (int ch = 0; ch < d_n && d_status == GC_OK; ch++) d_status = gc_trk_loop_set_input_stream(d_loop, ch, d_ring);
        d_acq.resize(d_n);
        d_pull_in_item.resize(d_n);
        d_pull_in.assign(d_n, 0);
        d_active.assign(d_n, 0);
        d_position.assign(d_n, 0);
        d_events.resize(d_n);
    }

    //! starts slot `ch` of d_loop at stream sample start_index; *pull_in (not NULL with Policy::pull_in_item) receives the item of the alignment
    virtual gc_status start_slot(int ch, const Gnss_Synchro& acq, uint64_t start_index, Gnss_Synchro* pull_in) = 0;
    //! the slot's code period in samples
    virtual uint32_t vector_length_of(int ch) const = 0;
    //! what a valid period of slot `ch` hands to the telemetry decoder
    virtual Gnss_Synchro to_synchro(int ch, const gc_loop_record& r) const = 0;

    const gnsscorr::TrkLoopPolicy d_policy;
    gc_stream* d_ring;
    gc_trk_loop* d_loop = nullptr;
    int d_n = 0;
    gc_status d_status = GC_OK;
    std::vector<Gnss_Synchro> d_acq;

private:
    std::mutex d_mutex;
    std::vector<Gnss_Synchro> d_pull_in_item;
    std::vector<char> d_pull_in, d_active;
    std::vector<uint64_t> d_position;
    std::vector<std::vector<int>> d_events;
    std::vector<gc_loop_record> d_records;
};

#endif  // GNSSCORR_TRACKING_BLOCK_BASE_H_
