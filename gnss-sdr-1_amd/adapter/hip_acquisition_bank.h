/*!
 * \file hip_acquisition_bank.h
 * \brief The acquisition stage of a whole constellation as ONE object on the RF stream ring: the counterpart of hip_tracking_group.
 *
 * In the reference every channel owns a pcps_acquisition block that searches ONE satellite at a time on its copy of the input
 * (channel.cc:59-115, pcps_acquisition.cc:668-927).  Here one engine (gc_acq) holds the replicas of every PRN of a signal, and a
 * search(first_index) call runs the same PCPS search -- wipe-off, FFT, x conj(FFT(code)), IFFT, |.|^2, statistic -- for ALL of them on
 * the samples already resident in the ring (the Doppler wipe-off and the forward FFT of the input are computed once per bin and
 * shared by the satellites), and returns a Gnss_Synchro with the Acq_* fields of every satellite above the threshold, ready for
 * hip_tracking_group::start_tracking.  Sizes, thresholds and the result mapping are those of the reference adapters
 * (pcps_acquisition_adapters.h); GPS L1 C/A, L5I, Galileo E1 B / C, E5a, BeiDou B1I, B3I.
 *
 * use_acquisition_resampler (GNSS-SDR.use_acquisition_resampler, gnss_flowgraph.cc:375-499): the bank derives a decimated ring from
 * `ring` on the device (hip_ring_decimator.h) at about the signal's optimal search rate -- GPS_L1_CA_OPT_ACQ_FS_HZ 1 000 000,
 * GPS_L5_OPT_ACQ_FS_HZ 10 000 000, GALILEO_E1_OPT_ACQ_FS_HZ 2 000 000, GALILEO_E5A_OPT_ACQ_FS_HZ 10 000 000, none for BeiDou -- builds
 * engine and replicas at that rate, and scales delay and sample stamp back to the ring's rate as pcps_acquisition.cc:756-762 does.
 * Everything the caller sees stays at the ring's rate; tracking stays on `ring`.  When the plan's decimation is 1 the flag does
 * nothing.  Deviation: the reference switches the resampler off for item types other than gr_complex; here every ring format works.
 *
 * cccwsr (Galileo E1 "1B" only): every satellite is searched on BOTH components the way pcps_cccwsr_acquisition_cc does (:316-370,
 * data and pilot correlations combined as d + jp and d - jp, the larger wins) -- a paired MAX engine (gc_acq_create_paired) whose slots
 * hold gc_cccwsr_replicas(E1-B, E1-C); statistic, threshold and result mapping stay those of the one-replica search.
 *
 * fine_doppler: after a search the detections -- and only they -- are refined in ONE call of the fine Doppler stage
 * (gc_fine_doppler_estimate_stream, the estimate_Doppler of pcps_acquisition_fine_doppler_cc): on the ring the search read and at
 * that ring's rate, over the 10 code periods that begin at the first dwell's first sample, zero padding 8, with
 * GC_FINE_ALIGN_EXACT.  Acq_doppler_hz becomes the fine value (fs / (80 samples per code): 12.5 Hz for a 1 ms code) unless the stage
 * reports GC_FINE_EDGE; fine_result() gives the stage's record.  The ring must hold those 10 code periods: when it does not (or the
 * stage fails otherwise) the detections keep their coarse Doppler and last_status() is the stage's error.  With the flag off
 * nothing changes.
 */
#ifndef GNSSCORR_HIP_ACQUISITION_BANK_H_
#define GNSSCORR_HIP_ACQUISITION_BANK_H_

#include "gnss_sdr_types.h"
#include "hip_ring_decimator.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

class hip_acquisition_bank
{
public:
    /*! system / signal: 'G' "1C" | "L5", 'E' "1B" | "5X", 'C' "B1" | "B3"; prns: the satellites searched; fs_in: the ring's sampling rate;
     *  doppler_max / doppler_step [Hz]; threshold on the block's statistic (pcps_acquisition.cc:565-665); max_dwells non-coherent dwells */
    hip_acquisition_bank(gc_ctx* ctx, gc_stream* ring, char system, const std::string& signal, const std::vector<uint32_t>& prns, int64_t fs_in, uint32_t doppler_max,
        uint32_t doppler_step, float threshold, uint32_t max_dwells = 1, bool use_cfar = true, int iq_format = GC_IQ_F32, bool use_acquisition_resampler = false,
        bool cccwsr = false, bool fine_doppler = false)
        : d_ring(ring), d_acq_ring(ring), d_system(system), d_signal(signal), d_prns(prns), d_threshold(threshold), d_max_dwells(std::max(1u, max_dwells))
    {
        double code_rate = 1.023e6, code_len = 1023.0;
        uint32_t ms_per_code = 1, opt_acq_fs = 0;
        if (system == 'G' && signal == "1C") { opt_acq_fs = 1000000; }
        else if (system == 'G' && signal == "L5") { code_rate = 10.23e6; code_len = 10230.0; opt_acq_fs = 10000000; }
        else if (system == 'E' && signal == "1B") { code_len = 4092.0; ms_per_code = 4; opt_acq_fs = 2000000; }
        else if (system == 'E' && signal == "5X") { code_rate = 1.023e7; code_len = 10230.0; opt_acq_fs = 10000000; }
        else if (system == 'C' && signal == "B1") { code_rate = 2.046e6; code_len = 2046.0; }
        else if (system == 'C' && signal == "B3") { code_rate = 10.23e6; code_len = 10230.0; }
        else
            {
                d_status = GC_ERR_INVALID;
                return;
            }
        if (use_acquisition_resampler)
            {
                // the search runs on a derived ring at resampled_fs, gr_complex whatever the source's item type
                d_resampler.reset(new hip_ring_decimator(ctx, ring, fs_in, opt_acq_fs));
                d_status = d_resampler->last_status();
                if (d_status != GC_OK) return;
                if (d_resampler->enabled())
                    {
                        d_ratio = d_resampler->decimation();
                        d_latency = d_resampler->latency();
                        fs_in = d_resampler->resampled_fs();
                        iq_format = GC_IQ_F32;
                    }
                else
                    d_resampler.reset();
            }
        gc_acq_conf c;
        std::memset(&c, 0, sizeof c);
        c.fs_in = fs_in;
        c.sampled_ms = ms_per_code;
        c.ms_per_code = ms_per_code;
        c.samples_per_ms = static_cast<float>(fs_in) * 0.001f;
        c.samples_per_code = c.samples_per_ms * static_cast<float>(ms_per_code);
        c.samples_per_chip = static_cast<uint32_t>(std::ceil((1.0 / code_rate) * static_cast<float>(fs_in)));
        if (system == 'C')
            {
                // the BeiDou adapters leave ms_per_code and samples_per_chip at Acq_Conf's zeros and count in code lengths
                // (beidou_b1i_pcps_acquisition.cc:73-104): the block then doubles its FFT (pcps_acquisition.cc:78-85)
                c.ms_per_code = 0;
                c.samples_per_chip = 0;
                c.samples_per_ms = static_cast<float>(std::round(static_cast<double>(fs_in) / (code_rate / code_len)));
                c.samples_per_code = c.samples_per_ms;
            }
        c.doppler_max = doppler_max;
        c.doppler_step = doppler_step;
        c.max_dwells = d_max_dwells;
        c.use_CFAR_algorithm_flag = use_cfar ? 1 : 0;
        cccwsr = cccwsr && system == 'E' && signal == "1B";
        d_status = cccwsr ? gc_acq_create_paired(ctx, &c, static_cast<int>(prns.size()), GC_ACQ_COMBINE_MAX, &d_acq) : gc_acq_create(ctx, &c, static_cast<int>(prns.size()), &d_acq);
        if (d_status == GC_OK && iq_format != GC_IQ_F32) d_status = gc_acq_set_input_format(d_acq, iq_format);
        if (d_status != GC_OK) return;
        uint32_t fft = 0, consumed = 0, bins = 0;
        gc_acq_fft_size(d_acq, &fft, &consumed, &bins);
        d_consumed = consumed;
        if (d_resampler)
            {
                d_status = d_resampler->open(static_cast<uint64_t>(consumed) * (d_max_dwells + 1), consumed);
                if (d_status != GC_OK) return;
                d_acq_ring = d_resampler->ring();
            }
        d_samples_per_code = static_cast<uint32_t>(std::floor(static_cast<double>(fs_in) / (code_rate / code_len)));
        if (fine_doppler)
            {
                gc_fine_doppler_conf f;
                std::memset(&f, 0, sizeof f);
                f.fs_in = fs_in;
                f.samples_per_code = d_samples_per_code;
                f.prn_replicas = 10;
                f.zero_padding_factor = 8;
                f.window_hz = 1000.0f;
                f.alignment = GC_FINE_ALIGN_EXACT;
                d_status = gc_fine_doppler_create(ctx, &f, static_cast<int>(prns.size()), &d_fine);
                if (d_status != GC_OK) return;
                d_fine_results.resize(prns.size());
            }
        // replicas: one code period at fs, tiled over the coherent time (the adapters' set_local_code)
        std::vector<float> one(2 * (d_samples_per_code + 16)), tiled(2 * static_cast<size_t>(consumed));
        std::vector<float> pilot, rep_a, rep_b;
        if (cccwsr) pilot.resize(tiled.size()), rep_a.resize(tiled.size()), rep_b.resize(tiled.size());
        for (size_t s = 0; s < prns.size() && d_status == GC_OK; s++)
            {
                const int32_t fs = static_cast<int32_t>(fs_in);
                if (system == 'G' && signal == "1C") d_status = gc_gps_l1_ca_code_gen_complex_sampled(one.data(), prns[s], fs, 0, nullptr);
                else if (system == 'G') d_status = gc_gps_l5i_code_gen_complex_sampled(one.data(), prns[s], fs, nullptr);
                else if (system == 'E' && signal == "1B") d_status = gc_galileo_e1_code_gen_complex_sampled(one.data(), "1B", 0, prns[s], fs, 0, nullptr);
                else if (system == 'E') d_status = gc_galileo_e5_a_code_gen_complex_sampled(one.data(), "5X", prns[s], fs, 0, nullptr);
                else if (signal == "B1") d_status = gc_beidou_b1i_code_gen_complex_sampled(one.data(), prns[s], fs, 0, nullptr);
                else d_status = gc_beidou_b3i_code_gen_complex_sampled(one.data(), prns[s], fs, 0, nullptr);
                if (d_status != GC_OK) return;
                for (size_t i = 0; i < consumed; i++)
                    {
                        tiled[2 * i] = one[2 * (i % d_samples_per_code)];
                        tiled[2 * i + 1] = one[2 * (i % d_samples_per_code) + 1];
                    }
                if (d_fine) d_status = gc_fine_doppler_set_code(d_fine, static_cast<int>(s), one.data());
                if (d_status != GC_OK) return;
                if (!cccwsr)
                    {
                        d_status = gc_acq_set_local_code(d_acq, static_cast<int>(s), tiled.data());
                        continue;
                    }
                d_status = gc_galileo_e1_code_gen_complex_sampled(one.data(), "1C", 0, prns[s], fs, 0, nullptr);
                if (d_status != GC_OK) return;
                for (size_t i = 0; i < consumed; i++)
                    {
                        pilot[2 * i] = one[2 * (i % d_samples_per_code)];
                        pilot[2 * i + 1] = one[2 * (i % d_samples_per_code) + 1];
                    }
                d_status = gc_cccwsr_replicas(tiled.data(), pilot.data(), consumed, rep_a.data(), rep_b.data());
                if (d_status == GC_OK) d_status = gc_acq_set_local_code_pair(d_acq, static_cast<int>(s), rep_a.data(), rep_b.data());
            }
        d_results.resize(prns.size());
        d_ready = (d_status == GC_OK);
    }
    ~hip_acquisition_bank()
    {
        if (d_acq) gc_acq_destroy(d_acq);
        if (d_fine) gc_fine_doppler_destroy(d_fine);
    }
    hip_acquisition_bank(const hip_acquisition_bank&) = delete;
    hip_acquisition_bank& operator=(const hip_acquisition_bank&) = delete;

    //! samples of the ring one dwell consumes (pcps_acquisition: d_consumed_samples, times the resampler's decimation)
    uint32_t consumed_samples() const { return d_consumed * d_ratio; }

    /*! With use_acquisition_resampler: lets the derived ring catch up with the ring (asynchronous; GC_OK and nothing to do
     *  without the resampler).  search() does this itself, but the decimator needs the ring samples from its last output on: call
     *  update() after every push -- or at least once per ring capacity of pushed samples -- when searches are sporadic.  Once the
     *  ring has run more than its capacity ahead of the derived ring, update() and every later search() return GC_ERR_STATE: the
     *  derived ring cannot skip samples (derived sample m is ring sample m * ratio), and the bank has to be built anew. */
    gc_status update()
    {
        if (d_resampler) d_status = d_resampler->update();
        return d_resampler ? d_status : GC_OK;
    }

    /*! One search of every satellite on ring samples [first_index, first_index + max_dwells * consumed_samples()): max_dwells
     *  non-coherent dwells, then the detections (statistic > threshold), strongest first.  Acq_samplestamp_samples is the stream
     *  index of the LAST dwell's first sample, as the block stamps it (pcps_acquisition.cc:768).  With the resampler the search
     *  starts at the next multiple of the decimation at or above first_index, so up to ratio - 1 further ring samples must have been
     *  pushed, and Acq_samplestamp_samples counts from that multiple. */
    std::vector<Gnss_Synchro> search(uint64_t first_index)
    {
        std::vector<Gnss_Synchro> found;
        // construction failed; a failed search is NOT sticky -- except a resampler that fell behind the ring, see update()
        if (d_acq == nullptr || !d_ready) return found;
        if (d_resampler)
            {
                // the derived ring catches up with the source; derived sample m is source sample m * ratio
                d_status = d_resampler->update();
                if (d_status != GC_OK) return found;
                first_index = (first_index + d_ratio - 1) / d_ratio;
            }
        d_status = gc_acq_reset(d_acq);
        uint64_t stamp = first_index;
        for (uint32_t dwell = 0; dwell < d_max_dwells && d_status == GC_OK; dwell++)
            {
                stamp = first_index + static_cast<uint64_t>(dwell) * d_consumed;
                d_status = gc_acq_dwell_stream(d_acq, d_acq_ring, stamp, d_results.data());
            }
        if (d_status != GC_OK) return found;
        std::vector<size_t> order;
        for (size_t s = 0; s < d_prns.size(); s++)
            if (d_results[s].test_statistics > d_threshold) order.push_back(s);
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return d_results[a].test_statistics > d_results[b].test_statistics; });
        if (d_fine) refine(first_index, order);
        for (size_t s : order)
            {
                Gnss_Synchro g;
                g.System = d_system;
                g.Signal[0] = d_signal[0];
                g.Signal[1] = d_signal[1];
                g.PRN = d_prns[s];
                if (d_resampler)
                    {
                        // take into account the acquisition resampler ratio and the filter's latency (pcps_acquisition.cc:756-762);
                        // the delay may come out negative, as in the reference
                        g.Acq_delay_samples = static_cast<double>(d_results[s].acq_delay_samples) * static_cast<double>(d_ratio);
                        g.Acq_delay_samples -= static_cast<double>(d_latency);
                        g.Acq_doppler_hz = d_results[s].acq_doppler_hz;
                        g.Acq_samplestamp_samples = static_cast<uint64_t>(std::rint(static_cast<double>(stamp) * static_cast<double>(d_ratio)));
                    }
                else
                    {
                        g.Acq_delay_samples = d_results[s].acq_delay_samples;
                        g.Acq_doppler_hz = d_results[s].acq_doppler_hz;
                        g.Acq_samplestamp_samples = stamp;
                    }
                g.Flag_valid_acquisition = true;
                found.push_back(g);
            }
        return found;
    }

    //! fine_doppler: the stage's record of satellite `sat` in the last search (status 0: not detected, or the stage did not run)
    const gc_fine_doppler_result& fine_result(size_t sat) const
    {
        static const gc_fine_doppler_result none{};
        return sat < d_fine_results.size() ? d_fine_results[sat] : none;
    }
    //! the statistic of every searched satellite in the last search (same order as `prns`)
    float statistic(size_t sat) const { return d_results[sat].test_statistics; }
    gc_status last_status() const { return d_status; }
    //! acquisition resampler: decimation in use (1: none), its latency in ring samples, and the rate the search runs at
    uint32_t resampler_ratio() const { return d_ratio; }
    uint32_t resampler_latency_samples() const { return d_latency; }

private:
    // the detections `order` of the search that began at first_index of the searched ring, in one call; acq_doppler_hz of d_results
    // is replaced where the stage refined
    void refine(uint64_t first_index, const std::vector<size_t>& order)
    {
        for (auto& r : d_fine_results) std::memset(&r, 0, sizeof r);
        if (order.empty()) return;
        std::vector<gc_fine_doppler_request> req(order.size());
        std::vector<gc_fine_doppler_result> res(order.size());
        for (size_t i = 0; i < order.size(); i++)
            {
                const gc_acq_result& r = d_results[order[i]];
                req[i].slot = static_cast<uint32_t>(order[i]);
                req[i].delay_samples = static_cast<uint32_t>(r.acq_delay_samples) % d_samples_per_code;
                req[i].coarse_doppler_hz = r.acq_doppler_hz;
            }
        d_status = gc_fine_doppler_estimate_stream(d_fine, d_acq_ring, first_index, req.data(), static_cast<int>(req.size()), res.data());
        if (d_status != GC_OK) return;
        for (size_t i = 0; i < order.size(); i++)
            {
                d_fine_results[order[i]] = res[i];
                if (res[i].status == GC_FINE_REFINED) d_results[order[i]].acq_doppler_hz = res[i].doppler_hz;
            }
    }

    gc_stream* d_ring;
    gc_stream* d_acq_ring;            // the ring the dwells read: d_ring, or the resampler's derived ring
    std::unique_ptr<hip_ring_decimator> d_resampler;
    uint32_t d_ratio = 1, d_latency = 0;
    gc_acq* d_acq = nullptr;
    gc_fine_doppler* d_fine = nullptr;
    std::vector<gc_fine_doppler_result> d_fine_results;
    bool d_ready = false;  // construction went through (every replica installed)
    char d_system;
    std::string d_signal;
    std::vector<uint32_t> d_prns;
    float d_threshold;
    uint32_t d_max_dwells;
    uint32_t d_consumed = 0, d_samples_per_code = 0;
    gc_status d_status = GC_OK;
    std::vector<gc_acq_result> d_results;
};

#endif  // GNSSCORR_HIP_ACQUISITION_BANK_H_
