// acq_engine_sizes_selftest.cpp -- the size rules of the acquisition engines (gnss-sdr-1_amd/csrc/acq_engine_sizes.h) on the host.
// Prints one line per case: `name fft_size consumed eff input_len n_bins n_bins_alloc max_dwells use_cfar replicas sats_per_batch
// q_cells`, or `name empty` for an empty grid; then `pair name sats_per_batch` for the batch rule of the inverse passes.  CPU only;
// tests/test_acq_engine_sizes.py holds the expected lines, derived by hand from the reference formulas the header cites.
#include "acq_engine_sizes.h"
#include <cstdio>

static gc_acq_conf base()
{
    gc_acq_conf c{};
    c.fs_in = 4000000;
    c.sampled_ms = 1;
    c.ms_per_code = 1;
    c.samples_per_ms = 4000.0f;
    c.samples_per_code = 4000.0f;
    c.samples_per_chip = 4;
    c.doppler_max = 5000;
    c.doppler_step = 250;
    c.max_dwells = 1;
    c.use_CFAR_algorithm_flag = 1;
    c.doppler_step2 = 125.0f;
    return c;
}

static AcqEngineSpec spec_of(AcqKind kind)
{
    AcqEngineSpec s;
    s.kind = kind;
    return s;
}

static const size_t BIG = (size_t)140 << 20;

static AcqEngineSizes show(const char* name, const gc_acq_conf& c, const AcqEngineSpec& s, int n_sats = 1, size_t budget = BIG)
{
    const AcqEngineSizes z = acq_engine_sizes(c, s, n_sats, budget);
    if (z.empty_grid)
        std::printf("%s empty\n", name);
    else
        std::printf("%s %u %u %u %u %u %u %u %d %d %d %zu\n", name, z.fft_size, z.consumed, z.eff, z.input_len, z.n_bins, z.n_bins_alloc, z.max_dwells,
            z.use_cfar ? 1 : 0, z.replicas, z.sats_per_batch, z.q_cells);
    return z;
}

int main()
{
    gc_acq_conf c = base();
    show("plain", c, spec_of(ACQ_PLAIN));
    c.num_doppler_bins_override = 41;
    show("override", c, spec_of(ACQ_PLAIN));

    c = base();
    c.sampled_ms = 2;  // two code periods of 1 ms
    show("zero_padded", c, spec_of(ACQ_PLAIN));

    c = base();
    c.bit_transition_flag = 1;
    c.max_dwells = 3;
    show("bit_transition", c, spec_of(ACQ_PLAIN));

    c = base();
    c.max_dwells = 2;
    show("two_dwells_cfar", c, spec_of(ACQ_PLAIN));

    c = base();
    c.make_2_steps = 1;
    c.num_doppler_bins_step2 = 50;
    show("step_two_larger", c, spec_of(ACQ_PLAIN));
    c.num_doppler_bins_step2 = 4;
    show("step_two_smaller", c, spec_of(ACQ_PLAIN));

    c = base();
    AcqEngineSpec s = spec_of(ACQ_PAIRED);
    s.combine = GC_ACQ_COMBINE_MAX;
    show("paired", c, s);

    c = base();
    c.sampled_ms = 4;
    s = spec_of(ACQ_QUICKSYNC);
    s.fold = 4;
    show("quicksync", c, s);

    c = base();
    c.sampled_ms = 2;
    c.ms_per_code = 4;  // as gc_acq_create_tong leaves it is sampled_ms; the rule holds whatever it says
    show("tong", c, spec_of(ACQ_TONG));

    c = base();
    for (int hyp = 1; hyp <= 2; hyp++)
        for (int both = 0; both <= 1; both++)
            {
                s = spec_of(ACQ_CAF);
                s.caf.both = both;
                s.caf.hyp = hyp;
                char name[32];
                std::snprintf(name, sizeof name, "caf_both%d_hyp%d", both, hyp);
                show(name, c, s);
            }

    // batching: a satellite's row-pass output is 40 bins x 4000 samples x 8 bytes = 1 280 000 bytes
    c = base();
    const size_t per_sat = 1280000;
    show("batch_all", c, spec_of(ACQ_PLAIN), 5, 5 * per_sat);
    show("batch_less_than_one", c, spec_of(ACQ_PLAIN), 5, per_sat - 1);
    show("batch_three_fit", c, spec_of(ACQ_PLAIN), 5, 3 * per_sat + 7);
    const AcqEngineSizes z = show("batch_two_fit", c, spec_of(ACQ_PLAIN), 5, 2 * per_sat + 7);
    // the inverse passes on those 80 rows: a dwell's 40 spectra per satellite, a dwell pair's 80, and a step-two grid of 4 bins
    std::printf("pair single %d\n", acq_inverse_sats_per_batch(z.q_cells, 40, 5));
    std::printf("pair pair %d\n", acq_inverse_sats_per_batch(z.q_cells, 80, 5));
    std::printf("pair step_two %d\n", acq_inverse_sats_per_batch(z.q_cells, 4, 5));

    c = base();
    c.doppler_max = 0;
    show("empty_plain", c, spec_of(ACQ_PLAIN));
    show("one_bin_tong", c, spec_of(ACQ_TONG));
    return 0;
}
