// trk_window_plan.h -- what the multicorrelator (trk_device.hpp: trk_epoch, trk_loop) decides from integers and the code NCO's
// scalars alone, for one (window, slice): how the window is cut in chunks and which of them may be fetched whole, which samples
// the slice touches, which chips those samples read and where the kernel finds them.  Pure functions, host and device, compiled
// without HIP by tests/trk_window_plan_selftest.cpp (tests/test_trk_window_plan.py).
// The kernels call posmod, chip_index, chip_index_hd, TRK_RESIDENT_PAD and trk_whole_first / trk_whole_end (lc0, lc1: what keeps the
// whole-chunk fetch of a ragged chunk inside the buffer) from here.  The rest of the chunk plan, the sample range, the code span and
// the table path are stated here in trk_epoch's own formulas and operation order, and trk_epoch still computes them itself:
// calling all of them from it left the batched kernels' code as it was but moved the register allocation of 22 closed-loop kernels
// and cost the closed loop 1 %, so for those the tie is the test, which holds this header, trk_epoch's statement
// in Python (tests/open_loop_matrix_cases.py::epoch_path) and the device results together.
// The float expressions keep the reference's operation order (one rounding per operation): build with -ffp-contract=off.
#ifndef TRK_WINDOW_PLAN_H
#define TRK_WINDOW_PLAN_H
#include <cmath>

#ifdef __HIP__
#define TRK_WINDOW_PLAN_HD_MEMBER __host__ __device__ __forceinline__
#define TRK_WINDOW_PLAN_UNROLL _Pragma("unroll")
#else
#define TRK_WINDOW_PLAN_HD_MEMBER inline
#define TRK_WINDOW_PLAN_UNROLL
#endif
#define TRK_WINDOW_PLAN_HD static TRK_WINDOW_PLAN_HD_MEMBER

#define TRK_RESIDENT_PAD 64  // chips behind the doubled code image of a resident table (trk_device.hpp)

TRK_WINDOW_PLAN_HD int trk_imin(int x, int y) { return x < y ? x : y; }
TRK_WINDOW_PLAN_HD int trk_imax(int x, int y) { return x > y ? x : y; }
TRK_WINDOW_PLAN_HD unsigned long long trk_umin(unsigned long long x, unsigned long long y) { return x < y ? x : y; }

TRK_WINDOW_PLAN_HD int posmod(int i, int L)
{
    int r = i % L;
    return r < 0 ? r + L : r;
}

// chip index before wrapping, generic resampler order: ((step*n) + shift) - rem
TRK_WINDOW_PLAN_HD int chip_index(float step, float nf, float shift, float rem)
{
    float a = step * nf;
    float b = a + shift;
    float c = b - rem;
    return (int)floorf(c);
}

// high-dynamics first tap: (((step*n) + rate*(float)(n*n)) + shift0) - rem, n*n in uint32
TRK_WINDOW_PLAN_HD int chip_index_hd(float step, float rate, unsigned n, float shift0, float rem)
{
    float a = step * (float)n;
    float r = rate * (float)(n * n);
    float b = a + r;
    float c = b + shift0;
    float d = c - rem;
    return (int)floorf(d);
}

// ---- chunk geometry ----
// where the window starts in the channel's buffer, and where that buffer ends (a ring's mirror is not counted)
TRK_WINDOW_PLAN_HD unsigned long long trk_window_off(unsigned long long sample_offset, unsigned ring_len)
{
    return ring_len ? sample_offset % ring_len : sample_offset;  // (one 64-bit division per epoch)
}
TRK_WINDOW_PLAN_HD unsigned long long trk_window_end(unsigned long long n_iq, unsigned ring_len) { return ring_len ? (unsigned long long)ring_len : n_iq; }
// samples between the aligned address the chunks are counted from and the window's first one, whose address is `first_elem` elements:
// the grid has 2 * align_pairs elements
TRK_WINDOW_PLAN_HD int trk_window_lead(unsigned long long first_elem, int align_pairs) { return (int)(first_elem & (unsigned long long)(2 * align_pairs - 1)); }

// Chunks [trk_whole_first, trk_whole_end) of a window lie inside the channel's buffer as WHOLE chunks: the only thing between the
// whole-chunk fetch of a ragged chunk and a read outside the buffer.  off, end: trk_window_off / trk_window_end; a: trk_window_lead;
// n_chunks: of the window.  trk_epoch calls these two.
TRK_WINDOW_PLAN_HD int trk_whole_first(unsigned long long off, int a) { return off >= (unsigned long long)a ? 0 : 1; }
template <int CHUNK>
TRK_WINDOW_PLAN_HD int trk_whole_end(unsigned long long off, unsigned long long end, int a, int n_chunks)
{
    const unsigned long long room = end > off ? end - off : 0;
    return (int)trk_umin((unsigned long long)n_chunks, (room + (unsigned long long)a) / CHUNK);
}

// The chunks of one (window, slice).  The window's N samples start `a` elements behind an aligned address; chunks of CHUNK elements
// are counted from that address: sample n is element v = n + a, in chunk v / CHUNK.  Slice `slice` of n_slices takes chunks [c0, c1).
template <int CHUNK>
struct TrkChunkPlan
{
    int a, N;
    int V;         // N + a: elements from the aligned address to the window's end
    int n_chunks;  // of the window
    int cps;       // chunks per slice
    int c0, c1;    // this slice's
    // Chunks [lc0, lc1) lie inside the channel's buffer as WHOLE chunks (the ragged first / last chunk of a window usually does: its
    // neighbours in the stream are there), so they may be fetched like the others -- 16-byte loads, prefetched -- and the samples
    // outside the window zeroed in registers
    int lc0, lc1;

    // A chunk is "full" when every lane's two samples lie inside the window: plain 16-byte loads, no masks, no clamps.  Only the
    // first chunk (odd-aligned window) and the last one can be ragged.
    TRK_WINDOW_PLAN_HD_MEMBER bool chunk_is_full(int c) const { return (c > 0 || a == 0) && (c + 1) * CHUNK <= V; }
    // a chunk that may be fetched whole: every full chunk (it lies inside the window, mirror of a ring included), and with `whole`
    // the ragged ones found inside the buffer
    TRK_WINDOW_PLAN_HD_MEMBER bool loadable(int c, bool whole) const { return chunk_is_full(c) || (whole && c >= lc0 && c < lc1); }
};

// off, end: trk_window_off / trk_window_end
template <int CHUNK>
TRK_WINDOW_PLAN_HD TrkChunkPlan<CHUNK> trk_chunk_plan(unsigned long long off, unsigned long long end, int a, int N, int slice, int n_slices)
{
    TrkChunkPlan<CHUNK> w;
    w.a = a;
    w.N = N;
    w.V = N + a;
    w.n_chunks = (w.V + CHUNK - 1) / CHUNK;
    w.cps = (w.n_chunks + n_slices - 1) / n_slices;
    w.c0 = slice * w.cps;
    w.c1 = trk_imin(w.n_chunks, w.c0 + w.cps);
    w.lc0 = trk_whole_first(off, a);
    w.lc1 = trk_whole_end<CHUNK>(off, end, a, w.n_chunks);
    return w;
}

// ---- sample range ----
// Sample numbers the slice touches (clamped lanes included): [n_lo, n_hi].  hdr: the high-dynamics resampler's taps are tap 0
// delayed and wrapped at N, so every slice may read any sample's chip.
struct TrkSampleRange
{
    int n_lo, n_hi;
};
template <int CHUNK>
TRK_WINDOW_PLAN_HD TrkSampleRange trk_sample_range(const TrkChunkPlan<CHUNK>& w, bool hdr)
{
    TrkSampleRange r;
    if (hdr)
        {
            r.n_lo = 0;
            r.n_hi = trk_imax(w.N - 1, 0);
        }
    else
        {
            r.n_lo = trk_imax(w.c0 * CHUNK - w.a, 0);
            r.n_hi = trk_imax(trk_imin(w.c1 * CHUNK - w.a, w.N) - 1, r.n_lo);
        }
    return r;
}

// ---- code span ----
// Chips [lo, hi] the samples [n_lo, n_hi] read over all taps, and whether the chip index is monotone in the sample number (then
// no sample between them reads a chip outside).  data: the data component's prompt-only correlator rides along (pilot tracking)
struct TrkCodeSpan
{
    int lo, hi;
    bool monotone;
};
template <int NTAPS>
TRK_WINDOW_PLAN_HD TrkCodeSpan trk_code_span(bool hdr, bool data, float step, float rem, float rate, const float (&shifts)[NTAPS], TrkSampleRange r)
{
    TrkCodeSpan s;
    float smin = shifts[0], smax = shifts[0];
    if (!hdr)
        {
            TRK_WINDOW_PLAN_UNROLL
            for (int t = 1; t < NTAPS; t++)
                {
                    smin = fminf(smin, shifts[t]);
                    smax = fmaxf(smax, shifts[t]);
                }
        }
    if (hdr)
        {
            s.lo = chip_index_hd(step, rate, (unsigned)r.n_lo, shifts[0], rem);
            s.hi = chip_index_hd(step, rate, (unsigned)r.n_hi, shifts[0], rem);
            if (data)
                {
                    // the data tap walks the same samples with the prompt shift instead of the first tap's
                    s.lo = trk_imin(s.lo, chip_index_hd(step, rate, (unsigned)r.n_lo, shifts[NTAPS / 2], rem));
                    s.hi = trk_imax(s.hi, chip_index_hd(step, rate, (unsigned)r.n_hi, shifts[NTAPS / 2], rem));
                }
            // float ops are monotone, so the index is monotone in n when both terms are
            s.monotone = (step > 0.0f) && (rate >= 0.0f) && ((unsigned long long)r.n_hi * r.n_hi < 0xffffffffull);
        }
    else
        {
            s.lo = chip_index(step, (float)r.n_lo, smin, rem);
            s.hi = chip_index(step, (float)r.n_hi, smax, rem);
            s.monotone = (step >= 0.0f);
        }
    return s;
}

// ---- table path ----
// Where the loop finds the chips of [lo, hi].  The LDS behind the header holds lds_table_floats floats; a chip takes `words` of
// them (2: complex chips), twice that with the data component's replica.
enum TrkTablePath
{
    TRK_TABLE_WINDOW,        // code[(lo + k) mod L], k < span, filled into LDS with two conditional subtractions; lookups need no wrap
    TRK_TABLE_WINDOW_MOD,    // the same window filled with `% L` (it wraps the code more than twice)
    TRK_TABLE_RESIDENT,      // the caller keeps the doubled image R[i] = code[i mod L] in LDS: the window is addressed inside it
    TRK_TABLE_RESIDENT_MOD,  // ... a span too long for the image: its first L entries, lookups wrapped with the reference's modulo
    TRK_TABLE_LDS,           // the whole table filled into LDS, lookups wrapped
    TRK_TABLE_GLOBAL         // neither fits the launch's LDS: lookups in global memory, wrapped (gtab launches only)
};
struct TrkTablePlan
{
    TrkTablePath path;
    int lo;    // chip number of the table's entry 0 (windows; 0 for the wrapped forms)
    int span;  // chips of the window (windows)
};
TRK_WINDOW_PLAN_HD bool trk_table_windowed(TrkTablePath p) { return p == TRK_TABLE_WINDOW || p == TRK_TABLE_WINDOW_MOD || p == TRK_TABLE_RESIDENT; }

// The predicates the path is made of, in the order trk_epoch evaluates them; trk_table_plan() names the outcome.
TRK_WINDOW_PLAN_HD long long trk_span(int lo, int hi) { return (long long)hi - (long long)lo + 1; }
// the window [lo, hi] fits the launch's LDS
TRK_WINDOW_PLAN_HD bool trk_window_fits(bool monotone, long long span_ll, int words, bool data, int lds_table_floats)
{
    return monotone && span_ll > 0 && span_ll * (long long)words * (data ? 2 : 1) <= (long long)lds_table_floats;
}
// the whole table fits the launch's LDS.  gtab: the launch may have been given less (else the caller guarantees that it fits)
TRK_WINDOW_PLAN_HD bool trk_table_fits(bool gtab, int L, int words, bool data, int lds_table_floats)
{
    return !gtab || (long long)L * (long long)words * (data ? 2 : 1) <= (long long)lds_table_floats;
}
// the doubled resident image is in place: the window can be addressed inside it (chip - lo + cbase < 2 L + pad)
TRK_WINDOW_PLAN_HD bool trk_resident_window_fits(bool monotone, long long span_ll, int L) { return monotone && span_ll > 0 && span_ll <= (long long)L + TRK_RESIDENT_PAD; }
// a window that starts at chip cbase of the code ends below 3 L: two conditional subtractions wrap it, instead of a division
TRK_WINDOW_PLAN_HD bool trk_window_wraps_twice_at_most(int cbase, int span, int L) { return cbase + span <= 3 * L; }

TRK_WINDOW_PLAN_HD TrkTablePlan trk_table_plan(int lo, int hi, bool monotone, int words, bool data, int L, int lds_table_floats, bool resident, bool gtab)
{
    const long long span_ll = trk_span(lo, hi);
    TrkTablePlan t = {TRK_TABLE_LDS, 0, 0};
    if (resident)
        {
            if (trk_resident_window_fits(monotone, span_ll, L))
                {
                    t.path = TRK_TABLE_RESIDENT;
                    t.lo = lo - posmod(lo, L);
                    t.span = (int)span_ll;
                }
            else
                t.path = TRK_TABLE_RESIDENT_MOD;  // the image's first L entries with the modulo form
        }
    else if (trk_window_fits(monotone, span_ll, words, data, lds_table_floats))
        {
            t.span = (int)span_ll;
            t.lo = lo;
            t.path = trk_window_wraps_twice_at_most(posmod(lo, L), t.span, L) ? TRK_TABLE_WINDOW : TRK_TABLE_WINDOW_MOD;
        }
    else if (!trk_table_fits(gtab, L, words, data, lds_table_floats))
        t.path = TRK_TABLE_GLOBAL;
    return t;
}

#endif
