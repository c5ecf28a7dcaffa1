/*
 * gnsscorr.h -- C ABI of libgnsscorr.so, the MI355X (gfx950, HIP) acquisition +
 * tracking correlator engine.
 *
 * This is the drop-in boundary for ONE path of GNSS-SDR (zhufengGNSS/gnss-sdr-1):
 *
 *   tracking   Cpu_Multicorrelator_Real_Codes                      (reference:
 *              src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.h:45-69)
 *              = volk_gnsssdr_32f_xn_resampler_32f_xn               (code NCO)
 *              + volk_gnsssdr_32fc_32f_rotator_dot_prod_32fc_xn     (carrier NCO + E/P/L)
 *   acquisition pcps_acquisition                                    (reference:
 *              src/algorithms/acquisition/gnuradio_blocks/pcps_acquisition.h:81-261,
 *              .cc:239-274 set_local_code, :313-368 init, :668-927 acquisition_core)
 *
 * Conventions: plain C types only (no C++/torch types); every function returns
 * a gc_status (0 = ok) and records a message readable with gc_last_error();
 * no exception crosses the ABI.  "host" pointers are caller-owned host memory,
 * "dev" pointers are caller-owned device (HBM) memory on the context's GPU.
 * Complex values are interleaved float32 (re, im), i.e. std::complex<float> /
 * gr_complex / lv_32fc_t.  A `stream` argument is a hipStream_t passed as
 * void* (NULL = the context's own stream).  The library fails loudly
 * (GC_ERR_NO_DEVICE) when no HIP device is usable: there is no CPU fallback.
 *
 * Threading follows the reference (one correlator / acquisition object per
 * channel, driven by that channel's thread): a handle is used by one thread at
 * a time; different handles of one context may be used from different threads
 * at once (their calls are serialised on the context's mutex and stream).
 *
 * The C++ classes in gnss-sdr-1_amd/adapter/ (Hip_Multicorrelator_Real_Codes,
 * hip_pcps_acquisition, the TrackingInterface/AcquisitionInterface-shaped
 * adapters) are thin inline wrappers over these entry points; INTEGRATION.md
 * shows the binding a GNSS-SDR maintainer adds.
 */
#ifndef GNSSCORR_H
#define GNSSCORR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int gc_status;
enum
{
    GC_OK = 0,
    GC_ERR_INVALID = 1,   /* bad argument / shape */
    GC_ERR_NO_DEVICE = 2, /* no usable HIP device (no CPU fallback exists) */
    GC_ERR_HIP = 3,       /* a HIP runtime call failed */
    GC_ERR_STATE = 4      /* call sequence error (e.g. correlate before init) */
};

/* Last error message of the calling thread ("" when none). */
const char* gc_last_error(void);
/* Library version string. */
const char* gc_version(void);
/* Layout check between a binding and the loaded library: the sizes of the structures that cross the ABI, as the CALLER's
 * header (or ctypes / cgo / JNI mirror) sees them.  GC_OK when they all match the library's.  C and C++ callers use
 * GC_ABI_CHECK() after including this header (the macro is at its end). */
gc_status gc_abi_check(size_t sizeof_epoch_params, size_t sizeof_loop_conf, size_t sizeof_loop_record, size_t sizeof_loop_sync_conf,
    size_t sizeof_acq_conf, size_t sizeof_acq_result);
/* Number of visible HIP devices (0 when none; never fails). */
int gc_device_count(void);
/* 1 when the library was built with -DGNSSCORR_EXPERIMENTS: it then also carries the measured-slower kernel variants and reads
 * their GNSSCORR_* tuning variables.  The product build returns 0 and reads none of them. */
int gc_build_has_experiments(void);

/* ------------------------------------------------------------------------ */
/* Context: one per GPU.  Owns a HIP stream and scratch buffers.             */
/* ------------------------------------------------------------------------ */
typedef struct gc_ctx gc_ctx;
gc_status gc_ctx_create(int device, gc_ctx** out);
/* Drops the caller's reference.  Handles created on the context keep it (and its
 * stream) alive until the last of them is destroyed, so the order of the destroy
 * calls does not matter; the same holds for a gc_stream and the batches reading it. */
gc_status gc_ctx_destroy(gc_ctx* ctx);
gc_status gc_ctx_synchronize(gc_ctx* ctx);

/* ------------------------------------------------------------------------ */
/* Level 1 -- one correlator object per channel, host pointers, synchronous. */
/* Method-for-method image of Cpu_Multicorrelator_Real_Codes                 */
/* (cpu_multicorrelator_real_codes.h:48-57).  Pointer arguments are RETAINED, */
/* not copied, exactly like the reference (cpu_multicorrelator_real_codes.cc: */
/* 79-98): `shifts_chips` and the code table are re-read on every correlate   */
/* call, so the caller may edit the shifts between calls.                     */
/* ------------------------------------------------------------------------ */
typedef struct gc_correlator gc_correlator;
gc_status gc_correlator_create(gc_ctx* ctx, gc_correlator** out);
gc_status gc_correlator_destroy(gc_correlator* c);
/* ::set_high_dynamics_resampler (.cc:189-193).  The reference constructor
 * defaults this flag to TRUE (.cc:49); so does gc_correlator_create. */
gc_status gc_correlator_set_high_dynamics_resampler(gc_correlator* c, int use_high_dynamics_resampler);
/* ::init (.cc:62-76) */
gc_status gc_correlator_init(gc_correlator* c, int max_signal_length_samples, int n_correlators);
/* ::set_local_code_and_taps (.cc:79-89) */
gc_status gc_correlator_set_local_code_and_taps(gc_correlator* c, int code_length_chips,
    const float* local_code_in, float* shifts_chips);
/* ::set_input_output_vectors (.cc:92-98); corr_out: n_correlators complex,
 * sig_in: >= signal_length_samples complex (host memory) */
gc_status gc_correlator_set_input_output_vectors(gc_correlator* c, float* corr_out, const float* sig_in);
/* ::Carrier_wipeoff_multicorrelator_resampler, 7-argument form (.cc:129-152) */
gc_status gc_correlator_carrier_wipeoff_multicorrelator_resampler(gc_correlator* c,
    float rem_carrier_phase_in_rad, float phase_step_rad, float phase_rate_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips,
    int signal_length_samples);
/* 6-argument form (.cc:155-170): always the plain rotator; the resampler still
 * follows the high-dynamics flag */
gc_status gc_correlator_carrier_wipeoff_multicorrelator_resampler_6(gc_correlator* c,
    float rem_carrier_phase_in_rad, float phase_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips,
    int signal_length_samples);
/* ::free (.cc:173-186) */
gc_status gc_correlator_free(gc_correlator* c);
/* Engine statistics (no reference counterpart).  Concurrent calls of Carrier_wipeoff_multicorrelator_resampler from the
 * channel threads of one context are combined into batches, one kernel launch each ("epoch batcher"): launches so far, calls
 * served, calls whose input window was shared with another call of the same batch (same sig_in pointer: one copy to the GPU
 * for the group), and the largest batch.  Any pointer may be NULL. */
gc_status gc_correlator_batch_stats(gc_ctx* ctx, uint64_t* n_batches, uint64_t* n_requests, uint64_t* n_shared_windows, int* max_batch);
/* Optional, no reference counterpart: page-locks caller memory that the correlators of this context read their input from --
 * typically the GNU Radio buffer behind the tracking blocks' input port (every channel's sig_in points into it,
 * gnss_flowgraph.cc:496-499).  Windows inside a registered buffer go to the GPU without the staging copy, and the windows of one
 * batch that overlap (channels at neighbouring read positions) cross PCIe once, as one transfer of their union.  The memory must
 * stay valid until it is unregistered or the context is destroyed.  Fails (and changes nothing) where the runtime cannot pin the
 * range, e.g. some doubly mapped circular buffers. */
gc_status gc_ctx_register_host_buffer(gc_ctx* ctx, const void* base, size_t bytes);
gc_status gc_ctx_unregister_host_buffer(gc_ctx* ctx, const void* base);

/* The same object with COMPLEX chips is the image of Cpu_Multicorrelator
 * (cpu_multicorrelator.h:46-64; GLONASS L1/L2 and the GPS L1 C-Aid trackers):
 * volk_gnsssdr_32fc_xn_resampler_32fc_xn (.cc:103-113) followed by
 * volk_gnsssdr_32fc_x2_rotator_dot_prod_32fc_xn (.cc:116-130).  It has no
 * carrier-rate / code-rate arguments and no high-dynamics variant.
 * local_code_in_iq: code_length_chips (re, im) pairs, pointer retained. */
gc_status gc_correlator_set_local_code_and_taps_complex(gc_correlator* c, int code_length_chips,
    const float* local_code_in_iq, float* shifts_chips);
/* Cpu_Multicorrelator::Carrier_wipeoff_multicorrelator_resampler, 5 arguments
 * (cpu_multicorrelator.cc:116-130); GC_ERR_STATE unless the code is complex
 * (float pairs, or lv_16sc_t with the setters below). */
gc_status gc_correlator_carrier_wipeoff_multicorrelator_resampler_5(gc_correlator* c,
    float rem_carrier_phase_in_rad, float phase_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips,
    int signal_length_samples);

/* With lv_16sc_t chips, input and output the object is the image of
 * Cpu_Multicorrelator_16sc (cpu_multicorrelator_16sc.h:44-67; the *_sc C-Aid
 * trackers): volk_gnsssdr_16ic_xn_resampler_16ic_xn followed by
 * volk_gnsssdr_16ic_x2_rotator_dot_prod_16ic_xn (.cc:78-103), run with the
 * 5-argument call above.  Arithmetic: each rotated sample is rounded to int16
 * (rintf), multiplied with the int16 chip (int16 wrap) and summed.  The sums
 * are formed exactly in 32 bits and saturated once, which equals the
 * reference's running saturating sum whenever no intermediate sum leaves the
 * int16 range; the rounding of a sample can differ by one LSB where the
 * reference's sequentially rounded float phase puts it on the other side of
 * x.5.  int16 arrays are (re, im) interleaved. */
gc_status gc_correlator_set_local_code_and_taps_16sc(gc_correlator* c, int code_length_chips,
    const int16_t* local_code_in_iq, float* shifts_chips);
gc_status gc_correlator_set_input_output_vectors_16sc(gc_correlator* c, int16_t* corr_out, const int16_t* sig_in);

/* ------------------------------------------------------------------------ */
/* RF stream ring: the IQ samples of one RF stream, pushed to a GPU once and    */
/* read by every channel / acquisition of that stream (all channels of a        */
/* GNSS-SDR flowgraph read the same stream, gnss_flowgraph.cc:496-499).  A ring  */
/* of capacity_samples in HBM plus a mirror of its first max_window_samples, so  */
/* that any window of <= max_window_samples is contiguous; consumers address it  */
/* with ABSOLUTE sample numbers (0 = first sample ever pushed).  Pushes are      */
/* asynchronous (own HIP stream, pinned staging) and overlap with compute; a     */
/* push waits only for launches that may still read the samples it evicts.       */
/* ------------------------------------------------------------------------ */
typedef struct gc_stream gc_stream;
gc_status gc_stream_create(gc_ctx* ctx, int iq_format, uint64_t capacity_samples, uint32_t max_window_samples,
    gc_stream** out);
gc_status gc_stream_destroy(gc_stream* s);
/* Appends n_samples (host memory, gc_iq_format of the stream; at most capacity_samples per call).
 * first_index (optional) receives the absolute number of the first appended sample. */
gc_status gc_stream_push(gc_stream* s, const void* host_iq, uint64_t n_samples, uint64_t* first_index);
/* Same for a PAGE-LOCKED host buffer (hipHostMalloc / hipHostRegister, e.g. a pinned torch tensor): the DMA
 * reads it directly, without the staging copy, so it must stay untouched until gc_stream_synchronize(). */
gc_status gc_stream_push_pinned(gc_stream* s, const void* pinned_host_iq, uint64_t n_samples, uint64_t* first_index);
/* The same page-locked block into several rings -- the RF stream's copy on each GPU of a node (channels are
 * sharded over the GPUs, every GPU needs the whole stream, no collective): G independent H2D copies enqueued back to back, each
 * on its ring's own copy stream.  The rings share the sample format; the block stays untouched until every ring is synchronised. */
gc_status gc_stream_broadcast_pinned(gc_stream* const* rings, int n_rings, const void* pinned_host_iq, uint64_t n_samples);
/* Resident range [oldest_index, head_index) and the ring capacity (any pointer may be NULL). */
gc_status gc_stream_info(gc_stream* s, uint64_t* oldest_index, uint64_t* head_index, uint64_t* capacity_samples);
/* Waits until every push so far has landed in HBM. */
gc_status gc_stream_synchronize(gc_stream* s);
/* Copies the resident window [first_index, first_index + n_samples) to host memory in the ring's format (tests, failure dumps).
 * Synchronous: waits for the pushes so far.  GC_ERR_STATE when the window is not resident. */
gc_status gc_stream_read(gc_stream* s, uint64_t first_index, uint64_t n_samples, void* host_out);
/* DIAGNOSTICS (tests, failure dumps; nothing a receiver needs).  A ring's storage is capacity_samples, then the mirror of
 * max_window_samples, then 2 samples of slack that nothing writes; in front of it and behind it lies a guard band filled with a
 * fixed byte at creation.
 * gc_stream_debug_read_storage copies the RAW storage positions [first_position, first_position + n_samples), anywhere in
 * [0, capacity_samples + max_window_samples + 2), to host memory in the ring's format, without any residency check: what a kernel
 * that reads a window through the mirror sees.  Synchronous: waits for what has been enqueued on the ring.  GC_ERR_INVALID when
 * the range leaves the storage.
 * gc_stream_debug_guards copies both guard bands to the host and reports, as 1 or 0, whether every byte of the band in front of
 * the ring and of the band behind it still holds the fill: a 0 means that something stored outside the ring's storage.
 * gc_stream_debug_set_origin makes an empty ring start at sample number `origin` instead of 0, as if `origin` samples had been
 * pushed and evicted: gc_stream_info reports oldest_index == head_index == origin, the first push returns first_index == origin
 * and lands at storage position origin % capacity_samples (mirror included), everything below `origin` is not resident to any
 * reader, and the storage stays zero-filled.  It lets a test run the readers of a ring at the sample numbers of a stream that has
 * been running for hours (past 2^31, 2^32, 2^53) without pushing that many samples; a receiver never calls it.  Allowed once, on a
 * ring that holds nothing and has no producer on the device (GC_ERR_STATE otherwise, nothing changes); an origin above 2^62 is
 * GC_ERR_INVALID -- a condition of this hook, which keeps head arithmetic and index * decimation products of a test from
 * wrapping, not a limit of the ring.  Origin 0, the default, is a ring as it always was.
 * A ring with an origin other than 0 can be the SOURCE of a gc_ring_decimator and of a gc_ring_resampler, while nothing has been
 * evicted from it since the origin: the stage's first output is the first one whose whole input window lies at or above the
 * origin, and the output ring receives that output's number as its own origin (so nothing in front of the origin is ever read).
 * gc_ring_notch_create refuses such a source with GC_ERR_STATE; a gc_conditioner and a gc_signal_generator number their own
 * input and take an output ring with origin 0 only, and so does every derived stage: an OUTPUT ring gets its origin from the
 * stage, never from this call. */
gc_status gc_stream_debug_read_storage(gc_stream* s, uint64_t first_position, uint64_t n_samples, void* host_out);
gc_status gc_stream_debug_guards(gc_stream* s, int32_t* front_intact, int32_t* back_intact);
gc_status gc_stream_debug_set_origin(gc_stream* s, uint64_t origin);

/* ------------------------------------------------------------------------ */
/* Signal conditioner: a frequency-translating FIR decimator in front of a      */
/* ring.  The reference puts a signal conditioner (data-type adapter, input      */
/* filter, resampler) between every source and its channels                      */
/* (gnss_flowgraph.cc:496-499 connects the channels to its output); this is the   */
/* input filter Freq_Xlating_Fir_Filter                                          */
/* (src/algorithms/input_filter/adapters/freq_xlating_fir_filter.cc: keys IF,      */
/* sampling_frequency, decimation_factor, taps) with the data-type adapter folded  */
/* in.  Raw samples x[n] (n = absolute number, x[n] = 0 for n < 0) are pushed to   */
/* the conditioner; a kernel writes                                              */
/*                                                                            */
/*   y[m] = sum_{k=0}^{T-1} h[k] * x[mD - k] * exp(-j 2 pi phi(mD - k))          */
/*   phi(n) = ((n * inc) mod 2^64) >> 32, a fraction of a turn in units of 2^-32  */
/*   inc    = round(translate_hz / fs_in * 2^64) mod 2^64   (IEEE double, ties to even) */
/*                                                                            */
/* into the output ring (GC_IQ_F32; or quantised into a GC_IQ_I16 / GC_IQ_I8    */
/* ring, "Integer output rings" below), which acquisition, tracking batches and  */
/* closed-loop engines read like any other ring, addressing it by absolute sample */
/* number AT THE OUTPUT RATE fs_in / D.  Mix-then-filter, the same mathematics as  */
/* GNU Radio's rotated-taps form.  The phase is a closed form of the sample number: */
/* it does not drift, needs no state and does not depend on the push sizes;         */
/* translate_hz = 0 skips the mixer, and T = 1, h = {1}, D = 1 is then a bit-exact   */
/* copy of the converted input.  Integer input is converted with a plain cast;       */
/* products and sums are float32, in tap order.  Output m exists once input mD has   */
/* been pushed: after N inputs the ring's head is ceil(N / D).  The filter delays the */
/* signal by its group delay, (T - 1) / 2 INPUT samples for symmetric taps, which is  */
/* the caller's to account for (e.g. in the code phase of a pseudorange), as in the   */
/* reference.                                                                  */
/* ------------------------------------------------------------------------ */
typedef struct
{
    double fs_in;          /* rate of the raw samples [Hz] */
    double translate_hz;   /* frequency moved to 0 (the reference's IF); |translate_hz| <= fs_in / 2 */
    uint32_t decimation;   /* D, 1..64 */
    uint32_t n_taps;       /* T, 1..1024 */
    int32_t in_format;     /* gc_iq_format or gc_raw_real_format of the raw samples */
    int32_t reserved;
} gc_conditioner_conf; /* 32 bytes */
/* sizeof(gc_conditioner_conf) as the library sees it (layout check of a binding; gc_abi_check covers the older structures) */
size_t gc_conditioner_conf_size(void);

typedef struct gc_conditioner gc_conditioner;
/* taps: n_taps real float32 (copied).  out_ring: an empty GC_IQ_F32 ring of the same context, or an empty GC_IQ_I16 / GC_IQ_I8 ring opened with
 * gc_stream_accept_quantised_output ("Integer output rings" below; any other integer ring is refused with GC_ERR_INVALID, as before
 * integer output existed); the conditioner keeps a reference on
 * it (the ring handle may be destroyed first) and is its only producer from here on: gc_stream_push / gc_stream_push_pinned on the
 * ring return GC_ERR_STATE.  The configuration and the taps are checked before anything touches a device. */
gc_status gc_conditioner_create(gc_ctx* ctx, const gc_conditioner_conf* conf, const float* taps, gc_stream* out_ring,
    gc_conditioner** out);
gc_status gc_conditioner_destroy(gc_conditioner* c);
/* Appends n_in raw samples (host memory, in_format) and enqueues the kernel for the outputs they complete.  first_out / n_out
 * (optional): the absolute number of the first new output and their count (0 when the push completes none).  The last T - 1 raw
 * samples stay in HBM for the next push: results do not depend on how the input is cut into pushes.  Asynchronous like
 * gc_stream_push (the output ring's copy stream; gc_stream_synchronize waits for it); at most capacity outputs per call. */
gc_status gc_conditioner_push(gc_conditioner* c, const void* host_raw, uint64_t n_in, uint64_t* first_out, uint64_t* n_out);
/* Same for a PAGE-LOCKED host buffer: no staging copy; the buffer stays untouched until gc_stream_synchronize() on the output ring. */
gc_status gc_conditioner_push_pinned(gc_conditioner* c, const void* pinned_host_raw, uint64_t n_in, uint64_t* first_out, uint64_t* n_out);
/* Raw samples pushed so far and the output ring's head, ceil(in_head / D) -- with pulse blanking ceil(decided / D), see below
 * (any pointer may be NULL). */
gc_status gc_conditioner_info(gc_conditioner* c, uint64_t* in_head, uint64_t* out_head);
/* Low-pass design for the conditioner (the reference's filter blocks take taps from the configuration or design them with
 * gr::filter::firdes::low_pass; Remez designs stay with the caller, who passes taps): a Hamming-windowed sinc of odd length
 *   T = (int)(53 fs / (22 transition_hz)), plus 1 when that is even              (53 dB: the Hamming window's attenuation)
 *   h[i] = g(i - M) * (0.54 - 0.46 cos(2 pi i / (T - 1))),  M = (T - 1) / 2,  w0 = 2 pi cutoff_hz / fs
 *   g(0) = w0 / pi,  g(k) = sin(k w0) / (k pi)
 * scaled so that sum(h) = gain (the response at DC); computed in double, returned as float32.  *n_taps receives T; taps may be
 * NULL to ask for T alone; GC_ERR_INVALID when T > capacity. */
gc_status gc_fir_low_pass(double gain, double fs, double cutoff_hz, double transition_hz, float* taps, int capacity, int* n_taps);

/* Integer output rings: the reference's Freq_Xlating_Fir_Filter takes output_item_type cshort or cbyte next to gr_complex
 * (float_to_short on each component; complex_float_to_complex_byte, i.e. volk_gnsssdr_32fc_convert_8ic: scale by 127, clamp, rintf),
 * and Fir_Filter has cshort -> cshort and cbyte -> cbyte.  Here the format is the output ring's: the conditioner and the ring
 * decimator (below) write a ring of any gc_iq_format, and the tracking batch, the closed-loop engine and acquisition read a
 * GC_IQ_I16 / GC_IQ_I8 ring at 4 / 2 bytes per sample instead of 8.
 *
 * y[m] is the float32 output defined above: the same accumulation, the same bits.  Into a GC_IQ_I16 ring (MIN = -32768,
 * MAX = 32767) or a GC_IQ_I8 ring (MIN = -128, MAX = 127) each component c of y[m] is stored as
 *
 *   v = c * scale                      one float32 product
 *   v = MAX if v > MAX;  MIN if v < MIN;  unchanged otherwise
 *   q = (intN) rintf(v)                round to nearest, ties to even
 *   a NaN component stores 0
 *
 * -- clamp first, then round: the order of volk_gnsssdr_32fc_convert_8ic_generic and of VOLK's 32f_s32f_convert_16i.  scale = 1
 * gives the reference's cshort output and Fir_Filter's cbyte output, scale = 127 Freq_Xlating_Fir_Filter's cbyte output.  scale
 * is a finite float32 > 0 and defaults to 1.  A component counts as CLIPPED when v > MAX or v < MIN: strict comparisons, made before
 * the rounding; a NaN is not clipped.  The library keeps a running count of clipped components per conditioner and per decimator;
 * every output sample is counted once, the copy the kernel writes behind the ring (for windows that would wrap) is not counted
 * again.  first_out, n_out, gc_conditioner_info, blanking and the real and 2-bit input formats behave as with a GC_IQ_F32 ring: all of
 * them count samples.  gc_stream_read on the ring returns int16 / int8 (re, im) pairs, as for a pushed ring.  A GC_IQ_F32 ring has
 * no scale: it holds y[m] itself, bit for bit what the library stored before integer rings existed.
 *
 * Quantising is lossy, so a ring takes it only when asked to: an integer ring is by default a ring for host pushes, and
 * gc_conditioner_create / gc_ring_decimator_create go on refusing it (GC_ERR_INVALID) exactly as they did before integer output existed
 * -- a float pipeline pointed at a cshort ring by mistake does not silently lose its precision.  gc_stream_accept_quantised_output
 * opens an integer ring for such a producer. */
/* Declares that the empty GC_IQ_I16 / GC_IQ_I8 ring `s` may become the output ring of a gc_conditioner or gc_ring_decimator.
 * GC_ERR_INVALID for a GC_IQ_F32 ring (nothing is quantised into it); GC_ERR_STATE once samples have been pushed or a producer
 * exists.  Touches no device.  The ring still takes host pushes until a producer is created on it. */
gc_status gc_stream_accept_quantised_output(gc_stream* s);
/* Only before the first push (GC_ERR_STATE afterwards).  GC_ERR_INVALID for a scale that is not finite and positive, and for a
 * conditioner whose output ring is GC_IQ_F32.  The arguments are checked before anything touches a device. */
gc_status gc_conditioner_set_output_scale(gc_conditioner* c, float scale);
/* The output ring's gc_iq_format, the scale in use and the clipped components so far (any pointer may be NULL).  Synchronous: waits
 * for the pushes so far and copies the counter back from the device.  A GC_IQ_F32 ring reports scale 1 and 0 clipped. */
gc_status gc_conditioner_output_info(gc_conditioner* c, int32_t* out_format, float* scale, uint64_t* clipped_components);

/* Real raw samples: one real channel sampled at an intermediate frequency, the other half of what the reference's
 * Freq_Xlating_Fir_Filter takes (freq_xlating_fir_filter.cc: input_item_type "float", "short", "byte" next to the complex types), and
 * the output of its unpack_byte_2bit_samples block (signal_source/gnuradio_blocks) taken packed, four samples to a byte.  Values of
 * gc_conditioner_conf.in_format for the conditioner ONLY: a gc_stream ring, the tracking engines and acquisition take the three
 * gc_iq_format values and reject these like any unknown value.  3..15 are not used.
 *
 * For a real raw sample x[n] (n = absolute number, x[n] = 0 for n < 0) the mixer's output is
 *
 *   z[n] = ( x[n] * cos(2 pi phi(n)),  -( x[n] * sin(2 pi phi(n)) ) )     one float32 product each
 *   z[n] = ( x[n], 0 )                                                     when inc = 0 (no mixer)
 *   y[m] = sum_k h[k] z[mD - k]                                            the accumulation of the complex formats
 *
 * with the phi, inc, cosine / sine, plain cast of integer input and tap order of the complex formats: every output compares equal
 * to what the matching complex format gives for the samples (x[n], 0) -- only the sign of a zero may differ -- while a sample takes
 * 4, 2, 1 or 1/4 bytes on its way to the device instead of 8, 4 or 2.  n_in, in_head, first_out and n_out count SAMPLES in every
 * format.  GC_RAW_REAL_2BIT: sample 4b + i is bits 2i .. 2i + 1 of byte b, least-significant pair first, read as a two's-complement
 * 2-bit integer (-2, -1, 0 or 1: the reference's `signed two_bit_sample : 2`, DC bias included); a push whose n_in is not a multiple
 * of 4 returns GC_ERR_INVALID before anything is enqueued (the reference's block works in whole bytes too); n_in = 0 stays legal. */
typedef enum
{
    GC_RAW_REAL_F32 = 16, /* one float32 per sample: "float" */
    GC_RAW_REAL_I16 = 17, /* one int16 per sample:   "short" */
    GC_RAW_REAL_I8 = 18,  /* one int8 per sample:    "byte" */
    GC_RAW_REAL_2BIT = 19 /* four samples per byte:  unpack_byte_2bit_samples */
} gc_raw_real_format;

/* Pulse blanking in the conditioner: the reference's interference mitigation Pulse_Blanking_Filter
 * (src/algorithms/input_filter/gnuradio_blocks/pulse_blanking_cc.cc, adapter .../adapters/pulse_blanking_filter.cc) on the device.
 * It acts on the RAW samples, by absolute sample number, BEFORE the mixer and the FIR: a pulse is removed before the low-pass smears
 * it over its neighbours (mixing does not change a segment's energy).  The reference's adapter with IF != 0 filters first and blanks
 * second; for IF = 0 the two orders are the same definition.
 *
 * Segment s is the raw samples [sL, (s + 1)L); E[s] is the sum of re^2 + im^2 over it (float32, plain cast of integer input).  The
 * state machine is the reference's, statement for statement, in float32:
 *
 *   state: n = 0, last_filtered = false, noise = 0
 *   for s = 0, 1, 2, ...:
 *     if n < segments_est and not last_filtered:
 *         noise = (float(n) * noise + E[s] / float(2L)) / float(n + 1);           pass
 *     else if E[s] / noise > threshold:  blank segment s (all L samples read as zero);  last_filtered = true
 *     else:  pass;  last_filtered = false;  if n > segments_reset: n = 0
 *     n = n + 1
 *
 * Quirk kept from the reference: after a reset n becomes 1, not 0, so the re-estimate starts as the mean of the OLD floor and one
 * new segment, and takes segments_est - 1 segments.  n is a uint32 and wraps where the reference's int32 overflows.
 * threshold: the upper pfa quantile of a chi-squared distribution with 2L degrees of freedom, rounded to float32
 * (gc_chi2_upper_quantile; the reference takes it from Boost), unless the caller supplies one.
 *
 * A segment is decided only once all L of its samples have been pushed (the reference never processes a partial segment either).
 * With blanking on, decided = floor(in_head / L) * L; output m exists once raw sample mD is decided; the ring's head is
 * ceil(decided / D), and gc_conditioner_info and the first_out / n_out of a push report exactly that.  Outputs, state and counters do
 * not depend on how the input is cut into pushes.  A conditioner on which blanking was never configured behaves exactly as without
 * this section: the same launches in the same order, the same bits.
 *
 * Real raw samples (GC_RAW_REAL_F32 / _I16 / _I8): the reference's blanking block takes gr_complex only, so this is the same
 * definition applied to one real component per sample.  The state machine is the one above; E[s] is the sum of x^2 over the
 * segment's L samples; the noise floor uses E[s] / float(L) in place of E[s] / float(2L); a threshold of 0 becomes the upper pfa
 * quantile of a chi-squared distribution with L degrees of freedom.  GC_RAW_REAL_2BIT: gc_conditioner_set_pulse_blanking returns
 * GC_ERR_INVALID -- zeroing a segment in place would need sub-byte read-modify-write across threads at its ragged edges. */
typedef struct
{
    float pfa;               /* false-alarm probability of one segment, 0 < pfa < 1 */
    float threshold;         /* 0: computed from pfa and length; otherwise finite and > 0, used as is */
    uint32_t length;         /* L, samples per segment, 1..4096 */
    uint32_t segments_est;   /* segments of a noise-floor estimate, >= 1 */
    uint32_t segments_reset; /* a passing segment with n above this starts a new estimate */
    uint32_t reserved;
} gc_blanking_conf; /* 24 bytes */
size_t gc_blanking_conf_size(void);
/* Only before the first push (GC_ERR_STATE afterwards).  The limits are checked before anything touches a device
 * (GC_ERR_INVALID). */
gc_status gc_conditioner_set_pulse_blanking(gc_conditioner* c, const gc_blanking_conf* conf);
/* Segments decided and blanked so far, the noise floor, n and the threshold in use (any pointer may be NULL).  Synchronous: waits
 * for the pushes so far and copies the state back from the device.  GC_ERR_STATE when blanking is not configured. */
gc_status gc_conditioner_blanking_info(gc_conditioner* c, uint64_t* segments_decided, uint64_t* segments_blanked, float* noise_power,
    uint32_t* n_segments, float* threshold);
/* x with P(chi-squared with dof degrees of freedom > x) = pfa, in double: the regularised upper incomplete gamma function (series /
 * continued fraction) inverted by safeguarded Newton steps.  dof > 0, 0 < pfa < 1. */
gc_status gc_chi2_upper_quantile(double dof, double pfa, double* out);

/* ------------------------------------------------------------------------ */
/* Level 2 -- batched tracking engine: all channels of a GPU, many epochs,    */
/* one launch; IQ, parameters and results resident in HBM.                    */
/* ------------------------------------------------------------------------ */

/* One channel-epoch of work: the arguments the reference hands to its two
 * kernels (resampler_32f_xn.h:77 / rotator_dot_prod_32fc_xn.h:81) for one call
 * of Carrier_wipeoff_multicorrelator_resampler, plus where the window starts. */
typedef struct
{
    uint64_t sample_offset;    /* first IQ sample of the window, relative to the channel's IQ base */
    float phase0_re, phase0_im;        /* lv_cmake(cos(rem_carr), -sin(rem_carr))   (.cc:141) */
    float phase_inc_re, phase_inc_im;  /* std::exp(lv_32fc_t(0, -phase_step_rad))   (.cc:149) */
    float phase_rate_re, phase_rate_im;/* std::exp(lv_32fc_t(0, -phase_rate_step))  (.cc:145); (1,0) = none */
    float rem_code_phase_chips;        /* in code samples = chips * samples_per_chip */
    float code_phase_step_chips;
    float code_phase_rate_step_chips;
    int32_t n_samples;                 /* integration length (signal_length_samples) */
} gc_epoch_params; /* 48 bytes */

/* Fills a gc_epoch_params from the reference's scalar arguments with the same
 * float arithmetic as cpu_multicorrelator_real_codes.cc:141-149 (host libm). */
void gc_epoch_params_fill(gc_epoch_params* p, uint64_t sample_offset,
    float rem_carrier_phase_in_rad, float phase_step_rad, float phase_rate_step_rad,
    float rem_code_phase_chips, float code_phase_step_chips, float code_phase_rate_step_chips,
    int signal_length_samples);

/* IQ sample formats accepted from HBM.  Integer formats are what SDR front-ends deliver and the reference
 * converts to gr_complex before its float correlators (volk_gnsssdr_16ic_convert_32fc,
 * pcps_acquisition.cc:676-679; data_type_adapter blocks): the engine converts on load (plain cast), so
 * results equal the float path on the converted samples while HBM bytes per sample drop from 8 to 4 / 2. */
typedef enum
{
    GC_IQ_F32 = 0, /* interleaved float32 (re, im): gr_complex / lv_32fc_t */
    GC_IQ_I16 = 1, /* interleaved int16   (re, im): lv_16sc_t ("cshort") */
    GC_IQ_I8 = 2   /* interleaved int8    (re, im): lv_8sc_t  ("cbyte") */
} gc_iq_format;

typedef struct gc_trk_batch gc_trk_batch;
/* n_channels channels with n_taps correlator taps each; code tables up to
 * max_code_length entries.  high_dyn selects the high-dynamics resampler +
 * rotator pair for every channel of the batch. */
gc_status gc_trk_batch_create(gc_ctx* ctx, int n_channels, int n_taps, int max_code_length,
    int high_dyn, gc_trk_batch** out);
gc_status gc_trk_batch_destroy(gc_trk_batch* b);
/* Uploads channel `ch`'s code table (float[code_length], +-1 or any real
 * replica) and tap shifts (float[n_taps], in code samples). (host pointers)
 * Setters take effect at the next run call; they wait for launches on the
 * context's own stream, but launches still in flight on a CALLER stream
 * (gc_trk_batch_run_dev) must be synchronised by the caller first. */
gc_status gc_trk_batch_set_code(gc_trk_batch* b, int ch, const float* code, int code_length,
    const float* shifts_chips);
gc_status gc_trk_batch_set_shifts(gc_trk_batch* b, int ch, const float* shifts_chips);
/* Complex chips for every channel of the batch (Cpu_Multicorrelator,
 * cpu_multicorrelator.cc:82-130): switch the batch with set_complex_codes(b, 1)
 * (drops the codes loaded so far; not available with high_dyn; max_code_length
 * <= 7936), then load code_length (re, im) pairs per channel. */
gc_status gc_trk_batch_set_complex_codes(gc_trk_batch* b, int on);
gc_status gc_trk_batch_set_code_complex(gc_trk_batch* b, int ch, const float* code_iq, int code_length,
    const float* shifts_chips);
/* Cpu_Multicorrelator_16sc arithmetic for every channel of the batch (see
 * gc_correlator_set_local_code_and_taps_16sc): set_16sc(b, 1) switches the
 * input format to GC_IQ_I16 and drops codes and inputs loaded so far (not
 * available with high_dyn); codes are code_length (re16, im16) pairs; the
 * output of run / run_dev is n_taps lv_16sc_t (4 bytes) per channel-epoch. */
gc_status gc_trk_batch_set_16sc(gc_trk_batch* b, int on);
gc_status gc_trk_batch_set_code_16sc(gc_trk_batch* b, int ch, const int16_t* code_iq, int code_length,
    const float* shifts_chips);
/* Sample format of every channel's IQ buffer (default GC_IQ_F32). */
gc_status gc_trk_batch_set_input_format(gc_trk_batch* b, int iq_format);
/* Points channel `ch` at its IQ samples in HBM (n_samples complex samples of the batch's format,
 * aligned to one sample).  Channels of one RF stream may share the same pointer. */
gc_status gc_trk_batch_set_input_dev(gc_trk_batch* b, int ch, const void* dev_iq, uint64_t n_samples);
/* Channel `ch` reads the ring `s` (same format as the batch): gc_epoch_params.sample_offset is then an
 * ABSOLUTE sample number of that stream and n_samples <= the stream's max_window.  gc_trk_batch_run checks
 * every window against the resident range; gc_trk_batch_run_dev cannot (parameters live in HBM): tell it the
 * oldest sample its launches read with set_read_floor so that later pushes need not wait for them (default:
 * everything resident, i.e. the next evicting push waits for the launch).  A floor below the resident range
 * is GC_ERR_STATE at the launch, a floor above the ring's head GC_ERR_INVALID: it would protect nothing the
 * launch reads.  A window whose sample_offset + n_samples passes 2^64 is refused like any other that is not
 * resident. */
gc_status gc_trk_batch_set_input_stream(gc_trk_batch* b, int ch, gc_stream* s);
gc_status gc_trk_batch_set_read_floor(gc_trk_batch* b, uint64_t oldest_index_read);
/* Correlates n_epochs epochs of every channel.  dev_params: n_channels*n_epochs
 * gc_epoch_params, channel-major.  dev_out: n_channels*n_epochs*n_taps complex.
 * Asynchronous on `stream`. */
gc_status gc_trk_batch_run_dev(gc_trk_batch* b, int n_epochs, const gc_epoch_params* dev_params,
    void* dev_out, void* stream);
/* Same with host parameter/result buffers (copies + synchronises). */
gc_status gc_trk_batch_run(gc_trk_batch* b, int n_epochs, const gc_epoch_params* host_params,
    float* host_out);
/* Engine tuning (no reference counterpart).  Nominal integration length: lets
 * gc_trk_batch_run_dev pick how many slices to cut an epoch into when the
 * batch alone would not fill the GPU, and size the LDS code window of a launch by what
 * one slice of such an epoch touches (long codes: Galileo E1's 8184 samples are cut in
 * two so that a workgroup holds half the table; gc_trk_batch_run_dev assumes ONE code period
 * per nominal window, gc_trk_batch_run reads the code steps of its records).  Results never
 * depend on it: a record outside the bound is served from the whole table, in LDS when the
 * launch's LDS holds it, from global memory otherwise (slower: a batch of long codes whose
 * windows span several code periods should use set_slices(-1)).  set_slices(0) = automatic;
 * set_slices(-1) = automatic slicing by load only, the window sized for the longest code
 * (the behaviour before round 4; A/B timing). */
gc_status gc_trk_batch_set_nominal_length(gc_trk_batch* b, int n_samples);
gc_status gc_trk_batch_set_slices(gc_trk_batch* b, int n_slices);

/* ------------------------------------------------------------------------ */
/* Level 3 -- closed-loop tracking on the device: the correlations AND the      */
/* per-epoch DLL/PLL maths of dll_pll_veml_tracking run inside one launch for    */
/* n_epochs code periods per channel (no host round trip per millisecond).       */
/* ------------------------------------------------------------------------ */

/* What the tracking block knows when start_tracking() is called: the Dll_Pll_Conf fields it reads
 * (src/algorithms/tracking/libs/dll_pll_conf.h:39-80), the per-signal constants of its constructor
 * (dll_pll_veml_tracking.cc:113-330) and the acquisition hand-over from Gnss_Synchro (:555-557). */
typedef struct
{
    double fs_in;
    double signal_carrier_freq_hz;
    double code_chip_rate_hz;
    double code_period_s;
    double carrier_lock_th;
    double acq_delay_samples;          /* Gnss_Synchro::Acq_delay_samples */
    double acq_doppler_hz;             /* Gnss_Synchro::Acq_doppler_hz */
    uint64_t acq_samplestamp_samples;  /* Gnss_Synchro::Acq_samplestamp_samples */
    uint64_t sample_counter;           /* stream sample count at the first sample of the channel's IQ buffer */
    uint32_t code_length_chips;
    uint32_t code_samples_per_chip;
    uint32_t vector_length;
    uint32_t pull_in_time_s;
    int32_t veml;                      /* != 0: 5 taps VE/E/P/L/VL (Galileo E1), else 3 taps E/P/L */
    int32_t pll_filter_order, dll_filter_order;
    int32_t enable_fll_pull_in, enable_fll_steady_state;
    int32_t cn0_samples, cn0_min, max_lock_fail;
    float pll_bw_hz, dll_bw_hz, fll_bw_hz;
    float early_late_space_chips, very_early_late_space_chips;
    uint32_t high_dyn_smoother_length; /* 0: Dll_Pll_Conf::high_dyn false; n > 0: high_dyn with smoother_length n (<= 16): the
                                        * high-dynamics resampler / rotator kernels and the carrier / code rate smoothers of
                                        * update_tracking_vars (:1016-1033, :1047-1064) */
} gc_loop_conf;

/* One code period of one channel: the correlator outputs plus what the block writes to Gnss_Synchro
 * (dll_pll_veml_tracking.cc:1730-1770, 1898-1906) and to its binary dump (:1196-1243). */
typedef struct
{
    float corr[10];              /* n_taps complex correlator outputs (re, im); in a mixed engine (gc_trk_loop_set_mixed)
                                  * each channel's own tap count */
    float carrier_doppler_hz, code_freq_chips;
    float carr_phase_error_hz, carr_error_filt_hz, code_error_chips, code_error_filt_chips;
    float cn0_db_hz, carrier_lock_test;
    uint64_t sample_counter;     /* Tracking_sample_counter after this epoch */
    double acc_carrier_phase_rad;
    double rem_code_phase_samples;
    int32_t state;               /* d_state after this code period: 0 = standby (after loss of lock), 1 = pull-in pending,
                                  * 2 = wide tracking / symbol synchronisation, 3 = extended integration, 4 = narrow tracking */
    int32_t valid;               /* Flag_valid_symbol_output */
    int32_t current_prn_length_samples;
    int32_t extend_count;        /* d_extend_correlation_symbols_count when log_data ran (scale factor of the dump, :1179-1191) */
    float accu[10];              /* d_VE/E/P/L/VL_accu as log_data sees them (before the reset that follows a loop update) */
    float prompt_data[2];        /* d_Prompt_Data (pilot tracking: prompt of the data component), else the prompt tap */
    int32_t integrating;         /* 1: the period only accumulated (state 3, log_data(true)); 0: the loop filters ran */
    int32_t reserved;
} gc_loop_record;

/* Symbol synchronisation, extended integration and pilot tracking (dll_pll_veml_tracking.cc:1601-1896): what the block's
 * constructor derives from the signal (:113-336) plus the Dll_Pll_Conf fields of the narrow stage.  Without it a channel
 * stays in state 2 (1 code period per loop update, data component), which is what the block does for a signal whose
 * telemetry preamble is never found. */
typedef struct
{
    int32_t extend_correlation_symbols;   /* Dll_Pll_Conf::extend_correlation_symbols (>= 1; 1 = no extension) */
    int32_t track_pilot;                  /* Dll_Pll_Conf::track_pilot: `code` of gc_trk_loop_start is the pilot replica,
                                           * data_code the data component's; four-quadrant PLL once the secondary code is locked */
    int32_t symbols_per_bit;              /* d_symbols_per_bit */
    int32_t secondary_code_length;        /* d_secondary_code_length, 0 = no secondary code (<= 128) */
    int32_t preamble_length_symbols;      /* d_preamble_length_symbols, 0 = none (<= 192) */
    float bit_sync_min_time_s;            /* tracking time before the preamble search starts: 10 in the reference (:1648) */
    float pll_bw_narrow_hz, dll_bw_narrow_hz;
    float early_late_space_narrow_chips, very_early_late_space_narrow_chips;
    char secondary_code[128];             /* '0' / '1', like the reference's secondary-code strings */
    int8_t preamble_symbols[192];         /* +1 / -1 (d_preambles_symbols) */
} gc_loop_sync_conf;

/* Fills the signal-dependent part of a gc_loop_sync_conf the way the block's constructor and start_tracking do
 * (dll_pll_veml_tracking.cc:113-336, :631-705): symbols per bit, secondary code, telemetry preamble for
 * system / signal 'G' "1C" | "2S" | "L5", 'E' "1B" | "5X", 'C' "B1" | "B3" and the satellite `prn` (BeiDou GEO 1..5 broadcast D2;
 * Galileo E5a-Q has one secondary code per PRN).  track_pilot is cleared for signals without a pilot component;
 * bit_sync_min_time_s is set to the reference's 10 s; the narrow-stage fields are left for the caller (Dll_Pll_Conf). */
gc_status gc_loop_sync_for_signal(char system, const char* signal, uint32_t prn, int track_pilot, int extend_correlation_symbols,
    gc_loop_sync_conf* out);

typedef struct gc_trk_loop gc_trk_loop;
gc_status gc_trk_loop_create(gc_ctx* ctx, int n_channels, int max_code_length, gc_trk_loop** out);
gc_status gc_trk_loop_destroy(gc_trk_loop* l);
/* Sample format of every channel's input (default GC_IQ_F32; cshort / cbyte samples are converted on load like
 * in the batched engine).  Call before binding inputs. */
gc_status gc_trk_loop_set_input_format(gc_trk_loop* l, int iq_format);
/* IQ block of channel `ch` in HBM (samples of the engine's format); epochs are correlated until it is exhausted. */
gc_status gc_trk_loop_set_input_dev(gc_trk_loop* l, int ch, const void* dev_iq, uint64_t n_samples);
/* Channel `ch` reads the RF stream ring `s` (same sample format) instead of a fixed block: bind before
 * gc_trk_loop_start; the channel then starts at absolute sample gc_loop_conf.sample_counter and every launch
 * correlates the code periods that are complete in the ring at that moment (the remaining records of the
 * launch are marked invalid, state unchanged), so "push a block, run" is the whole host loop.
 * gc_trk_loop_run reports GC_ERR_STATE when a channel has fallen behind the ring's oldest sample. */
gc_status gc_trk_loop_set_input_stream(gc_trk_loop* l, int ch, gc_stream* s);
/* Installs (sync != NULL) or removes the synchronisation / extension description of channel `ch`; it takes effect at the
 * next gc_trk_loop_start.  data_code (data_code_length floats, same length as the tracking replica) is required with
 * track_pilot and ignored otherwise.  All channels of a default engine share the pilot mode; a mixed engine
 * (gc_trk_loop_set_mixed) takes it per channel. */
gc_status gc_trk_loop_set_sync(gc_trk_loop* l, int ch, const gc_loop_sync_conf* sync, const float* data_code, int data_code_length);
/* dll_pll_veml_tracking::start_tracking (:549-747): uploads the replica (code_length_chips *
 * code_samples_per_chip floats), sets the taps from the spacings and initialises the loop.  In a default engine every
 * running channel has the same tap count (veml) and pilot mode; a mixed engine (gc_trk_loop_set_mixed) lifts both checks.
 * The high_dyn mode is always shared by the running channels of one engine. */
gc_status gc_trk_loop_start(gc_trk_loop* l, int ch, const gc_loop_conf* conf, const float* code, int code_length);
/* Puts channel `ch` back in standby (all-zero records, state 0) until the next gc_trk_loop_start; channels that were never
 * started are in the same state, so an engine can be sized for the receiver's channel count and filled as acquisitions succeed. */
gc_status gc_trk_loop_stop(gc_trk_loop* l, int ch);
/* n_epochs code periods of every channel in ONE launch.  dev_records: n_channels*n_epochs records,
 * channel-major.  The loop state persists on the device between calls. */
/* Launch geometry of the engine, for tests and tuning (0 = automatic, the default): threads per workgroup (256, 512 or 1024; the
 * default follows the channel count) and workgroups per channel-period.  slices_per_channel > 1 (a period cut into slices, one launch
 * per code period, the last slice to finish runs the loop maths) measured slower than one workgroup per channel (13.4 vs 11.4 us per
 * period at 32 channels) and is accepted by experiments builds only; the product library takes 0 or 1. */
gc_status gc_trk_loop_set_geometry(gc_trk_loop* l, int threads_per_workgroup, int slices_per_channel);
/* Mixed mode (on != 0): every channel slot carries its own tap count (3 or 5), pilot mode, code length and code period, and
 * all channels still run in one launch on one stream (a hybrid receiver: GPS L1 C/A, Galileo E1 and BeiDou B1I slots on one
 * RF stream).  The launch sizes its LDS code image for the largest need among the started channels.  Run semantics do not
 * change: n_epochs is the capacity per channel, and a channel whose input ends (the n_samples of gc_trk_loop_set_input_dev,
 * or the ring's head) writes invalid records after that, so a caller that wants T seconds of every channel sizes n_epochs
 * for the SHORTEST code period (64 ms of GPS: 64 records, of which a 4 ms Galileo E1 channel fills 16).  high_dyn stays
 * engine-wide.  Allowed only while no channel is started (GC_ERR_STATE otherwise); a mixed engine runs one workgroup per
 * channel (no slices_per_channel > 1). */
gc_status gc_trk_loop_set_mixed(gc_trk_loop* l, int on);
gc_status gc_trk_loop_run_dev(gc_trk_loop* l, int n_epochs, gc_loop_record* dev_records, void* stream);
gc_status gc_trk_loop_run(gc_trk_loop* l, int n_epochs, gc_loop_record* host_records);

/* GLONASS L1 / L2 C/A channels of a loop engine: the reference tracks them with a block of its own
 * (glonass_l1_ca_dll_pll_tracking_cc.cc / glonass_l2_...: start_tracking :160-243, general_work :549-777) whose loop is not the
 * veml loop -- second-order Tracking_2nd_DLL_filter / Tracking_2nd_PLL_filter, the FDMA channel offset in the carrier NCO but
 * not in the Doppler, a block length round()-ed every period with the code NCO command folded in (the period correlates the
 * length of the previous update and consumes the new one), a C/N0 window of its own.  What the block knows at start_tracking(): */
typedef struct
{
    double fs_in;                     /* a whole number of samples per second (the block's int64_t fs_in) */
    double band_carrier_freq_hz;      /* 1.602e9 (L1) or 1.246e9 (L2) */
    double channel_offset_hz;         /* DFRQ * k of the slot: 0.5625e6 * k or 0.4375e6 * k */
    double carrier_lock_th;
    double acq_delay_samples, acq_doppler_hz;
    uint64_t acq_samplestamp_samples, sample_counter;
    uint32_t vector_length;           /* round(fs_in / 1000) */
    int32_t cn0_samples, cn0_min, max_lock_fail;   /* cn0_samples 1..64 */
    float pll_bw_hz, dll_bw_hz, early_late_space_chips;
    uint32_t reserved;
} gc_glonass_loop_conf;
size_t gc_glonass_loop_conf_size(void);
/* start_tracking of the GLONASS block for channel `ch`; the library generates the 511-chip replica itself (the engine's
 * max_code_length must be >= 511).  Input binding, stop, geometry, run and run_dev are those of every loop engine.  The running
 * channels of an engine are all veml (gc_trk_loop_start) or all GLONASS: starting the other kind while a channel runs is
 * GC_ERR_STATE, and so is a GLONASS start on a mixed engine (gc_trk_loop_set_mixed) -- a receiver runs a GLONASS engine beside
 * its other engine.  With ring input 2 * vector_length <= the stream's max_window (GC_ERR_INVALID
 * otherwise, like every argument out of range).  Every argument is checked before anything touches a device.
 * A period runs only when its whole block [position, position + current block length) lies below the launch's limit (the end of
 * the bound block, or the ring's head); otherwise that epoch and every later one of the launch write invalid records (all zero
 * but `state` and `sample_counter`) and the state is unchanged, so records do not depend on how input is cut into pushes or
 * launches.  The pull-in alignment runs before the first period and emits no record.  Loss of lock (the fail counter exceeds
 * max_lock_fail): that period's record is still valid, the channel then sits in state 0 like a veml channel that lost lock.
 * Deviation from the reference, which reads past the 2 * vector_length items its scheduler guarantees: a new block length outside
 * [1, 2 * vector_length] ends tracking the same way (state 0, a lost-lock event) and that period consumes nothing.
 * gc_loop_record of a GLONASS channel:
 *   corr[0..5]                    E, P, L
 *   accu[0..5]                    the same values
 *   prompt_data                   the prompt
 *   carrier_doppler_hz            Doppler WITHOUT the FDMA offset
 *   code_freq_chips               code frequency after the update
 *   carr_phase_error_hz / carr_error_filt_hz      PLL discriminator output (cycles) and the PLL filter's output
 *   code_error_chips / code_error_filt_chips      DLL discriminator output and the DLL filter's output
 *   cn0_db_hz, carrier_lock_test  as in the block
 *   sample_counter                the block's Tracking_sample_counter: counter + new block length
 *   acc_carrier_phase_rad, rem_code_phase_samples as in the block
 *   current_prn_length_samples    the new block length
 *   state                         0 standby / 1 pull-in pending / 2 tracking
 *   valid                         1
 *   integrating, extend_count     0
 * A second deviation: a start is the start of a fresh block object.  The reference's start_tracking keeps the C/N0 window's fill, the
 * last C/N0 and the last lock test of the object's previous run; here every start clears them (C/N0 0, lock test 1 until the first
 * estimate), whatever the slot tracked before. */
gc_status gc_trk_loop_start_glonass(gc_trk_loop* l, int ch, const gc_glonass_loop_conf* conf);
/* The pull-in alignment that a start with `conf` performs before its first period (glonass_l1_ca_dll_pll_tracking_cc.cc:570-590),
 * computed on the host by the statements the kernel runs; needs no device.  Any output pointer may be NULL: the samples skipped,
 * the block's d_sample_counter behind them (the Tracking_sample_counter of the item the block writes there) and its
 * d_acc_carrier_phase_rad.  The loop fields of `conf` (bandwidths, C/N0 settings, vector_length) are not read. */
gc_status gc_glonass_loop_pull_in(const gc_glonass_loop_conf* conf, int32_t* samples_offset, uint64_t* sample_counter, double* acc_carrier_phase_rad);

/* ------------------------------------------------------------------------ */
/* PRN replica generators (host side, set-up path).  Same outputs as the      */
/* reference's generators; dest buffers are caller-owned host memory.         */
/* ------------------------------------------------------------------------ */
/* gps_l1_ca_code_gen_float (src/algorithms/libs/gps_sdr_signal_processing.cc:119-130): 1023 chips, +-1;
 * PRN 1..32 and SBAS 120..138 */
gc_status gc_gps_l1_ca_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift);
/* gps_l1_ca_code_gen_complex_sampled (…:151-196): (int)(fs/1000) complex samples; *n_samples (optional) = count */
gc_status gc_gps_l1_ca_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, uint32_t chip_shift, int32_t* n_samples);
/* glonass_l1_ca_code_gen_complex / _complex_sampled (src/algorithms/libs/glonass_l1_signal_processing.cc:37-153;
 * glonass_l2_signal_processing.cc is the same sequence): 511 chips, one code for every satellite (FDMA).  The float
 * form holds the real parts (the reference's chips are (+-1, 0)); sampled: (int)(fs/1000) complex samples. */
gc_status gc_glonass_l1_ca_code_gen_float(float* dest, uint32_t chip_shift);
gc_status gc_glonass_l1_ca_code_gen_complex_sampled(float* dest, int32_t fs, uint32_t chip_shift, int32_t* n_samples);
/* beidou_b1i_code_gen_float / _complex_sampled (src/algorithms/libs/beidou_b1i_signal_processing.cc:115-191): 2046 chips */
gc_status gc_beidou_b1i_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift);
gc_status gc_beidou_b1i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, uint32_t chip_shift, int32_t* n_samples);
/* galileo_e1_code_gen_sinboc11_float (src/algorithms/libs/galileo_e1_signal_processing.cc:108-119): 8184 samples
 * (2 per chip) of the E1-B ("1B") or E1-C ("1C") primary code, PRN 1..50.  The memory codes are read from
 * data/galileo_e1_primary_codes.bin next to the library (or $GNSSCORR_GALILEO_E1_CODES). */
gc_status gc_galileo_e1_code_gen_sinboc11_float(float* dest, const char* signal, uint32_t prn);
/* galileo_e1_code_gen_complex_sampled (…:232-255) without secondary code: 4 ms of samples at fs */
gc_status gc_galileo_e1_code_gen_complex_sampled(float* dest, const char* signal, int32_t cboc, uint32_t prn, int32_t fs,
    uint32_t chip_shift, int32_t* n_samples);
/* The 10.23 / 0.5115 Mcps signals.  Their per-PRN constants (IS-GPS-200 Table 3-IIa, IS-GPS-705 Table 3-Ia/Ib, BDS-SIS-ICD-B3I
 * G2 phases, Galileo OS SIS ICD E5a memory codes) are read from data/prn_tables.bin and data/galileo_e5a_primary_codes.bin
 * next to the library (or $GNSSCORR_DATA_DIR).  All codes are 10230 chips.
 * gps_l2c_m_code_gen_float / _complex_sampled (src/algorithms/libs/gps_l2c_signal.cc:75-137): PRN 1..50; the sampled form
 * holds (int)(fs / 50) complex samples (one 20 ms code) and digitises with a true ceil() */
gc_status gc_gps_l2c_m_code_gen_float(float* dest, uint32_t prn);
gc_status gc_gps_l2c_m_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, int32_t* n_samples);
/* gps_l5i / gps_l5q _code_gen_float / _complex_sampled (src/algorithms/libs/gps_l5_signal.cc:197-344): PRN 1..50 */
gc_status gc_gps_l5i_code_gen_float(float* dest, uint32_t prn);
gc_status gc_gps_l5q_code_gen_float(float* dest, uint32_t prn);
gc_status gc_gps_l5i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, int32_t* n_samples);
gc_status gc_gps_l5q_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, int32_t* n_samples);
/* beidou_b3i_code_gen_float / _complex_sampled (src/algorithms/libs/beidou_b3i_signal_processing.cc:37-246): PRN 1..63 */
gc_status gc_beidou_b3i_code_gen_float(float* dest, int32_t prn, uint32_t chip_shift);
gc_status gc_beidou_b3i_code_gen_complex_sampled(float* dest, uint32_t prn, int32_t fs, uint32_t chip_shift, int32_t* n_samples);
/* galileo_e5_a_code_gen_complex_primary / _complex_sampled (src/algorithms/libs/galileo_e5_signal_processing.cc:38-142):
 * 10230 complex chips; signal "5I" -> (I, 0), "5Q" -> (0, Q), "5X" -> (I, Q); PRN 1..50 */
gc_status gc_galileo_e5_a_code_gen_complex_primary(float* dest, int32_t prn, const char* signal);
gc_status gc_galileo_e5_a_code_gen_complex_sampled(float* dest, const char* signal, uint32_t prn, int32_t fs, uint32_t chip_shift,
    int32_t* n_samples);
/* Secondary (overlay) code of a signal as a '0'/'1' string, the form gc_loop_sync_conf.secondary_code takes and the reference
 * keeps in its system_parameters headers: "1C" (Galileo E1-C CS25), "B1" / "B3" (BeiDou NH20), "L5I" (NH10), "L5Q" (NH20),
 * "5I" (Galileo E5a-I CS20), "5Q" (E5a-Q CS100 of `prn`; the reference's table holds PRN 1..47).  prn is ignored otherwise. */
gc_status gc_secondary_code(const char* signal, uint32_t prn, char* dest, int32_t capacity, int32_t* length);

/* ------------------------------------------------------------------------ */
/* Acquisition -- PCPS (parallel code phase search), batched over satellites. */
/* ------------------------------------------------------------------------ */

/* Image of Acq_Conf (src/algorithms/acquisition/libs/acq_conf.h:38-66), the
 * fields pcps_acquisition reads on this path, plus doppler_step (set through
 * set_doppler_step in the reference, pcps_acquisition.h:228). */
typedef struct
{
    int64_t fs_in;
    uint32_t sampled_ms;
    uint32_t ms_per_code;
    float samples_per_ms;
    float samples_per_code;
    uint32_t samples_per_chip;
    uint32_t doppler_max;
    uint32_t doppler_step;
    uint32_t max_dwells;
    int32_t bit_transition_flag;
    int32_t use_CFAR_algorithm_flag;
    /* engine extension: when > 0 overrides ceil(2*doppler_max/doppler_step)
     * (pcps_acquisition.cc:326) as the number of Doppler bins */
    uint32_t num_doppler_bins_override;
    /* two-step acquisition (Acq_Conf::make_2_steps, num_doppler_bins_step2, doppler_step2;
     * defaults 4 bins of 125 Hz, gps_l1_ca_pcps_acquisition.cc:86-88) */
    int32_t make_2_steps;
    uint32_t num_doppler_bins_step2;
    float doppler_step2;
} gc_acq_conf;

/* Per-satellite result of one dwell: what acquisition_core leaves in
 * Gnss_Synchro / d_test_statistics / d_mag / d_input_power (:747-768). */
typedef struct
{
    uint32_t indext;          /* argmax code-phase index in the grid row */
    int32_t doppler_hz;       /* -doppler_max + doppler_step*row (:588) */
    uint32_t doppler_index;
    float test_statistics;    /* CFAR: max/N^4/input_power; else first/second peak */
    float mag;                /* raw grid maximum */
    float input_power;
    float second_peak;          /* as the reference computes it (the N-byte memcpy at :647) */
    float second_peak_full_row; /* second peak with the whole peak row considered */
    double acq_delay_samples; /* fmod((float)indext, samples_per_code) (:766) */
    double acq_doppler_hz;
} gc_acq_result;

typedef struct gc_acq gc_acq;
/* pcps_acquisition ctor + init() for n_sats satellites searched at once. */
gc_status gc_acq_create(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, gc_acq** out);
gc_status gc_acq_destroy(gc_acq* a);
gc_status gc_acq_fft_size(const gc_acq* a, uint32_t* fft_size, uint32_t* consumed_samples,
    uint32_t* num_doppler_bins);
/* pcps_acquisition::set_local_code for satellite slot `sat` (host pointer to
 * consumed_samples complex; fft_size/2 with bit_transition_flag). */
gc_status gc_acq_set_local_code(gc_acq* a, int sat, const float* code);
/* d_old_freq of the reference (pcps_acquisition.cc:242-247, :276-293, :371-380): a frequency added to every bin of
 * the coarse Doppler grid -- an intermediate frequency, or the GLONASS FDMA channel offset DFRQ1_GLO * k the reference
 * installs in set_local_code() for "1G" / "2G" signals.  Rebuilds the wipe-off table (float32 running phase);
 * reported Doppler values stay relative to the offset, as in the reference.  Default 0. */
gc_status gc_acq_set_frequency_offset(gc_acq* a, int64_t offset_hz);
/* New search: the dwell counter restarts and the magnitude grids read as zero (the first dwell after a
 * reset overwrites them; nothing is enqueued by this call, so it needs no stream). */
gc_status gc_acq_reset(gc_acq* a);
/* Second step of make_2_steps (pcps_acquisition.cc:771-829, 957-963): enable != 0 switches the search to
 * num_doppler_bins_step2 bins of doppler_step2 Hz centred on doppler_center_hz
 * (update_grid_doppler_wipeoffs_step2, :383-390) and restarts the dwell counter; enable == 0 returns to
 * the coarse grid.  Results then follow the step-two Doppler formula (:589-591). */
gc_status gc_acq_set_step_two(gc_acq* a, int enable, float doppler_center_hz);
/* Sample format of the device input blocks of gc_acq_dwell_dev / gc_acq_dwell_enqueue (default GC_IQ_F32;
 * GC_IQ_I16 is the block's "cshort" item type, converted like volk_gnsssdr_16ic_convert_32fc does,
 * pcps_acquisition.cc:676-679).  gc_acq_dwell (host pointer) always takes gr_complex. */
gc_status gc_acq_set_input_format(gc_acq* a, int iq_format);
/* One dwell of acquisition_core for every satellite on the same input block
 * (consumed_samples complex).  Non-coherent accumulation across calls like the
 * reference (d_num_noncoherent_integrations_counter).  results: n_sats. */
gc_status gc_acq_dwell_dev(gc_acq* a, const void* dev_iq, gc_acq_result* host_results, void* stream);
gc_status gc_acq_dwell(gc_acq* a, const float* host_iq, gc_acq_result* host_results);
/* Enqueue-only variant for throughput runs: results stay in HBM until
 * gc_acq_fetch_results().  The input block has been consumed (in stream order) when the call returns its work to `stream`.
 * Dwells of one search enqueued back to back on one stream are searched in PAIRS (pcps_acquisition.cc:730-739 adds the second
 * |.|^2 to the first; here both are added in one pass and the grid is written once): the inverse passes of a dwell with
 * dwell counter < max_dwells are held back until the next call on the handle -- an accumulating dwell joins it, anything else
 * (fetch, grid read, new code, reset ...) first completes it alone or, for a reset, discards it.  Results and grids are bit-identical
 * to per-dwell processing; a gc_acq_flush() behind every dwell gives per-dwell processing (the evaluation after every dwell of pcps_acquisition.cc:747-755). */
gc_status gc_acq_dwell_enqueue(gc_acq* a, const void* dev_iq, void* stream);
gc_status gc_acq_fetch_results(gc_acq* a, gc_acq_result* host_results, void* stream);
/* Enqueues on `stream` whatever the enqueue-only calls have held back -- the inverse passes of a dwell waiting for a partner
 * and the statistics kernel of the last dwell (pcps_acquisition.cc:747-755 evaluates after every dwell) -- without copying
 * anything to the host and without synchronising: afterwards the device-side results are those of the last dwell, in stream
 * order.  gc_acq_fetch_results() = this + the copy + a stream synchronisation. */
gc_status gc_acq_flush(gc_acq* a, void* stream);
/* One dwell on the block of consumed_samples that starts at absolute sample first_index of the ring `s`
 * (the stream's format must equal gc_acq_set_input_format's; synchronous like gc_acq_dwell). */
gc_status gc_acq_dwell_stream(gc_acq* a, gc_stream* s, uint64_t first_index, gc_acq_result* host_results);
/* Copies satellite `sat`'s magnitude grid (num_doppler_bins * fft_size floats) to host. */
gc_status gc_acq_get_grid(gc_acq* a, int sat, float* host_grid);

/* Paired engine: every satellite slot holds TWO replicas, A and B, and each dwell searches both against the same spectra -- the
 * operation the reference ships three times:
 *   pcps_cccwsr_acquisition_cc.cc:316-370          data and pilot correlations combined as d + jp and d - jp, the larger wins
 *   galileo_pcps_8ms_acquisition_cc.cc:303-345     two sign hypotheses of an 8 ms replica, the larger wins
 *   galileo_e5a_noncoherent_iq_acquisition_caf_cc  |corr_I|^2 + |corr_Q|^2
 * For every dwell, Doppler bin and sample, with a = |IFFT(X_bin conj(FFT(A)))|^2 and b the same for B:
 *   GC_ACQ_COMBINE_MAX   c = max(a, b)
 *   GC_ACQ_COMBINE_SUM   c = a + b   (float32, a first)
 * The grid gets c on the first dwell and prev + c on later dwells: c stands wherever a one-replica dwell puts its |.|^2 (grid, row
 * maxima, the scratch image of the second-peak search, gc_acq_result, gc_acq_get_grid, GC_ACQ_PEEK_ROW_MAX), and the two |.|^2 are
 * combined on the device before the cell is written once.  CCCWSR is two complex replicas by linearity: d + jp belongs to
 * A = cd - j cp and d - jp to B = cd + j cp (gc_cccwsr_replicas).  Any other `combine` returns GC_ERR_INVALID.  Everything else --
 * conf, bit transition, step two, frequency offset, input formats, the enqueue / flush / fetch calls -- is gc_acq_create's; dwells
 * enqueued back to back are never held back for one another and give the results of one gc_acq_dwell per block, bit for bit. */
enum { GC_ACQ_COMBINE_MAX = 1, GC_ACQ_COMBINE_SUM = 2 };
gc_status gc_acq_create_paired(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, int combine, gc_acq** out);
/* set_local_code of both replicas of slot `sat` (pcps_cccwsr_acquisition_cc.cc:161-179, galileo_pcps_8ms_acquisition_cc.cc:147-166):
 * two host pointers with the length rules of gc_acq_set_local_code; an all-zero replica is legal (its |.|^2 is 0).  Paired engines
 * only: GC_ERR_INVALID on a gc_acq_create engine, as gc_acq_set_local_code is on a paired one. */
gc_status gc_acq_set_local_code_pair(gc_acq* a, int sat, const float* code_a, const float* code_b);
/* The replica pairs of the reference's two-hypothesis blocks, n complex samples each (interleaved floats; outputs may not alias inputs):
 *   gc_cccwsr_replicas   A = cd - j cp, B = cd + j cp: |d + jp|^2 and |d - jp|^2 of pcps_cccwsr_acquisition_cc.cc:342-351 are the
 *                        |.|^2 of the correlations with A and B
 *   gc_e1_8ms_replicas   A = code, B = code with its second code period [samples_per_code, 2 * samples_per_code) negated
 *                        (galileo_pcps_8ms_acquisition_cc.cc:150-165); n >= 2 * samples_per_code */
gc_status gc_cccwsr_replicas(const float* code_data, const float* code_pilot, uint32_t n, float* replica_a, float* replica_b);
gc_status gc_e1_8ms_replicas(const float* code, uint32_t n, uint32_t samples_per_code, float* replica_a, float* replica_b);
/* QuickSync engine (pcps_quicksync_acquisition_cc.cc): with N = samples_per_code, f = folding_factor, M = N / f (integer division)
 * and L = f N, a dwell wipes the carrier off L samples, folds the f * f pieces of M samples into one (float32 products and sums,
 * first piece first), correlates circularly at FFT size M against the code folded the same way, and then resolves the f aliased
 * delays k* + i M of the winning cell by f time-domain correlations with the unfolded code -- on the device, with no host round trip.
 *   Doppler bins    -doppler_max + b doppler_step for every value <= +doppler_max (the grid is INCLUSIVE: 21 bins for 5000 / 500,
 *                   :226-231); a doppler_step of 0 means 250 (:219-222); num_doppler_bins_override as in gc_acq_create
 *   conf fields     fs_in, sampled_ms, samples_per_ms, samples_per_code, doppler_max, doppler_step, max_dwells,
 *                   bit_transition_flag, num_doppler_bins_override.  The last two of the block's own parameters only steer its decision
 *                   state machine (:503-527), which lives with the caller (adapter/hip_pcps_quicksync_acquisition.h): every dwell
 *                   stands alone, overwrites the grid, and dwells are never held back for one another
 *   GC_ERR_INVALID  folding_factor outside 1 .. 100, M < 1, sampled_ms * samples_per_ms < L, make_2_steps set
 * On such a handle gc_acq_fft_size reports M, L and the inclusive bin count; gc_acq_set_local_code takes ONE code period of N
 * complex samples; a dwell consumes L samples; gc_acq_get_grid gives num_doppler_bins * M floats, |IFFT_M(.)|^2 unnormalised;
 * gc_acq_peek gives 2 L floats for WIPEOFF and 2 M for SPECTRUM and CODE; input formats, rings, enqueue / flush / fetch work as
 * documented above.  gc_acq_set_step_two, gc_acq_set_frequency_offset and gc_acq_set_local_code_pair return GC_ERR_INVALID.
 * gc_acq_result: indext = k* (folded index of the first grid maximum, bins ascending), doppler_index / doppler_hz / acq_doppler_hz
 * of its bin, mag = the grid maximum, input_power = mean |x|^2 over L samples, test_statistics = mag / M^4 / input_power (:422, :480),
 * acq_delay_samples = k* + i* M of the first largest candidate (:471-474), both second_peak fields 0.
 * Two deviations from the block: its candidate accumulators (`complex_acumulator[100]`, :442) are never initialised and are taken
 * as zero; its candidate correlations read past the end of the wiped-off block when f = 1 (k* + N > L), here they stop at L. */
gc_status gc_acq_create_quicksync(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, uint32_t folding_factor, gc_acq** out);
/* d_possible_delay[i] and d_corr_output_f[i], i < folding_factor, of satellite slot `sat` in the last dwell (the values the block logs at
 * :549-552).  Synchronises the context stream: call it behind the fetch of a dwell enqueued on another stream. */
gc_status gc_acq_quicksync_candidates(gc_acq* a, int sat, uint32_t* possible_delay, float* corr_output_f);
/* The adapters' default folding factor, ceil(sqrt(log2(code_length))) (gps_l1_ca_pcps_quicksync_acquisition.cc). */
gc_status gc_quicksync_default_folding_factor(uint32_t code_length, uint32_t* out);
/* The adapters' calculate_threshold: ncells = (code_length / folding_factor) * bins (integer division, bins counted inclusively),
 * lambda = code_length / (double)folding_factor, threshold = -log(1 - pow(1 - pfa, 1 / ncells)) / lambda. */
gc_status gc_quicksync_threshold(float pfa, uint32_t code_length, uint32_t folding_factor, uint32_t doppler_max, uint32_t doppler_step, float* out);
/* Tong engine (pcps_tong_acquisition_cc.cc): the reference's variable-dwell sequential detector.  With N = sampled_ms * samples_per_ms
 * (the transform size: no zero padding, no bit transition; gc_acq_set_local_code takes N complex samples), every dwell adds
 *   grid[b][k] += |IFFT(FFT(x * wipeoff[b]) * conj(FFT(code)))[k]|^2 * s,   s = 1 / (fnf * fnf * P),  fnf = (float)N * (float)N,
 * P = mean |x|^2 of THIS dwell's block, all in float32, the product rounded before it is added (:310-360; the first dwell of a search
 * stores).  Then, per satellite and ON THE DEVICE: d_mag = the largest cell (rows ascending, the first maximum of a row, a later row
 * only with a strictly larger value, nothing wins against 0 or with NaN, :363-375), and the decision (:393-415)
 *   dwell_count++;  if d_mag > threshold * dwell_count (float32): tong_count++, positive when it equals tong_max_val
 *                   else:                                          tong_count--, negative when it reaches 0
 *                   dwell_count >= tong_max_dwells: negative, also over a positive of the same dwell
 * from tong_count = tong_init_val.  A satellite that has decided is FROZEN: later dwells leave its grid, its row maxima
 * (GC_ACQ_PEEK_ROW_MAX), its gc_acq_result and its status as its deciding dwell left them, and their column pass moves no data for it.
 *   Doppler bins    -doppler_max + b doppler_step for every value <= +doppler_max (inclusive: 41 bins for 5000 / 250, :200-205); a
 *                   doppler_step of 0 means 250; num_doppler_bins_override as in gc_acq_create
 *   conf fields     fs_in, sampled_ms, samples_per_ms, samples_per_code, doppler_max, doppler_step, num_doppler_bins_override
 *   GC_ERR_INVALID  unless 1 <= tong_init_val < tong_max_val and tong_max_dwells >= 1; bit_transition_flag or make_2_steps set
 * On such a handle gc_acq_fft_size reports N, N and the inclusive bin count; every dwell call (gc_acq_dwell, _dev, _enqueue, _stream) runs
 * ONE Tong dwell, decision included -- dwells are never held back for one another; gc_acq_reset starts a new search (counters back to
 * their initial values, nothing frozen, the grid reads as zero); gc_acq_get_grid gives the normalised grid; gc_acq_set_step_two,
 * gc_acq_set_frequency_offset and gc_acq_set_local_code_pair return GC_ERR_INVALID.
 * gc_acq_result: mag = test_statistics = d_mag, input_power = P of the dwell, indext / doppler_index / doppler_hz / acq_doppler_hz of
 * d_mag's cell, acq_delay_samples = indext % (uint32_t)samples_per_code (integer, :371), both second_peak fields 0.  A dwell in which no
 * cell wins (P = 0) keeps the cell fields of the dwell before it (zero at the start of a search), as Gnss_Synchro does. */
gc_status gc_acq_create_tong(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, uint32_t tong_init_val, uint32_t tong_max_val, uint32_t tong_max_dwells,
    gc_acq** out);
/* d_threshold: one per engine, used by the decisions of the dwells enqueued after the call.  Default +inf: every dwell counts down. */
gc_status gc_acq_tong_set_threshold(gc_acq* a, float threshold);
enum { GC_ACQ_TONG_RUNNING = 0, GC_ACQ_TONG_POSITIVE = 1, GC_ACQ_TONG_NEGATIVE = 2 };
/* Per satellite (the struct tag shares its name with the call below: write `struct gc_acq_tong_status`). */
struct gc_acq_tong_status
{
    int32_t state;        /* GC_ACQ_TONG_RUNNING / _POSITIVE / _NEGATIVE */
    uint32_t tong_count;  /* d_tong_count */
    uint32_t dwell_count; /* the dwell that decided, or the last dwell run */
};
/* The status of all n_sats satellites (synchronises the context stream). */
gc_status gc_acq_tong_status(gc_acq* a, struct gc_acq_tong_status* out /* n_sats */);
/* Enqueues min(max_new_dwells, tong_max_dwells - dwells so far in this search) dwells on consecutive blocks of N samples of the ring,
 * the first at absolute sample first_index, back to back on the context stream: no host decision and no synchronisation between
 * them, one fetch of results (n_sats) and status (n_sats, may be NULL) at the end.  A second call continues the search where the
 * first stopped.  A ring that does not hold all those samples is refused like gc_acq_dwell_stream refuses its block, before
 * anything is enqueued. */
gc_status gc_acq_tong_search_stream(gc_acq* a, gc_stream* ring, uint64_t first_index, uint32_t max_new_dwells, gc_acq_result* host_results,
    struct gc_acq_tong_status* host_status);
/* The Tong adapters' calculate_threshold in closed form: ncells = vector_length * bins (bins counted inclusively), lambda = vector_length,
 * threshold = quantile(Exp(lambda), (1 - pfa)^(1 / ncells)) = -log(1 - (1 - pfa)^(1 / ncells)) / lambda. */
gc_status gc_tong_threshold(float pfa, uint32_t vector_length, uint32_t doppler_max, uint32_t doppler_step, float* out);
/* CAF engine (galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc): the reference's E5a acquisition for 1 to 3 ms of coherent integration.
 * N = sampled_ms * samples_per_ms is transform size and block length (no bit-transition padding, no second step); every dwell stands
 * alone, overwrites the grid and is never held back.  A slot holds R = (1 + both_components) * hypotheses replicas in the order
 * IA, QA, IB, QB, where B is A with its first code period [0, (uint32_t)samples_per_code) negated (:258-280).
 * Per dwell: P = mean |x|^2; fnf4 = fnf * fnf, fnf = (float)N * (float)N.  Per Doppler bin b and replica X, with the plane
 * X = |IFFT(FFT(x * wipeoff[b]) * conj(FFT(X)))|^2: (kX, mX) = its first maximum, nX = mX / fnf4 (float32).  I takes A when
 * hypotheses == 1 or nIA >= nIB, else B; Q likewise with nQA >= nQB (:533, :543).  CAF_I[b] / CAF_Q[b] = the raw maximum of the chosen
 * I / Q plane; grid row b = chosen I plane (+ chosen Q plane, float32, I first), (k_b, m_b) its first maximum.
 * Per dwell: d_mag = the largest m_b / fnf4, bins ascending, a later bin only with a strictly larger value, nothing wins against 0 or
 * with NaN (:635).  The device keeps ONE statistic per satellite (gc_acq_reset zeroes it): with bit_transition_flag off, or when
 * kept < d_mag / P, the kept statistic := d_mag / P and indext, doppler_index, doppler_hz, acq_doppler_hz and acq_delay_samples =
 * indext % (uint32_t)samples_per_code follow d_mag's cell; otherwise they stay those of the earlier dwell (:645-653).  The block makes
 * that test at every running maximum of the bin walk; d_mag / P is monotone in d_mag, so testing the final maximum is the same.
 * A dwell in which no cell wins (an all-zero block: P = 0, every plane 0) changes neither the kept statistic nor the cell fields:
 * the statistic is then the one of the dwell before (0 after a reset), never 0 / 0.
 * CAF filter (caf_window_hz > 0, :685-770): H = caf_window_hz / (2 * doppler_step) (integer), CAF[d] = the triangular-weighted mean
 * of CAF_I around d plus that of CAF_Q, float32 running sums in index order with the block's three denominators
 * (csrc/acq_caf_filter.h); the first maximum of CAF overwrites doppler_index, doppler_hz and acq_doppler_hz in EVERY dwell, whatever
 * the keep rule said (:768-770).
 * `arithmetic` chooses between the block as written and the block as meant; the two differ in two places:
 *   GC_CAF_REFERENCE  (default, 0) nQB = IB[kQB] / fnf4 -- :523 reads d_magnitudeIB at QB's index -- and the filter weight is
 *                     1 - wf * (float)(unsigned)(d - i) in the I sums of the head (d < H) and middle sections and in the Q sum of the
 *                     middle section, where the block has no abs(): for i > d the difference wraps to 2^32 - (i - d)
 *   GC_CAF_EXACT      nQB = QB[kQB] / fnf4, weight 1 - wf * |d - i| everywhere
 * CAF_Q[b] is the chosen Q plane's own maximum in both (:560).  REFERENCE is the default because a receiver configured for the
 * reference block is expected to report what that block reports.
 *   Doppler bins    -doppler_max + b doppler_step for every value <= +doppler_max (inclusive, :300-307); at most 4096 bins
 *   conf fields     fs_in, sampled_ms, samples_per_ms, samples_per_code, doppler_max, doppler_step, max_dwells, bit_transition_flag
 *   GC_ERR_INVALID  hypotheses outside {1, 2}; both_components outside {0, 1}; unknown arithmetic; doppler_step == 0 (the block has no
 *                   default); bit_transition_flag with max_dwells < 1; make_2_steps; caf_window_hz > 0 with H == 0 or fewer than
 *                   2 H + 1 bins (the block reads out of range or divides by zero there); more than 4096 bins
 * On such a handle gc_acq_fft_size reports N, N and the inclusive bin count; gc_acq_set_local_code_iq sets a slot; every dwell call
 * (gc_acq_dwell, _dev, _enqueue / _flush / _fetch_results, _stream) and both integer input formats work; gc_acq_get_grid and
 * GC_ACQ_PEEK_ROW_MAX read the grid rows; GC_ACQ_PEEK_CODE takes index = R * satellite slot + replica; gc_acq_set_local_code,
 * gc_acq_set_local_code_pair, gc_acq_set_step_two and gc_acq_set_frequency_offset return GC_ERR_INVALID.
 * gc_acq_result: mag = d_mag of this dwell, input_power = P, test_statistics = the kept statistic, both second_peak fields 0.
 * The decision state machine (max_dwells dwells, then kept statistic > threshold) lives with the caller
 * (adapter/hip_e5a_noncoherent_iq_acquisition_caf.h); its threshold is gc_tong_threshold(pfa, N, doppler_max, doppler_step). */
enum { GC_CAF_REFERENCE = 0, GC_CAF_EXACT = 1 };
gc_status gc_acq_create_caf(gc_ctx* ctx, const gc_acq_conf* conf, int n_sats, int both_components, int hypotheses, uint32_t caf_window_hz,
    int arithmetic, gc_acq** out);
/* set_local_code (:234-282) of slot `sat`: N complex samples each; the library derives the B replicas.  code_q may be NULL only
 * without both_components (it is ignored then).  Zero padding is the caller's: a code with zeros behind it and hypotheses = 1.
 * CAF engines only: GC_ERR_INVALID on any other handle. */
gc_status gc_acq_set_local_code_iq(gc_acq* a, int sat, const float* code_i, const float* code_q);
/* CAF, CAF_I, CAF_Q (num_doppler_bins floats each) and the choice bytes (bit 0: I took B, bit 1: Q took B) of slot `sat` in the last
 * dwell; each output may be NULL.  `caf` reads as zeros when the filter is off, everything as zeros before the first dwell of a search.
 * Synchronises the context stream: call it behind the fetch of a dwell enqueued on another stream. */
gc_status gc_acq_caf_vectors(gc_acq* a, int sat, float* caf, float* caf_i, float* caf_q, uint8_t* choice);
/* Inspection of the engine's device-resident intermediates (tests, failure dumps; synchronises the context stream; natural element
 * order whatever the layout in HBM).  `what`:
 *   GC_ACQ_PEEK_WIPEOFF   index = Doppler bin: the wipe-off row exp(-j phase) of the ACTIVE grid, d_grid_doppler_wipeoffs[bin]
 *                         (pcps_acquisition.cc:296-310), fft_size complex values = 2 * fft_size floats
 *   GC_ACQ_PEEK_SPECTRUM  index = Doppler bin: FFT(x * wipeoff[bin]) of the last dwell's block (of the first block of a dwell
 *                         pair processed together) (:721), 2 * fft_size floats
 *   GC_ACQ_PEEK_CODE      index = satellite slot: conj(FFT(code)) (d_fft_codes, :272-273), 2 * fft_size floats; on a paired engine
 *                         index = 2 * satellite slot + replica (0: A, 1: B)
 *   GC_ACQ_PEEK_ROW_MAX   index = satellite slot: per Doppler bin the maximum of the grid row and its position as the statistics
 *                         kernel sees them (the column pass's block maxima, combined): 2 * num_doppler_bins floats (value, index) */
enum { GC_ACQ_PEEK_WIPEOFF = 0, GC_ACQ_PEEK_SPECTRUM = 1, GC_ACQ_PEEK_CODE = 2, GC_ACQ_PEEK_ROW_MAX = 3 };
gc_status gc_acq_peek(gc_acq* a, int what, int index, float* host_out);

/* ------------------------------------------------------------------------ */
/* Ring decimator: a decimated ring derived ON THE DEVICE from another ring -- */
/* the acquisition resampler.  With GNSS-SDR.use_acquisition_resampler=true    */
/* the reference puts one decimating low-pass FIR (fir_filter_ccf) per signal   */
/* between the conditioner and the acquisition blocks                          */
/* (src/core/receiver/gnss_flowgraph.cc:375-499): GPS L1 C/A is searched at     */
/* about 1 Msps whatever the channels' rate, tracking stays on the full-rate    */
/* stream, and the block scales delay and sample stamp back                    */
/* (pcps_acquisition.cc:756-762).  Here the source is a gc_stream ring in any   */
/* format -- pushed from the host or written by a gc_conditioner -- and         */
/*                                                                            */
/*   y[m] = sum_{k=0}^{T-1} h[k] * x[mD - k]      x[n] = 0 for n < 0            */
/*                                                                            */
/* (plain cast, float32 products and sums in tap order: the conditioner's        */
/* definition with translate_hz = 0, and its bits) is appended to a ring of any  */
/* gc_iq_format: a GC_IQ_I16 / GC_IQ_I8 ring receives y[m] quantised as the       */
/* conditioner's "Integer output rings" section states, by the same code.         */
/* Output m is source sample mD, delayed by the filter's (T - 1) / 2              */
/* source samples.  An output's bits are a function of the source samples alone: */
/* never of the update, the tile or how the source was pushed.                  */
/* ------------------------------------------------------------------------ */
typedef struct gc_ring_decimator gc_ring_decimator;
/* src_ring: a ring of the context in any format, empty or still holding sample 0 (GC_ERR_STATE otherwise).  out_ring: an empty
 * GC_IQ_F32 ring of the same context, or an empty integer ring opened with gc_stream_accept_quantised_output; the decimator is its only producer from here on (gc_stream_push* on it return GC_ERR_STATE).
 * decimation 1..64; taps: n_taps = 1..1024 real float32 (copied).  The decimator keeps a reference on both rings.  The arguments
 * are checked before anything touches a device (GC_ERR_INVALID). */
gc_status gc_ring_decimator_create(gc_ctx* ctx, gc_stream* src_ring, uint32_t decimation, const float* taps, uint32_t n_taps,
    gc_stream* out_ring, gc_ring_decimator** out);
gc_status gc_ring_decimator_destroy(gc_ring_decimator* d);
/* Appends every output the source's samples so far complete: afterwards the output ring's head is ceil(src_head / D).  first_out /
 * n_out (optional): the absolute number of the first new output and their count (0 when none is complete).  Asynchronous on the
 * output ring's copy stream (gc_stream_synchronize waits for it); the launch waits for the newest source push, and no source push
 * evicts what it reads.  GC_ERR_STATE, with nothing changed, when source sample max(0, m0 D - (T - 1)) (m0 = the output head) is no
 * longer resident: the source ran more than its capacity ahead.  More outputs than the output ring holds are appended in order, in
 * several pieces.  One update runs at a time; the call may come from another thread than the source's pushes. */
gc_status gc_ring_decimator_update(gc_ring_decimator* d, uint64_t* first_out, uint64_t* n_out);
/* The source head the newest successful update saw, and the output ring's head (any pointer may be NULL). */
gc_status gc_ring_decimator_info(gc_ring_decimator* d, uint64_t* src_consumed, uint64_t* out_head);
/* gc_conditioner_set_output_scale for the decimator: only before the first gc_ring_decimator_update (GC_ERR_STATE afterwards);
 * GC_ERR_INVALID for a scale that is not finite and positive and for a GC_IQ_F32 output ring. */
gc_status gc_ring_decimator_set_output_scale(gc_ring_decimator* d, float scale);
/* gc_conditioner_output_info for the decimator (any pointer may be NULL; synchronous). */
gc_status gc_ring_decimator_output_info(gc_ring_decimator* d, int32_t* out_format, float* scale, uint64_t* clipped_components);
/* The reference's rule for the acquisition resampler of a signal whose optimal search rate is opt_acq_fs_hz
 * (GPS_L1_CA_OPT_ACQ_FS_HZ = 1 000 000 ...), restated on the host:
 *   decimation   = floor(fs_in / opt), stepped down while fs_in % decimation != 0
 *   resampled_fs = fs_in / decimation
 *   taps         = gc_fir_low_pass(1.0, fs_in, resampled_fs / 2.1, resampled_fs / 10)
 *   latency      = (T - 1) / 2          source samples: set_resampler_latency
 * plus ONE rule of this library: the stepping down goes on to the next divisor of fs_in while decimation > 64 or T > 1024 (the
 * kernel's limits; T is about 24.1 x decimation, so in effect decimation <= 42).  opt >= fs_in, or a decimation that ends at 1, gives
 * decimation = 1, resampled_fs = fs_in, n_taps = 0, latency = 0: the reference's "Disabled acquisition resampler because the input
 * sampling frequency is too low".  taps may be NULL to ask for the sizes alone (any other pointer may be NULL too);
 * GC_ERR_INVALID when T > capacity. */
gc_status gc_acq_resampler_plan(int64_t fs_in, uint32_t opt_acq_fs_hz, uint32_t* decimation, int64_t* resampled_fs, float* taps,
    int capacity, int* n_taps, uint32_t* latency_samples);

/* ------------------------------------------------------------------------ */
/* Ring resampler: a ring derived ON THE DEVICE from another ring at an        */
/* ARBITRARY rate ratio -- the third stage of the reference's signal           */
/* conditioner (data_type_adapter -> input_filter -> resampler,                */
/* Resampler.implementation=Direct_Resampler with sample_freq_in /             */
/* sample_freq_out).  The source is a gc_stream ring in any format -- pushed   */
/* from the host, or written by a gc_conditioner or gc_ring_decimator.  Which   */
/* source sample an output is, is a closed form of the output's ABSOLUTE number:*/
/* an output's bits never depend on the update, the tile or how the source was */
/* pushed.  With M = 2^32:                                                     */
/*                                                                            */
/* GC_RESAMP_DIRECT: the reference's Direct_Resampler, nearest earlier sample,  */
/* no filter (direct_resampler_conditioner_{cc,cs,cb}.cc); out[m] = x[n_m],     */
/* bits as they are:                                                           */
/*   fs_in > fs_out   step = floor(M fs_out / fs_in) (IEEE double, to uint32)   */
/*                    n_m = ceil(m M / step)                                   */
/*                    outputs for a source head H >= 1: floor((H-1) step / M)+1 */
/*   fs_in < fs_out   step = floor(M fs_in / fs_out)                           */
/*                    n_m = floor((m + 1) step / M)                            */
/*                    outputs for a source head H: ceil(H M / step) - 1        */
/*   fs_in == fs_out  the identity, n_m = m (the reference's cast of 2^32 to    */
/*                    uint32 is undefined; on x86 it copies every sample)      */
/* These are the picks of the reference's running 32-bit phase.  As there, step */
/* is a floor and the realised rate is slightly below fs_out.  The output ring  */
/* must have the source ring's gc_iq_format (nothing is converted or           */
/* quantised: an integer ring needs no gc_stream_accept_quantised_output).     */
/* 1/64 <= fs_in / fs_out <= 64.                                               */
/*                                                                            */
/* GC_RESAMP_POLYPHASE: band-limited, for the role of the reference's           */
/* Mmse_Resampler (whose taps live in GNU Radio): NOT bit compatible with it.   */
/*   INC   = round(fs_in / fs_out * M)   quotient in IEEE double, ties to even  */
/*   pos_m = m INC      n_m = pos_m >> 32                                      */
/*   p_m   = (pos_m & (M - 1)) >> (32 - log2 P)                                */
/*   y[m]  = sum_{k=0}^{T-1} H[p_m][k] x[n_m - k]     x[n] = 0 for n < 0        */
/*   outputs for a source head H: ceil(H M / INC)                              */
/* (plain cast of integer sources, float32: H[p][0] x first, then one fmaf per  */
/* tap in k order).  H: a bank of P phases x T real float32 taps, row p first;  */
/* P a power of two in 1..256, T in 1..1024, P T <= 8192.                      */
/* 1/8 <= fs_in / fs_out <= 64.  The output ring must be GC_IQ_F32: integer     */
/* output through the conditioner's store epilogue is not implemented          */
/* (GC_ERR_INVALID).  The filter's group delay stays in the observables, as     */
/* with every other filter of the library.                                     */
/* ------------------------------------------------------------------------ */
enum { GC_RESAMP_DIRECT = 0, GC_RESAMP_POLYPHASE = 1 };
typedef struct gc_resampler_conf
{
    double fs_in;            /* rate of the source ring */
    double fs_out;           /* rate of the output ring */
    int32_t mode;            /* GC_RESAMP_DIRECT or GC_RESAMP_POLYPHASE */
    uint32_t phases;         /* GC_RESAMP_POLYPHASE: P */
    uint32_t taps_per_phase; /* GC_RESAMP_POLYPHASE: T */
    uint32_t reserved;       /* 0 */
    const float* bank;       /* GC_RESAMP_POLYPHASE: P * T floats, bank[p * T + k] = H[p][k] (copied); ignored in direct mode */
} gc_resampler_conf;
size_t gc_resampler_conf_size(void);
typedef struct gc_ring_resampler gc_ring_resampler;
/* src_ring: a ring of the context in any format, empty or still holding sample 0 (GC_ERR_STATE otherwise).  out_ring: an empty ring
 * of the same context -- of the source's format in direct mode, GC_IQ_F32 in polyphase mode; the resampler is its only producer from
 * here on (gc_stream_push* on it return GC_ERR_STATE) until gc_ring_resampler_destroy.  The resampler keeps a reference on both
 * rings.  The configuration is checked before anything touches a device (GC_ERR_INVALID). */
gc_status gc_ring_resampler_create(gc_ctx* ctx, gc_stream* src_ring, const gc_resampler_conf* conf, gc_stream* out_ring, gc_ring_resampler** out);
gc_status gc_ring_resampler_destroy(gc_ring_resampler* r);
/* Appends every output the source's samples so far complete: afterwards the output ring's head is the count stated above for the
 * source's head.  first_out / n_out (optional): the absolute number of the first new output and their count (0 when none is
 * complete).  Asynchronous on the output ring's copy stream (gc_stream_synchronize waits for it); the launch waits for the newest
 * source push, and no source push evicts what it reads.  GC_ERR_STATE, with nothing changed, when source sample n_{m0} (direct) or
 * max(0, n_{m0} - (T - 1)) (polyphase), m0 = the output head, is no longer resident: the source ran more than its capacity ahead.
 * More outputs than the output ring holds are appended in order, in several pieces.  One update runs at a time; the call may come
 * from another thread than the source's pushes. */
gc_status gc_ring_resampler_update(gc_ring_resampler* r, uint64_t* first_out, uint64_t* n_out);
/* The source head the newest successful update saw, and the output ring's head (any pointer may be NULL). */
gc_status gc_ring_resampler_info(gc_ring_resampler* r, uint64_t* src_consumed, uint64_t* out_head);
/* A bank for GC_RESAMP_POLYPHASE from the library's own low-pass design:
 *   g          = gc_fir_low_pass(gain = P, fs = P fs_in, cutoff = min(fs_in, fs_out) / 2.1, transition = min(fs_in, fs_out) / 10)
 *   T          = ceil(len(g) / P), g padded with zeros to P T
 *   bank[p][k] = g[k P + p]         written as bank[p * T + k]
 * (the two constants are those of gc_acq_resampler_plan).  Every row sums to about 1.  The group delay is that of the prototype at
 * P times the source rate, (len(g) - 1) / (2 P) source samples -- at most (P T - 1) / (2 P); it stays in the observables.  phases: a
 * power of two in 1..256.  bank may be NULL to ask for T alone.  GC_ERR_INVALID when T > 1024 or P T > 8192, and when P T > capacity. */
gc_status gc_resampler_design(double fs_in, double fs_out, uint32_t phases, float* bank, int capacity, int* taps_per_phase);

/* ------------------------------------------------------------------------ */
/* Notch filter ring stage: continuous-wave interference excised ON THE        */
/* DEVICE -- the reference's input filters Notch_Filter and Notch_Filter_Lite   */
/* (src/algorithms/input_filter/gnuradio_blocks/notch_cc.cc, notch_lite_cc.cc,  */
/* adapters .../adapters/notch_filter.cc, notch_filter_lite.cc).  A GC_IQ_F32   */
/* source ring in, a GC_IQ_F32 output ring out, at the same rate: output m is   */
/* source sample m, copied or filtered.  It is a ring of its own and not a pass */
/* inside the conditioner: the filter reads x[n-1] as it was BEFORE filtering,  */
/* so it cannot overwrite its own input the way pulse blanking does.            */
/* ------------------------------------------------------------------------ */
/* The samples are x[n], n the absolute sample number, x[-1] = 0.  Segment s is [sL, (s+1)L).
 *
 * State: n = 0 (uint32), active = false, noise = 0, last = (0,0), z0 = (0,0), cn = 0.  All arithmetic is float32 with contraction
 * off, unless said otherwise.
 *
 *   for s = 0, 1, 2, ...            (a segment is processed only when all L samples are in the source ring)
 *     if n < segments_est and not active:
 *         noise = (float(n) * noise + F[s]) / float(n + 1);   out = x, bit for bit
 *     else:
 *         E = sum over the segment of re^2 + im^2
 *         if E / noise > threshold:
 *             if not active: active = true; last = (0,0); (lite: cn = 0)
 *             filter the segment (below)
 *         else:
 *             if n > segments_reset: n = 0
 *             active = false;   out = x, bit for bit
 *     n = n + 1
 *
 * The filter, GC_NOTCH_FULL, for every sample k of the segment in order:
 *     c = x[k] * conj(x[k-1])
 *     z = c / |c|, (1,0) when |c| = 0     -- the reference's exp(j * atan2(c.im, c.re)) without the trigonometry: the same unit
 *                                            vector to rounding, from one square root and two divisions
 *     b = x[k] - z * x[k-1]
 *     a = (p * z.re, p * z.im)            p = p_c_factor
 *     out[k] = b + a * last
 *     last = out[k]
 * The filter, GC_NOTCH_LITE:
 *     when cn == 0, a new coefficient:  th1 = atan2f of x[sL+1] * conj(x[sL]);  th2 = atan2f of x[sL+L-1] * conj(x[sL+L-2]);
 *                                       z0 = (cosf(th), sinf(th)) with th = (th1 + th2) / 2
 *     then the same recursion with z = z0 for every sample;  then cn = (cn + 1) % segments_coeff
 *     z0 survives a passing segment, as in the reference.
 *
 * out[k] = b + a * last composes, sample after sample, to one affine map (A, B) per segment.  The device carries last from segment
 * to segment through these composites, last' = B + A * last, and computes the outputs of a segment by the recursion above from the
 * last carried INTO it: the last carried on differs from the segment's final output by rounding (it is what gc_ring_notch_state
 * reports), and every bit is a function of the stream alone.
 *
 * The noise floor F[s]:
 *   1. X[k] is the L-point DFT of the segment, summed directly in sample order with twiddles rounded from double: the order is a
 *      function of the segment alone.
 *   2. P[k] = 10 * log10f(|X[k]|^2 + 1e-20f)
 *   3. mean = sum(P) / L  and  cut = mean + 15                       (sums in bin order)
 *   4. kept bins are those with P[k] <= cut
 *   5. GC_NOTCH_FLOOR_REFERENCE:  fl = mean of P over the kept bins;  F = float(pow(10.0, double(fl) / 10.0) / double(float(2L))).
 *      This is the block as written: VOLK's power spectrum with normalisation 1, its spectral noise floor with 15 dB exclusion,
 *      and std::pow.
 *   6. GC_NOTCH_FLOOR_LINEAR:     F = mean of |X[k]|^2 over the same kept bins, divided by float(2L)
 *
 * threshold: the upper pfa quantile of a chi-squared distribution with 2L degrees of freedom (gc_chi2_upper_quantile), rounded to
 * float32, unless the caller supplies one (0: compute it) -- the pulse blanking convention.
 *
 * Quirks kept from the reference:
 *   Bias.        Averaging decibels biases the REFERENCE floor low by about e^-0.577: for L = 32 and complex Gaussian noise of power
 *                1 it gives noise about 0.25 where pulse blanking's E / float(2L) gives 0.5.  At pfa = 1e-3 (threshold 104.7) it
 *                then flags about 80 % of pure-noise segments (the median E / noise is about 125).  GC_NOTCH_FLOOR_LINEAR is the
 *                unbiased alternative (it flags none of them, and with a tone present exactly the segments the tone covers), after
 *                the precedent of the CAF engine's arithmetic = reference | exact.  The default is the reference's.
 *   Blind spot.  A tone already present while the floor is estimated raises the floor and is never flagged.
 *   Reset.       After a reset n becomes 1, not 0, as in pulse blanking: the re-estimate starts as the mean of the OLD floor and one
 *                new segment.  n wraps where the reference's int32 overflows.
 *
 * Outputs, flags, state and counters are bit-identical however the source was pushed and however the updates were cut, also where
 * the output ring's wrap cuts a segment in two; unflagged segments are copied bit for bit. */
enum { GC_NOTCH_FULL = 0, GC_NOTCH_LITE = 1 };
enum { GC_NOTCH_FLOOR_REFERENCE = 0, GC_NOTCH_FLOOR_LINEAR = 1 };
typedef struct gc_notch_conf
{
    float pfa;               /* false-alarm probability of one segment, 0 < pfa < 1 */
    float threshold;         /* 0: computed from pfa and length; otherwise finite and > 0, used as is */
    float p_c_factor;        /* p, the pole's radius: 0 <= p < 1 */
    uint32_t length;         /* L, samples per segment, 2..1024 (the noise-floor estimate uses a direct DFT) */
    uint32_t segments_est;   /* segments of a noise-floor estimate, >= 1 */
    uint32_t segments_reset; /* a passing segment with n above this starts a new estimate */
    uint32_t segments_coeff; /* GC_NOTCH_LITE: filtered segments per coefficient, >= 1 (also in full mode, where it is unused) */
    int32_t mode;            /* GC_NOTCH_FULL or GC_NOTCH_LITE */
    int32_t noise_floor;     /* GC_NOTCH_FLOOR_REFERENCE or GC_NOTCH_FLOOR_LINEAR */
    uint32_t reserved[3];    /* 0 */
} gc_notch_conf; /* 48 bytes */
size_t gc_notch_conf_size(void);
typedef struct gc_ring_notch gc_ring_notch;
/* src_ring: a GC_IQ_F32 ring of the context, empty or still holding sample 0 (GC_ERR_STATE otherwise), of more than L samples.
 * out_ring: an empty GC_IQ_F32 ring of the same context; the stage is its only producer from here on (gc_stream_push* on it return
 * GC_ERR_STATE) until gc_ring_notch_destroy.  Rings of another format: GC_ERR_INVALID.  The stage keeps a reference on both rings.
 * The configuration is checked before anything touches a device (GC_ERR_INVALID). */
gc_status gc_ring_notch_create(gc_ctx* ctx, gc_stream* src_ring, const gc_notch_conf* conf, gc_stream* out_ring, gc_ring_notch** out);
gc_status gc_ring_notch_destroy(gc_ring_notch* f);
/* Appends every segment the source's samples so far complete: afterwards the output ring's head is floor(source head / L) * L.
 * first_out / n_out (optional): the absolute number of the first new output and their count.  Asynchronous on the output ring's copy
 * stream; the launches wait for the newest source push, and no source push evicts what they read.  GC_ERR_STATE, with nothing
 * changed, when source sample m0 - 1 (m0 = the output head; sample 0 for m0 = 0) is no longer resident.  One update runs at a time. */
gc_status gc_ring_notch_update(gc_ring_notch* f, uint64_t* first_out, uint64_t* n_out);
/* The source head the newest successful update saw, and the output ring's head (any pointer may be NULL). */
gc_status gc_ring_notch_info(gc_ring_notch* f, uint64_t* src_consumed, uint64_t* out_head);
/* Segments decided and filtered so far, the noise floor, n, active, the threshold in use and last as (re, im) in last_re_im[2] (any
 * pointer may be NULL).  Synchronous: waits for the updates so far and copies the state back from the device. */
gc_status gc_ring_notch_state(gc_ring_notch* f, uint64_t* segments_decided, uint64_t* segments_filtered, float* noise_power, uint32_t* n_segments,
    int32_t* active, float* threshold, float* last_re_im);

/* ------------------------------------------------------------------------ */
/* Fine Doppler stage (pcps_acquisition_fine_doppler_cc.cc:400-479): the Doppler */
/* of an acquired satellite to fs / (P Z N) -- 12.5 Hz for a 1 ms code, P = 10,   */
/* Z = 8 -- from the P code periods the ring already holds.  It refines the       */
/* result of any engine above (plain, paired, QuickSync, Tong).                  */
/* ------------------------------------------------------------------------ */
/* With N = samples_per_code, P = prn_replicas, Z = zero_padding_factor, Next = P N Z, x[0 .. P N) the samples from first_index on,
 * s = delay_samples and fc = coarse_doppler_hz the block does
 *   r'           the code rotated by std::rotate(r, r + (N - s), r + N - 1) when s != 0 (:405-409).  The last iterator leaves the final
 *                element in place: r'[i] = code[N - s + i] for i < s - 1, code[i - (s - 1)] for s - 1 <= i < N - 1, code[N - 1] for
 *                i = N - 1.  GC_FINE_ALIGN_REFERENCE is that; GC_FINE_ALIGN_EXACT is r'[i] = code[(i - s) mod N]
 *   y[n]         x[n] r'[n mod N] for n < P N, zero up to Next
 *   p[k]         |sum_n y[n] exp(-j 2 pi k n / Next)|^2, and k* the first largest p[k] in array order
 *   f[k]         float32, from double arithmetic on float32 operands: ((float)fs / 2.0 * (float)k) / ((float)Next / 2.0) for
 *                k < Next / 2, (-(float)fs / 2.0 * (float)(Next - k)) / ((float)Next / 2.0) above
 *   acceptance   |f[k*] - fc| < 1000 in double: Acq_doppler_hz = f[k*], else the coarse value stays
 * Here only the bins that can be accepted are computed, as a direct sum: the window {k : |(double)f[k] - fc| < window_hz}, one
 * circular run (window_first_bin, window_bins) of array indices in ascending frequency (it may cross from index Next - 1 to 0, never
 * Nyquist).  The twiddle phase is always 2 pi ((k n) mod Next) / Next of an integer reduced in 64 bits; products and sums are float32
 * in an order that depends on the request and the samples alone, so a result's bits do not depend on the other requests of a call,
 * on the ring's format or on where the block lies in the ring.
 * DEVIATION: the block looks at the whole spectrum and keeps the coarse value when its maximum lies window_hz or more away; that
 * maximum is never computed here.  The window's maximum is returned with peak, mean (sum |y|^2 = the mean of p over all Next bins, by
 * Parseval: judge the peak against it) and GC_FINE_EDGE when the winner is the window's first or last bin in frequency order, which is
 * what a maximum outside the window looks like from inside. */
enum { GC_FINE_ALIGN_REFERENCE = 0, GC_FINE_ALIGN_EXACT = 1 };
enum { GC_FINE_REFINED = 1, GC_FINE_EDGE = 2 };
typedef struct gc_fine_doppler_conf
{
    int64_t fs_in;
    uint32_t samples_per_code;    /* N */
    uint32_t prn_replicas;        /* P, 1..50 (the block: 10) */
    uint32_t zero_padding_factor; /* Z, 1..16 (the block: 8) */
    float window_hz;              /* the block: 1000 */
    int32_t alignment;            /* GC_FINE_ALIGN_REFERENCE / _EXACT */
} gc_fine_doppler_conf;
typedef struct gc_fine_doppler_request
{
    uint32_t slot;          /* whose code (gc_fine_doppler_set_code) */
    uint32_t delay_samples; /* s < N */
    double coarse_doppler_hz;
} gc_fine_doppler_request;
typedef struct gc_fine_doppler_result
{
    double doppler_hz; /* (double)f[bin], also with GC_FINE_EDGE */
    uint32_t bin;      /* k*, the first largest p[k] of the window in array-index order */
    int32_t status;    /* GC_FINE_REFINED / GC_FINE_EDGE */
    float peak;        /* p[bin] */
    float mean;        /* sum |y[n]|^2 */
    uint32_t window_first_bin, window_bins;
} gc_fine_doppler_result;
typedef struct gc_fine_doppler gc_fine_doppler;
/* GC_ERR_INVALID, before anything touches a device: NULL arguments, n_slots < 1, fs_in < 1, N = 0, P outside 1..50, Z outside 1..16,
 * Next odd or above 2^24 (the table casts k to float), a window that is not finite and positive or reaches fs_in / 2, an unknown
 * alignment, a window of more than 8192 bins. */
gc_status gc_fine_doppler_create(gc_ctx* ctx, const gc_fine_doppler_conf* conf, int n_slots, gc_fine_doppler** out);
gc_status gc_fine_doppler_destroy(gc_fine_doppler* fd);
/* One code period, N complex float32 samples, of satellite slot `slot` (synchronous). */
gc_status gc_fine_doppler_set_code(gc_fine_doppler* fd, int slot, const float* code);
/* Refines n_requests (1 .. n_slots) requests on the P N samples of `ring` from absolute sample first_index on, in one launch, and
 * waits for the results.  A slot may appear in several requests.  The ring must live on the handle's GPU; its format is taken from
 * the ring; the block need only be resident: it may wrap the ring's end and need not fit the ring's max_window.  A read of the ring
 * is reserved before the residency check; a block that is not resident is refused before anything is enqueued (GC_ERR_STATE when
 * its first sample has been evicted, GC_ERR_INVALID when its end has not been pushed yet).
 * GC_ERR_INVALID, before anything touches a device: NULL arguments, n_requests outside 1..n_slots, a slot outside the handle or
 * without a code, delay_samples >= N, |coarse_doppler_hz| + window_hz >= fs_in / 2 or not finite, a window without a bin. */
gc_status gc_fine_doppler_estimate_stream(gc_fine_doppler* fd, gc_stream* ring, uint64_t first_index, const gc_fine_doppler_request* requests,
    int n_requests, gc_fine_doppler_result* results);
/* The same on P N gr_complex samples in host memory. */
gc_status gc_fine_doppler_estimate(gc_fine_doppler* fd, const float* host_iq, const gc_fine_doppler_request* requests, int n_requests,
    gc_fine_doppler_result* results);
/* Inspection: p over the window of request request_index of the last estimate call, window_bins floats in run order. */
gc_status gc_fine_doppler_spectrum(gc_fine_doppler* fd, int request_index, float* host_p);
/* The window rule on the host, no device: the circular run of {k : |(double)f[k] - coarse_hz| < window_hz}.  GC_ERR_INVALID for
 * next odd, 0 or above 2^24, fs_in < 1, |coarse_hz| + window_hz >= fs_in / 2, a window that is not finite and positive. */
gc_status gc_fine_doppler_window(int64_t fs_in, uint32_t next, double coarse_hz, double window_hz, uint32_t* first_bin, uint32_t* bins);
size_t gc_fine_doppler_conf_size(void);

/* ------------------------------------------------------------------------ */
/* Signal generator: a synthetic multi-satellite scene written ON THE DEVICE   */
/* into a ring -- the image of the reference's Signal_Generator source         */
/* (src/algorithms/signal_generator/, block signal_generator_c.cc).  A         */
/* generator is the producer of its ring, as a conditioner is, but has no      */
/* input.  As for every ring stage, a sample's bits are a closed form of its   */
/* ABSOLUTE number and never depend on the call, the tile or the piece of the  */
/* ring it lands in.                                                          */
/*                                                                            */
/* Ring sample i carries scenario sample t = t0 + i (uint64, wraps).  All      */
/* phases are exact integers on Q0.64 fixed point.  For satellite s (its       */
/* index in the configuration, from 0; 1..32 satellites):                      */
/*   code     U = code_phase0_q + t code_step_q   (128 bits, exact)            */
/*            k = U >> 64  the code period,  f = U mod 2^64  the place in it   */
/*            e = (f table_len) >> 64                                          */
/*   component c (1 or 2):  v_c = table_c[e] gain_c sym_c sec_c                */
/*            table_c  one code period, table_len equally spaced float32       */
/*                     entries (1..49104)                                      */
/*            sec_c  = secondary_c[(k + period_offset_c) mod secondary_len_c], */
/*                     +-1, length <= 100; 1 when absent                       */
/*            sym_c  = a random +-1 held for periods_per_symbol_c code periods */
/*                     (0: no data, 1), symbol number                          */
/*                     j = (k + period_offset_c) / periods_per_symbol_c        */
/*            b_s    = sum_c (axis_c ? j v_c : v_c)                            */
/*   carrier  theta = (carr_phase0_q + t carr_step_q) mod 2^64, in turns;      */
/*            w_s = exp(j 2 pi theta / 2^64), evaluated from the signed upper  */
/*            32 bits of theta rounded to float32                              */
/*   sample   x[i] = sum_s amplitude_s b_s w_s + sigma (g_re + j g_im)         */
/*            float32, satellites in index order, noise last                   */
/*   random   Philox4x32-10, key (seed_lo, seed_hi).  Noise of sample t:       */
/*            counter (t_lo, t_hi, 0, 0) -> x0..x3,                            */
/*            u1 = ((x0 >> 8) + 1) 2^-24, u2 = (x1 >> 8) 2^-24,                */
/*            r = sqrt(-2 ln u1), (g_re, g_im) = r (cos 2 pi u2, sin 2 pi u2). */
/*            Symbol j of component c of satellite s: counter                  */
/*            (j_lo, j_hi, 2 s + c, 1); +1 when x0 & 1 == 0, else -1.          */
/* The doubles of gc_siggen_sat become Q0.64 words by ONE rule, floor(x 2^64)  */
/* of x in [0, 1), exact for a double:                                         */
/*   code_step_q   = floor(code_periods_per_sample 2^64)                       */
/*   code_phase0_q = floor(code_phase0_periods 2^64)                           */
/*   carr_step_q   = floor(frac(doppler_hz / fs_hz) 2^64)   quotient in IEEE   */
/*                   double, frac(q) = q - floor(q) (1 becomes 0): a negative   */
/*                   frequency is the two's complement step                    */
/*   carr_phase0_q = floor(frac(carrier_phase0_turns) 2^64)                    */
/* gc_signal_generator_plan returns them without a device.                     */
/*                                                                            */
/* The output ring: an empty GC_IQ_F32 ring, or an empty integer ring opened    */
/* with gc_stream_accept_quantised_output, which receives the conditioner's     */
/* quantisation of the same float32 samples ("Integer output rings" above).    */
/*                                                                            */
/* NOT mirrored from the reference block: its unseeded                         */
/* std::default_random_engine (noise and data bits here are functions of       */
/* `seed`), and the PRN / PRN - 1 index slip of its E5a initialisation         */
/* (signal_generator_c.cc:111 against :399).                                   */
/* ------------------------------------------------------------------------ */
#define GC_SIGGEN_MAX_SATS 32
#define GC_SIGGEN_MAX_TABLE 49104 /* 4092 chips x 12: one period of E1 CBOC */
#define GC_SIGGEN_MAX_SECONDARY 100
enum { GC_SIGGEN_TABLES_AUTO = 0, GC_SIGGEN_TABLES_HBM = 1, GC_SIGGEN_TABLES_LDS = 2 };
typedef struct gc_siggen_component
{
    const float* table;          /* table_len floats (copied at create) */
    const int8_t* secondary;     /* secondary_len values +-1 (copied), or NULL */
    uint32_t secondary_len;      /* 0..100 */
    uint32_t periods_per_symbol; /* 0: no data */
    uint32_t period_offset;
    int32_t axis;                /* 0: real part, 1: imaginary part */
    float gain;
    uint32_t reserved;           /* 0 */
} gc_siggen_component;
typedef struct gc_siggen_sat
{
    double doppler_hz;              /* carrier frequency in the stream, any sign */
    double carrier_phase0_turns;
    double code_phase0_periods;     /* in [0, 1) */
    double code_periods_per_sample; /* in (0, 1) */
    double amplitude;
    uint32_t table_len;             /* entries per code period, both components */
    uint32_t n_components;          /* 1 or 2 */
    gc_siggen_component comp[2];
} gc_siggen_sat;
typedef struct gc_siggen_conf
{
    double fs_hz;
    double noise_sigma;       /* per part; 0: no noise */
    uint64_t seed;
    uint64_t t0;              /* scenario sample of ring sample 0 */
    uint32_t n_sats;          /* 1..32 */
    uint32_t table_placement; /* GC_SIGGEN_TABLES_AUTO, or one placement forced (_LDS: GC_ERR_INVALID when the tables do not fit) */
    const gc_siggen_sat* sats;
} gc_siggen_conf;
size_t gc_siggen_component_size(void);
size_t gc_siggen_sat_size(void);
size_t gc_siggen_conf_size(void);
typedef struct gc_signal_generator gc_signal_generator;
/* out_ring: an empty ring of the context (see above); the generator is its only producer from here on (gc_stream_push* on it
 * return GC_ERR_STATE) until gc_signal_generator_destroy, and keeps a reference on it.  Every argument is checked before anything
 * touches a device (GC_ERR_INVALID); tables and secondary codes are copied. */
gc_status gc_signal_generator_create(gc_ctx* ctx, const gc_siggen_conf* conf, gc_stream* out_ring, gc_signal_generator** out);
gc_status gc_signal_generator_destroy(gc_signal_generator* g);
/* Appends n_samples samples; first_index (optional): the absolute number of the first of them.  Asynchronous on the ring's copy
 * stream (gc_stream_synchronize waits for it); waits, like every producer, for launches that still read what it evicts.  More
 * samples than the ring holds are appended in order, in several pieces.  One call runs at a time. */
gc_status gc_signal_generator_generate(gc_signal_generator* g, uint64_t n_samples, uint64_t* first_index);
/* The ring's head: samples generated so far. */
gc_status gc_signal_generator_info(gc_signal_generator* g, uint64_t* head);
/* gc_conditioner_set_output_scale / gc_conditioner_output_info for the generator: the scale only before the first
 * gc_signal_generator_generate (GC_ERR_STATE afterwards), GC_ERR_INVALID for a scale that is not finite and positive and for a
 * GC_IQ_F32 ring. */
gc_status gc_signal_generator_set_output_scale(gc_signal_generator* g, float scale);
gc_status gc_signal_generator_output_info(gc_signal_generator* g, int32_t* out_format, float* scale, uint64_t* clipped_components);
/* The four Q0.64 words of one satellite by the rule above, on the host, no device (any pointer may be NULL). */
gc_status gc_signal_generator_plan(const gc_siggen_sat* sat, double fs_hz, uint64_t* code_step_q, uint64_t* code_phase0_q, uint64_t* carr_step_q,
    uint64_t* carr_phase0_q);
/* One satellite of the reference block's configuration (SignalSource.system_i, .signal_i, .PRN_i, .CN0_dB_i, .doppler_Hz_i,
 * .delay_chips_i, .delay_sec_i, .fs_hz, .BW_BB, .data_flag, .noise_flag) as a gc_siggen_sat, with the code generators above:
 *   "G" "1C"  one BPSK component of 1023 entries, N = round(fs / 1 kHz), code step 1 / N, 20 periods per symbol with data_flag;
 *             the noise-free sequence is gc_gps_l1_ca_code_gen_complex_sampled(prn, fs, 1023 - delay_chips), repeated
 *   "R" "1G"  the same with the 511-chip code; carrier = intermediate_freq_hz + 562.5 kHz x channel(prn) + doppler (the block
 *             hard-codes 4 MHz and says "must be set by the user")
 *   "E" "1B"  component 0: E1-B CBOC, 12 entries per chip, gain +1, one period per symbol; component 1: E1-C CBOC, gain -1, the
 *             25-chip secondary code, no data
 *   "E" "5X"  component 0: the I code, real axis, the 20-chip secondary code, 20 periods per symbol; component 1: the Q code,
 *             imaginary axis, the PRN's 100-chip secondary code; period_offset = delay_sec for both
 * amplitude = sqrt(10^(CN0 / 10) / (BW_BB fs / 2)), with a further 1 / sqrt(2) for Galileo; 1 when noise_flag is 0 (*noise_sigma:
 * 1 or 0).  code_phase0 lies one sample less 2^-16 behind the start of the (delayed) period, so that the floor of the table index
 * is the samplers' ceil((i + 1) L / N) - 1, evaluated exactly.  For G / R at 2.048, 4 and 6.625 Msps that is the sampled generator
 * sample for sample; where a sampler's float32 quotient lands an entry off (one sample per period at 25 Msps, isolated samples of the
 * CBOC tables) the generator keeps the formula.  Data symbols change at the satellite's own code-period boundary.
 * tables / secondaries: caller memory for 2 x table_capacity floats and 2 x 100 int8 that sat->comp[] will point into; they must
 * outlive gc_signal_generator_create.  table_capacity >= the signal's table length (GC_SIGGEN_MAX_TABLE always suffices). */
gc_status gc_siggen_reference_satellite(const char* system, const char* signal, uint32_t prn, double cn0_db, double doppler_hz, uint32_t delay_chips,
    uint32_t delay_sec, double fs_hz, double bw_bb, int data_flag, int noise_flag, double intermediate_freq_hz, gc_siggen_sat* sat, float* tables,
    uint32_t table_capacity, int8_t* secondaries, double* noise_sigma);

#define GC_ABI_CHECK() \
    gc_abi_check(sizeof(gc_epoch_params), sizeof(gc_loop_conf), sizeof(gc_loop_record), sizeof(gc_loop_sync_conf), sizeof(gc_acq_conf), sizeof(gc_acq_result))

#ifdef __cplusplus
}
#endif
#endif /* GNSSCORR_H */
