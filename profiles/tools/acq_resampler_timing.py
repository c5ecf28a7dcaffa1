"""Cost and gain of the acquisition resampler on one MI355X ("Ring decimator"):

(a) one synchronised RingDecimator.update() after a 16 ms push of a 25 Msps cshort stream (400 000 samples -> 16 000 outputs;
    D = 25, T = 603: gc_acq_resampler_plan(25e6, 1e6)).  The push itself is synchronised before the clock starts.
(b) a 32-PRN, 41-bin, 2-dwell GPS L1 C/A search on the 25 Msps ring (N = 25 000) against the same search on the derived 1 Msps ring
    (N = 1000), through the synchronous gc_acq_dwell_stream (one call per dwell), both in the same process, the legs alternating.

Host clock; warm-up in front of every timed window; every round is printed, so the spread is visible.

python profiles/tools/acq_resampler_timing.py [--reps 30] [--rounds 5] [--design DESIGN.md]

The figures recorded in DESIGN.md come from the defaults."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))

FS_IN, OPT = 25_000_000, 1_000_000
BLOCK = 400_000  # 16 ms at 25 Msps
N_SATS, DOPPLER_MAX, DOPPLER_STEP, N_BINS, DWELLS = 32, 5000, 250, 41, 2
BEGIN, END = "<!-- acq_resampler_timing:begin -->", "<!-- acq_resampler_timing:end -->"


def timed(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", help="also write the JSON here")
    ap.add_argument("--design", help="DESIGN.md to update between the acq_resampler_timing markers")
    args = ap.parse_args()
    import torch
    import gnsscorr
    ctx = gnsscorr.Context(0)  # no GPU: this raises; a timing without the device means nothing
    D, rfs, taps, latency = gnsscorr.acq_resampler_plan(FS_IN, OPT)
    assert (D, rfs, len(taps)) == (25, 1_000_000, 603)
    rng = np.random.Generator(np.random.PCG64(1))
    raw = np.clip(np.round(rng.standard_normal((BLOCK, 2)) * 45.0), -32767, 32767).astype(np.int16)
    pinned = torch.from_numpy(raw.copy()).pin_memory()
    src = gnsscorr.IqStream(ctx, 8 * BLOCK, 25_000, gnsscorr.GC_IQ_I16)
    out = gnsscorr.IqStream(ctx, 8 * BLOCK // D, 1000, gnsscorr.GC_IQ_F32)
    dec = gnsscorr.RingDecimator(ctx, src, D, taps, out)

    def push_update():
        src.push_pinned(pinned.data_ptr(), BLOCK)
        src.synchronize()
        t0 = time.perf_counter()
        dec.update()
        out.synchronize()
        return time.perf_counter() - t0

    for _ in range(10):
        push_update()
    update_us = [round(float(np.mean([push_update() for _ in range(args.reps)])) * 1e6, 2) for _ in range(args.rounds)]

    # (b): both engines search what the rings hold now
    def engine(fs, ring_format):
        n = fs // 1000
        a = gnsscorr.PcpsAcquisition(ctx, N_SATS, fs, 1, 1, np.float32(fs) * np.float32(0.001), float(n), max(1, -(-fs // 1_023_000)), DOPPLER_MAX,
            DOPPLER_STEP, max_dwells=DWELLS, num_doppler_bins_override=N_BINS)
        a.set_input_format(ring_format)
        for s in range(N_SATS):
            a.set_local_code(s, gnsscorr.gps_l1_ca_code_gen_complex_sampled(s + 1, fs))
        return a

    full, res = engine(FS_IN, gnsscorr.GC_IQ_I16), engine(rfs, gnsscorr.GC_IQ_F32)
    assert (full.fft_size, res.fft_size, full.num_doppler_bins, res.num_doppler_bins) == (25_000, 1000, N_BINS, N_BINS)
    _, head_src, _ = src.info()
    _, head_out, _ = out.info()

    def search(a, ring, first):
        a.reset()
        for k in range(DWELLS):
            r = a.dwell_stream(ring, first + k * a.consumed_samples)
        return r

    legs = {"full_rate_25Msps": lambda: search(full, src, head_src - BLOCK), "derived_1Msps": lambda: search(res, out, head_out - BLOCK // D)}
    for fn in legs.values():
        timed(fn, 5)
    rounds = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name, fn in legs.items():
            rounds[name].append(round(timed(fn, args.reps), 2))
    for h in (full, res, dec, out, src):
        h.close()
    ctx.close()
    med = {name: float(np.median(v)) for name, v in rounds.items()}
    result = {"fs_in": FS_IN, "decimation": D, "taps": len(taps), "block_samples": BLOCK, "outputs_per_block": BLOCK // D, "reps": args.reps,
        "update_us": update_us, "update_median_us": float(np.median(update_us)),
        "search": {"sats": N_SATS, "bins": N_BINS, "dwells": DWELLS, "rounds_us": rounds, "median_us": med,
            "ratio": med["full_rate_25Msps"] / med["derived_1Msps"]}}
    txt = json.dumps(result)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    if args.design:
        lines = [BEGIN,
            "(a) Synchronised `update()` after a 16 ms push (400 000 cshort samples at 25 Msps -> 16 000 outputs, `D = 25`, `T = 603`), median of "
            "%d rounds of %d: **%.1f us** (rounds: %s)." % (args.rounds, args.reps, result["update_median_us"], ", ".join("%.1f" % v for v in update_us)),
            "(b) 32 PRNs x 41 bins x 2 dwells of GPS L1 C/A (`gc_acq_dwell_stream`, synchronous), median of %d rounds of %d searches: on the "
            "25 Msps cshort ring (N = 25 000) **%.1f us** (rounds: %s), on the derived 1 Msps ring (N = 1000) **%.1f us** (rounds: %s): ratio "
            "**%.1f**." % (args.rounds, args.reps, med["full_rate_25Msps"], ", ".join("%.1f" % v for v in rounds["full_rate_25Msps"]),
                med["derived_1Msps"], ", ".join("%.1f" % v for v in rounds["derived_1Msps"]), result["search"]["ratio"]),
            END]
        with open(args.design) as f:
            doc = f.read()
        doc, n = re.subn(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: "\n".join(lines), doc, flags=re.S)
        assert n == 1, "DESIGN.md has no acq_resampler_timing markers"
        with open(args.design, "w") as f:
            f.write(doc)


if __name__ == "__main__":
    main()
