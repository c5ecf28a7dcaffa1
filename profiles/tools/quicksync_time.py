#!/usr/bin/env python3
"""Times the QuickSync search against the plain engine on the same samples, on the same box in the same call.  Per shape (N, f), 32
satellites x 41 Doppler bins, one CFAR dwell per search on L = f N samples of a synthetic GPS-like block:

  quicksync  gc_acq_create_quicksync: fold to M = N / f, transforms of M points, candidate check on the device
  plain      gc_acq_create with sampled_ms = ms_per_code = f: transforms of f N points, the code tiled f times

    python3 profiles/tools/quicksync_time.py [--warm 5] [--reps 50] [--rounds 5] [--out profiles/quicksync_latest.json]
    python3 profiles/tools/quicksync_time.py --shape 2 --reps 10 --rounds 1      one shape only, for a kernel trace:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o qs -- python3 profiles/tools/quicksync_time.py --shape 2 --reps 10 --rounds 1
    python3 profiles/tools/quicksync_time.py --fold-stats DIR0 DIR1 DIR2 --merge profiles/quicksync_latest.json
                                             adds the fold kernel's mean duration of the three traced runs and its achieved bytes / s

Device events around --reps searches behind --warm warm-up searches; the two engines alternate --rounds times and the median round is
reported with the spread (min, max).  The fold kernel's algorithmic bytes per search: per bin 8 f^2 M of wipe-off table read once and
8 M written, plus 8 f^2 M of the block, which every bin shares."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))
import numpy as np

SHAPES = [(4000, 2), (4000, 4), (25000, 4)]


def fold_bytes(N, f, bins):
    M = N // f
    return bins * (8 * f * f * M + 8 * M) + 8 * f * f * M


def time_shape(args, ctx, N, f):
    import torch
    import gnsscorr
    fs, L = N * 1000, f * N
    dev = torch.device("cuda", 0)
    common = dict(fs_in=fs, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=float(N), samples_per_chip=max(1, int(np.ceil(fs / 1.023e6))),
        doppler_max=5000, doppler_step=250, max_dwells=1, use_cfar=True, num_doppler_bins_override=args.bins)
    qs = gnsscorr.PcpsAcquisition(ctx, args.sats, sampled_ms=f, ms_per_code=1, folding_factor=f, **common)
    plain = gnsscorr.PcpsAcquisition(ctx, args.sats, sampled_ms=f, ms_per_code=f, **common)
    assert (qs.fft_size, qs.consumed_samples, qs.num_doppler_bins) == (N // f, L, args.bins)
    assert (plain.fft_size, plain.consumed_samples, plain.num_doppler_bins) == (L, L, args.bins)
    codes = [gnsscorr.gps_l1_ca_code_gen_complex_sampled(s % 32 + 1, fs)[:N] for s in range(args.sats)]
    for s, c in enumerate(codes):
        qs.set_local_code(s, c)
        plain.set_local_code(s, np.tile(c, f))
    # PRN 1 at 47 dB-Hz, delay 1234 samples, on the bin of 1250 Hz; unit-variance noise
    rng = np.random.Generator(np.random.PCG64(11))
    n = np.arange(L)
    x = (np.sqrt(10.0 ** 4.7 / fs) * np.roll(np.tile(codes[0], f), 1234) * np.exp(2j * np.pi * 1250.0 * n / fs)
        + (rng.standard_normal(L) + 1j * rng.standard_normal(L)) * np.sqrt(0.5)).astype(np.complex64)
    d_x = torch.from_numpy(x.view(np.float32).copy()).to(dev)
    tstream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    torch.cuda.synchronize()

    def search(acq):
        acq.reset()
        acq.dwell_enqueue(d_x.data_ptr(), stream)
        acq.flush(stream)

    def timed(acq):
        for _ in range(args.warm):
            search(acq)
        torch.cuda.synchronize()
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for _ in range(args.reps):
            search(acq)
        a1.record()
        torch.cuda.synchronize()
        return float(a0.elapsed_time(a1)) / args.reps

    t_qs, t_plain = [], []
    for _ in range(args.rounds):
        t_qs.append(timed(qs))
        t_plain.append(timed(plain))
    rq, rp = qs.fetch_results(stream)[0], plain.fetch_results(stream)[0]
    out = {"N": N, "f": f, "M": N // f, "L": L, "sats": args.sats, "bins": args.bins,
        "quicksync_ms": float(np.median(t_qs)), "quicksync_ms_min_max": [min(t_qs), max(t_qs)],
        "plain_ms": float(np.median(t_plain)), "plain_ms_min_max": [min(t_plain), max(t_plain)],
        "plain_over_quicksync": float(np.median(t_plain) / np.median(t_qs)),
        "quicksync_faster_in_every_round": bool(max(t_qs) < min(t_plain)),
        "quicksync_delay_doppler": [rq.acq_delay_samples, rq.doppler_hz], "plain_delay_doppler": [rp.acq_delay_samples % N, rp.doppler_hz],
        "fold_algorithmic_bytes": fold_bytes(N, f, args.bins)}
    qs.close()
    plain.close()
    return out


def fold_stats(dirs, merge):
    doc = json.load(open(merge))
    for d, shape in zip(dirs, doc["shapes"]):
        path = None
        for root, _, files in os.walk(d):
            for fn in sorted(files):
                if fn.endswith("kernel_stats.csv"):
                    path = os.path.join(root, fn)
        for r in csv.DictReader(open(path)):
            if "acq_qs_fold_kernel" in r["Name"]:
                shape["fold_kernel_us"] = float(r["AverageNs"]) / 1e3
                shape["fold_kernel_calls"] = int(r["Calls"])
                shape["fold_achieved_GBps"] = shape["fold_algorithmic_bytes"] / float(r["AverageNs"])
            if "acq_qs_verify_kernel" in r["Name"]:
                shape["verify_kernel_us"] = float(r["AverageNs"]) / 1e3
    with open(merge, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sats", type=int, default=32)
    ap.add_argument("--bins", type=int, default=41)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5, help="alternating timed rounds of each engine; the median is reported")
    ap.add_argument("--shape", type=int, default=-1, help="index into the shape list (default: all)")
    ap.add_argument("--out", default="")
    ap.add_argument("--fold-stats", nargs="*", default=None, help="rocprofv3 output directories of --shape 0, 1, 2 runs")
    ap.add_argument("--merge", default="")
    args = ap.parse_args()
    if args.fold_stats is not None:
        return fold_stats(args.fold_stats, args.merge)
    import gnsscorr
    ctx = gnsscorr.Context(0)
    shapes = SHAPES if args.shape < 0 else [SHAPES[args.shape]]
    out = {"command": "python3 profiles/tools/quicksync_time.py --warm %d --reps %d --rounds %d" % (args.warm, args.reps, args.rounds),
        "shapes": [time_shape(args, ctx, N, f) for N, f in shapes]}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
