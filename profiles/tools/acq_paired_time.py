#!/usr/bin/env python3
"""Times one two-replica search both ways on the same box in the same call: 16 Galileo E1 satellites x 41 Doppler bins at N = 16000
(4 Msps, 4 ms), CCCWSR replicas (cd - j cp, cd + j cp) of every PRN, MAX combining, one CFAR dwell per search --

  paired  a paired engine (gc_acq_create_paired): 16 slots of two replicas, one combined grid per satellite
  split   what a one-replica engine offers: 32 slots holding the same 32 replicas, two grids per satellite (the host would still have
          to combine them; that is not timed)

    python3 profiles/tools/acq_paired_time.py [--warm 5] [--reps 20] [--out profiles/paired_acq_latest.json]

HIP events around --reps searches behind --warm warm-up searches.  Prints one JSON line (and writes it to --out): ms per search of
both forms, their ratio, and whether the paired result equals the larger of the split pair's."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sats", type=int, default=16)
    ap.add_argument("--bins", type=int, default=41)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3, help="alternating timed rounds of each form; the median is reported")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import gnsscorr
    fs, n = 4_000_000, 16000
    dev = torch.device("cuda", 0)
    ctx = gnsscorr.Context(0)
    conf = dict(fs_in=fs, sampled_ms=4, ms_per_code=4, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=16000.0, samples_per_chip=4,
        doppler_max=5000, doppler_step=250, max_dwells=1, use_cfar=True, num_doppler_bins_override=args.bins)
    paired = gnsscorr.PcpsAcquisition(ctx, args.sats, combine="max", **conf)
    split = gnsscorr.PcpsAcquisition(ctx, 2 * args.sats, **conf)
    for s in range(args.sats):
        cd = gnsscorr.galileo_e1_code_gen_complex_sampled("1B", False, s + 1, fs)
        cp = gnsscorr.galileo_e1_code_gen_complex_sampled("1C", False, s + 1, fs)
        a, b = gnsscorr.cccwsr_replicas(cd, cp)
        paired.set_local_code_pair(s, a, b)
        split.set_local_code(2 * s, a)
        split.set_local_code(2 * s + 1, b)
    x = np.fromfile(os.path.join(ROOT, "tests", "golden", "kat_galileo_e1_id1_fs4msps_8ms.dat"), np.complex64)[:n]  # PRN 1
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

    t_paired, t_split = [], []
    for _ in range(args.rounds):
        t_paired.append(timed(paired))
        t_split.append(timed(split))
    rp, rs = paired.fetch_results(stream), split.fetch_results(stream)
    same = all(rp[s].mag == max(rs[2 * s].mag, rs[2 * s + 1].mag) for s in range(args.sats))
    found = int(np.argmax([r.test_statistics for r in rp])) == 0
    out = {"shape": "%d sats x %d bins, N = %d, MAX, 1 dwell" % (args.sats, args.bins, n), "warm": args.warm, "reps": args.reps,
        "paired_ms": float(np.median(t_paired)), "split_ms": float(np.median(t_split)), "paired_ms_rounds": t_paired, "split_ms_rounds": t_split,
        "paired_over_split": float(np.median(t_paired) / np.median(t_split)), "paired_equals_larger_of_split": bool(same), "found_prn1": bool(found)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    paired.close()
    split.close()


if __name__ == "__main__":
    main()
