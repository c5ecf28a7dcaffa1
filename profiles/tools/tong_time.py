#!/usr/bin/env python3
"""Times a Tong search against the plain engine on the same blocks, on the same box in the same call.  32 satellites x 41 Doppler
bins, N = 25000 (GPS L1 C/A at 25 Msps, 1 ms blocks), eight blocks; half of the satellites are in the signal (47 dB-Hz), half absent:

  tong            gc_acq_create_tong (2, 4, 8): eight dwells enqueued back to back, decided on the device, ONE fetch at the end; the
                  satellites that have decided are frozen and their column passes move nothing
  tong_unfrozen   the same engine with (8, 9, 8) and the default +inf threshold: every satellite counts down for all eight dwells,
                  nothing freezes before the last one -- what the eight dwells cost without the early exits
  plain           gc_acq_create with max_dwells = 8: eight dwells with a fetch and a host decision behind each (what driving a
                  variable-dwell detector from the host takes), every grid rewritten by every dwell

    python3 profiles/tools/tong_time.py [--warm 3] [--reps 10] [--rounds 5] [--out profiles/tong_latest.json]

Device events around --reps searches behind --warm warm-up searches, all work on one stream; the engines alternate --rounds times
and the median round is reported with the spread (min, max).  A ratio is stated only when the two spreads do not overlap."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sats", type=int, default=32)
    ap.add_argument("--bins", type=int, default=41)
    ap.add_argument("--n", type=int, default=25000)
    ap.add_argument("--dwells", type=int, default=8)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import gnsscorr
    ctx = gnsscorr.Context(0)
    N, D = args.n, args.dwells
    fs = N * 1000
    dev = torch.device("cuda", 0)
    common = dict(fs_in=fs, sampled_ms=1, ms_per_code=1, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=float(N),
        samples_per_chip=max(1, int(np.ceil(fs / 1.023e6))), doppler_max=5000, doppler_step=250, num_doppler_bins_override=args.bins)
    tong = gnsscorr.PcpsAcquisition(ctx, args.sats, tong=(2, 4, D), **common)
    unfrozen = gnsscorr.PcpsAcquisition(ctx, args.sats, tong=(D, D + 1, D), **common)
    plain = gnsscorr.PcpsAcquisition(ctx, args.sats, max_dwells=D, use_cfar=False, **common)
    codes = [gnsscorr.gps_l1_ca_code_gen_complex_sampled(s % 32 + 1, fs)[:N] for s in range(args.sats)]
    for s, c in enumerate(codes):
        for e in (tong, unfrozen, plain):
            e.set_local_code(s, c)
    # the even slots' PRNs at 47 dB-Hz on bins of the grid, unit-variance noise
    rng = np.random.Generator(np.random.PCG64(11))
    n = np.arange(D * N)
    x = (rng.standard_normal(D * N) + 1j * rng.standard_normal(D * N)) * np.sqrt(0.5)
    for s in range(0, args.sats, 2):
        x += np.sqrt(10.0 ** 4.7 / fs) * np.roll(np.tile(codes[s], D), 700 * s + 123) * np.exp(2j * np.pi * (250.0 * (s - 16)) * n / fs)
    x = x.astype(np.complex64)
    # noise cells average 1 / N per dwell and the largest of bins * N of them about ln(bins N) = 14 times that; a present satellite adds 2e-3
    threshold = 1.0e-3
    tong.set_threshold(threshold)
    d_x = torch.from_numpy(x.view(np.float32).copy()).to(dev)
    tstream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    torch.cuda.synchronize()

    def search_tong(acq):
        acq.reset()
        for d in range(D):
            acq.dwell_enqueue(d_x.data_ptr() + 8 * N * d, stream)
        return acq.fetch_results(stream)

    decisions = []

    def search_plain(acq):
        acq.reset()
        running = [True] * args.sats
        for d in range(D):
            acq.dwell_enqueue(d_x.data_ptr() + 8 * N * d, stream)
            res = acq.fetch_results(stream)
            # the host's decision of this dwell: a first-to-second-peak test per satellite
            running = [run and not (r.test_statistics > 2.0) for run, r in zip(running, res)]
        decisions.append(sum(running))
        return res

    def timed(fn, acq):
        for _ in range(args.warm):
            fn(acq)
        torch.cuda.synchronize()
        a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a0.record()
        for _ in range(args.reps):
            fn(acq)
        a1.record()
        torch.cuda.synchronize()
        return float(a0.elapsed_time(a1)) / args.reps

    t = {"tong": [], "tong_unfrozen": [], "plain": []}
    for _ in range(args.rounds):
        t["tong"].append(timed(search_tong, tong))
        t["plain"].append(timed(search_plain, plain))
        t["tong_unfrozen"].append(timed(search_tong, unfrozen))
    search_tong(tong)
    status = tong.tong_status()
    out = {"command": "python3 profiles/tools/tong_time.py --warm %d --reps %d --rounds %d" % (args.warm, args.reps, args.rounds),
        "N": N, "sats": args.sats, "bins": args.bins, "dwells": D, "threshold": threshold,
        "tong_states_present": [status[s].state for s in range(0, args.sats, 2)], "tong_deciding_dwell_present": [status[s].dwell_count for s in range(0, args.sats, 2)],
        "tong_states_absent": [status[s].state for s in range(1, args.sats, 2)], "tong_deciding_dwell_absent": [status[s].dwell_count for s in range(1, args.sats, 2)]}
    for k, v in t.items():
        out[k + "_ms"] = float(np.median(v))
        out[k + "_ms_min_max"] = [min(v), max(v)]
    for a, b in (("plain", "tong"), ("tong_unfrozen", "tong")):
        apart = max(t[b]) < min(t[a]) or max(t[a]) < min(t[b])
        out[a + "_over_" + b] = float(np.median(t[a]) / np.median(t[b])) if apart else None
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    for e in (tong, unfrozen, plain):
        e.close()
    ctx.close()


if __name__ == "__main__":
    main()
