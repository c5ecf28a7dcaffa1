#!/usr/bin/env python3
"""Times the E5a I/Q hypothesis search with CAF filter (gc_acq_create_caf) against what the same search takes without it, on the
same box in the same call.  16 satellites x 81 Doppler bins (10000 / 250, both ends), N = 30000 (E5a at 10 Msps, 3 ms), both
components and two hypotheses (R = 4), CAF window 3000 Hz (H = 6):

  caf     one dwell of the CAF engine: four |.|^2 planes per satellite, the per-bin choice, the grid rows, the result and the filter on
          the device; ONE fetch of 16 results
  plain   the same search as 64 slots of a plain engine (gc_acq_create, the replicas IA, QA, IB, QB of every satellite as slots of
          their own): one dwell, the four grids of every satellite fetched, and selection, sum, maximum and filter in numpy

    python3 profiles/tools/caf_time.py [--warm 5] [--reps 20] [--rounds 3] [--only caf|plain] [--out profiles/caf_latest.json]

Device events around --reps searches behind --warm warm-up searches, all work on one stream; the engines alternate --rounds times and
the median round is reported with the spread (min, max).  The share of acq_caf_select_kernel comes from a kernel trace of `--only caf`
(rocprofv3 --kernel-trace --stats -- python3 profiles/tools/caf_time.py --only caf --rounds 1); --select-us takes its mean duration
and the tool states the bytes per second it stands for: per grid row 2 N floats read and N written at R = 4."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sats", type=int, default=16)
    ap.add_argument("--spm", type=int, default=10000)
    ap.add_argument("--ms", type=int, default=3)
    ap.add_argument("--dmax", type=int, default=10000)
    ap.add_argument("--dstep", type=int, default=250)
    ap.add_argument("--window", type=int, default=3000)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["caf", "plain"], default=None)
    ap.add_argument("--select-us", type=float, default=0.0, help="mean duration of acq_caf_select_kernel from a kernel trace")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import gnsscorr
    import caf_ref
    ctx = gnsscorr.Context(0)
    spm, ms, S = args.spm, args.ms, args.sats
    N, fs = spm * ms, 1000 * spm
    bins = caf_ref.doppler_bins(args.dmax, args.dstep)
    H = args.window // (2 * args.dstep)
    dev = torch.device("cuda", 0)
    common = dict(fs_in=fs, sampled_ms=ms, samples_per_ms=np.float32(fs) * np.float32(0.001), samples_per_code=float(spm), samples_per_chip=1, doppler_max=args.dmax,
        doppler_step=args.dstep)
    codes = []
    for s in range(S):
        ci = np.tile(gnsscorr.galileo_e5_a_code_gen_complex_sampled("5I", s + 1, fs)[:spm], ms)
        cq = np.tile(gnsscorr.galileo_e5_a_code_gen_complex_sampled("5Q", s + 1, fs)[:spm], ms)
        codes.append((ci, cq))
    caf = plain = None
    if args.only != "plain":
        caf = gnsscorr.PcpsAcquisition(ctx, S, ms_per_code=1, caf=dict(both_components=1, hypotheses=2, window_hz=args.window, arithmetic="reference"), **common)
        for s, (ci, cq) in enumerate(codes):
            caf.set_local_code_iq(s, ci, cq)
    if args.only != "caf":
        plain = gnsscorr.PcpsAcquisition(ctx, 4 * S, ms_per_code=ms, num_doppler_bins_override=len(bins), **common)
        assert plain.fft_size == N
        for s, (ci, cq) in enumerate(codes):
            for i, rep in enumerate(caf_ref.replicas(ci, cq, 1, 2, spm)):
                plain.set_local_code(4 * s + i, rep)
    # the even slots' PRNs on bins of the grid, first code period sign-flipped for every other one of them, unit-variance noise
    rng = np.random.Generator(np.random.PCG64(11))
    n = np.arange(N)
    x = (rng.standard_normal(N) + 1j * rng.standard_normal(N)) * np.sqrt(0.5)
    for s in range(0, S, 2):
        sign = np.where((n // spm == 0) & (s % 4 == 0), -1.0, 1.0)
        x += 0.1 * np.roll(sign * (codes[s][0] + codes[s][1]), 700 * s + 123) * np.exp(2j * np.pi * (250.0 * (s - 8)) * n / fs)
    x = x.astype(np.complex64)
    d_x = torch.from_numpy(x.view(np.float32).copy()).to(dev)
    tstream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    torch.cuda.synchronize()
    fnf4 = (np.float32(N) * np.float32(N)) ** 2
    found = {}

    def search_caf(acq):
        acq.reset()
        acq.dwell_enqueue(d_x.data_ptr(), stream)
        res = acq.fetch_results(stream)
        found["caf"] = [(r.indext % spm, r.doppler_hz) for r in res]
        return res

    def search_plain(acq):
        acq.reset()
        acq.dwell_enqueue(d_x.data_ptr(), stream)
        acq.fetch_results(stream)
        out = []
        for s in range(S):
            g = [acq.grid(4 * s + i) for i in range(4)]  # IA, QA, IB, QB
            k = [np.argmax(p, axis=1) for p in g]
            rows = np.arange(len(bins))
            m = [p[rows, kk] for p, kk in zip(g, k)]
            n_qb = g[2][rows, k[3]] / fnf4  # the block's read of the IB plane (REFERENCE arithmetic)
            i_b = ~(m[0] / fnf4 >= m[2] / fnf4)
            q_b = ~(m[1] / fnf4 >= n_qb)
            grid = np.where(i_b[:, None], g[2], g[0]) + np.where(q_b[:, None], g[3], g[1])
            caf_i, caf_q = np.where(i_b, m[2], m[0]), np.where(q_b, m[3], m[1])
            kb = np.argmax(grid, axis=1)
            mb = grid[rows, kb] / fnf4
            b = int(np.argmax(mb))
            c = caf_ref.caf_filter(caf_i, caf_q, H, caf_ref.REFERENCE) if H > 0 else None
            d = caf_ref.first_max(c) if c is not None else b
            out.append((int(kb[b]) % spm, bins[d]))
        found["plain"] = out
        return out

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

    t = {"caf": [], "plain": []}
    for _ in range(args.rounds):
        if caf is not None:
            t["caf"].append(timed(search_caf, caf))
        if plain is not None:
            t["plain"].append(timed(search_plain, plain))
    out = {"command": "python3 profiles/tools/caf_time.py --warm %d --reps %d --rounds %d" % (args.warm, args.reps, args.rounds), "N": N, "sats": S, "bins": len(bins), "R": 4,
        "caf_half_window_bins": H}
    for k, v in t.items():
        if v:
            out[k + "_ms"] = float(np.median(v))
            out[k + "_ms_min_max"] = [min(v), max(v)]
    if t["caf"] and t["plain"]:
        apart = max(t["caf"]) < min(t["plain"]) or max(t["plain"]) < min(t["caf"])
        out["plain_over_caf"] = float(np.median(t["plain"]) / np.median(t["caf"])) if apart else None
        out["same_delays"] = [a[0] for a in found["caf"]] == [a[0] for a in found["plain"]]
        out["same_dopplers"] = [a[1] for a in found["caf"]] == [a[1] for a in found["plain"]]
    if "caf" in found:
        out["delays_found"] = [a[0] for a in found["caf"]]
    if args.select_us > 0.0:
        moved = 12.0 * N * S * len(bins)  # per grid row: two plane rows read, one grid row written
        out["select_kernel_us"] = args.select_us
        out["select_kernel_bytes"] = moved
        out["select_kernel_tb_per_s"] = moved / (args.select_us * 1e-6) / 1e12
        out["select_kernel_fraction_of_6.3_tb_per_s"] = out["select_kernel_tb_per_s"] / 6.3
        if t["caf"]:
            out["select_kernel_share_of_search"] = args.select_us * 1e-3 / float(np.median(t["caf"]))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    for e in (caf, plain):
        if e is not None:
            e.close()
    ctx.close()


if __name__ == "__main__":
    main()
