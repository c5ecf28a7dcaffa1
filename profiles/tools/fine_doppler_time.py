#!/usr/bin/env python3
"""Times one call of the fine Doppler stage (gnsscorr.FineDoppler.estimate_stream: upload of the requests, the partial and finish
kernels, the fetch of the results) and sets it beside the existing way to a finer Doppler, the second search of make_two_steps, on
the same box in the same call.  P = 10, Z = 8, +-1 kHz (159 bins of fs / (80 N)):

  fine        R requests on the 10 N samples of a ring, ONE call
  two_steps   R single-satellite engines with make_2_steps (4 bins of 125 Hz): per satellite set_step_two(True, its coarse Doppler)
              and one dwell on the device block, with its fetch -- a second full search per satellite, to 125 Hz instead of 12.5 Hz

    python3 profiles/tools/fine_doppler_time.py [--only fine|two_steps] [--warm 3] [--reps 10] [--rounds 5] [--out profiles/fine_doppler_latest.json]

Both are synchronous calls, so wall-clock time around --reps calls behind --warm warm-up calls is taken; the two alternate --rounds
times and the median round is reported with the spread (min, max).  --only two_steps touches nothing of the fine Doppler stage and
runs on a tree that does not have it yet.  The VALU ceiling of acq_fine_partial_kernel is stated from its disassembled inner loop
(hipcc -S: 198 VALU instructions per run of 32 samples, the re-seed included, 126 of them packed f32) at the issue rates of
profiles/r02_valu_issue_rates.txt for 4 waves per SIMD (4.47 cycles a packed, 2.99 a plain instruction): --loop-cycles per sample
and wave, times 3 waves x tiles x 1024 samples, on 1024 SIMDs at 2.4 GHz."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))
import numpy as np

SHAPES = ((32, 25000), (8, 4000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="", choices=("", "fine", "two_steps"))
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop-cycles", type=float, default=(126 * 4.47 + 72 * 2.99) / 32, help="VALU issue cycles per sample and wave in the partial kernel's inner loop")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import gnsscorr
    ctx = gnsscorr.Context(0)
    dev = torch.device("cuda", 0)
    out = {"command": "python3 profiles/tools/fine_doppler_time.py --warm %d --reps %d --rounds %d%s" % (args.warm, args.reps, args.rounds,
        (" --only " + args.only) if args.only else ""), "shapes": []}
    for R, N in SHAPES:
        fs, P, Z = N * 1000, 10, 8
        rng = np.random.Generator(np.random.PCG64(7))
        codes = [gnsscorr.gps_l1_ca_code_gen_complex_sampled(s % 32 + 1, fs)[:N] for s in range(R)]
        n = np.arange(P * N)
        x = (rng.standard_normal(P * N) + 1j * rng.standard_normal(P * N)) * np.sqrt(0.5)
        delays = [(700 * s + 123) % N for s in range(R)]
        true = [250.0 * (s - R // 2) + 87.5 for s in range(R)]
        coarse = [250.0 * round(f / 250.0) for f in true]
        for s in range(R):
            x += np.sqrt(10.0 ** 4.7 / fs) * np.roll(np.tile(codes[s], P), delays[s]) * np.exp(2j * np.pi * true[s] * n / fs)
        x = x.astype(np.complex64)
        rec = {"requests": R, "N": N, "P": P, "Z": Z}
        t = {}

        if args.only in ("", "fine"):
            fd = gnsscorr.FineDoppler(ctx, R, fs, N, prn_replicas=P, zero_padding_factor=Z, alignment="exact")
            for s, c in enumerate(codes):
                fd.set_code(s, c)
            ring = gnsscorr.IqStream(ctx, capacity_samples=P * N + 64, max_window_samples=1024)
            first = ring.push(x)
            requests = [(s, delays[s], coarse[s]) for s in range(R)]

            def call_fine():
                return fd.estimate_stream(ring, first, requests)

            res = call_fine()
            rec["fine_error_hz_max"] = float(max(abs(r.doppler_hz - f) for r, f in zip(res, true)))
            rec["window_bins"] = int(res[0].window_bins)
            tiles = -(-P * N // 1024)
            rec["valu_ceiling_ms"] = R * tiles * 3 * 1024 * args.loop_cycles / (1024 * 2.4e9) * 1e3
            rec["valu_ceiling_source"] = "%.2f VALU issue cycles per sample and wave in the inner loop (hipcc -S x profiles/r02_valu_issue_rates.txt), 3 waves per workgroup, %d tiles per request" % (args.loop_cycles, tiles)
            t["fine"] = call_fine
        if args.only in ("", "two_steps"):
            d_x = torch.from_numpy(x.view(np.float32).copy()).to(dev)
            engines = []
            for s in range(R):
                e = gnsscorr.PcpsAcquisition(ctx, 1, fs, 1, 1, np.float32(fs) * np.float32(0.001), float(N), max(1, int(np.ceil(fs / 1.023e6))), 5000, 250,
                    make_2_steps=True, num_doppler_bins_step2=4, doppler_step2=125.0)
                e.set_local_code(0, codes[s])
                engines.append(e)

            def call_two_steps():
                out_ = []
                for s, e in enumerate(engines):
                    e.set_step_two(True, coarse[s])
                    out_.append(e.dwell_dev(d_x.data_ptr())[0])
                return out_

            call_two_steps()
            t["two_steps"] = call_two_steps

        def timed(fn):
            for _ in range(args.warm):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            return (time.perf_counter() - t0) / args.reps * 1e3

        ms = {k: [] for k in t}
        for _ in range(args.rounds):
            for k, fn in t.items():
                ms[k].append(timed(fn))
        for k, v in ms.items():
            rec[k + "_ms"] = float(np.median(v))
            rec[k + "_ms_min_max"] = [min(v), max(v)]
        if "fine" in ms:
            rec["valu_ceiling_frac_of_call"] = rec["valu_ceiling_ms"] / rec["fine_ms"]
        if len(ms) == 2:
            apart = max(ms["fine"]) < min(ms["two_steps"]) or max(ms["two_steps"]) < min(ms["fine"])
            rec["two_steps_over_fine"] = float(np.median(ms["two_steps"]) / np.median(ms["fine"])) if apart else None
        out["shapes"].append(rec)
        if "fine" in t:
            fd.close()
            ring.close()
        if "two_steps" in t:
            for e in engines:
                e.close()
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
