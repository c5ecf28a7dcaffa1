#!/usr/bin/env python3
"""Times the signal generator stage: one second of a 25 Msps scene synthesised into a ring on the device, for S = 1, 8 and 32 GPS
L1 C/A satellites (with data), noise on and off, GC_IQ_F32 and GC_IQ_I8 rings, the tables in HBM and -- where S x 1023 entries fit --
in LDS; and, for the same scene on the same box, the torch expression of examples/receiver_bench.py:39-56 with the round trip it
makes: float64 temporaries on the device, the copy to pinned host memory, and the pushes back into a ring over the host link.  That
expression is what the stage replaces, so it is the baseline.

    python3 profiles/tools/siggen_time.py [--warm 2] [--reps 5] [--rounds 3] [--out profiles/siggen_latest.json]

A host clock around --reps generate(one second) calls that end in a synchronise of the ring's stream (a call is milliseconds long,
the clock's part is microseconds), behind --warm warm-up calls; the placements alternate --rounds times and the median round is
reported with the spread.  The store roofline is the ring's bytes per sample (8 for GC_IQ_F32, 2 for GC_IQ_I8) over the 6.4 TB/s a
bare store loop reaches on this chip (profiles/tools/write_ceiling.hip); the mirror part, at most max_window samples
per wrap, is not counted."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))
import numpy as np

FS = 25_000_000
N = FS // 1000
STORE_BYTES_PER_S = 6.4e12
CAPACITY = 1 << 22  # 4 Mi samples: a second is six pieces of the ring


def scene(gnsscorr, n_sats):
    rng = np.random.Generator(np.random.PCG64(2024))
    sats = []
    for s in range(n_sats):
        doppler, delay, cn0 = float(rng.uniform(-4500, 4500)), int(rng.integers(0, N)), float(rng.uniform(47, 51))
        rate = 1.023e6 * (1 + doppler / 1575.42e6)
        comp = dict(table=gnsscorr.gps_l1_ca_code_gen_float(s % 32 + 1), periods_per_symbol=20)
        sats.append(gnsscorr.SiggenSatellite(doppler, rate / 1023.0 / FS, [comp], amplitude=float(np.sqrt(10 ** (cn0 / 10) / FS)),
            code_phase0_periods=(1.0 - delay / N) % 1.0))
    return sats


def time_generator(args, ctx, gnsscorr, sats, noise, fmt, placement):
    ring = gnsscorr.IqStream(ctx, CAPACITY, 2 * N, iq_format=fmt)
    if fmt != gnsscorr.GC_IQ_F32:
        ring.accept_quantised_output()
    gen = gnsscorr.SignalGenerator(ctx, ring, FS, sats, noise_sigma=float(np.sqrt(0.5)) if noise else 0.0, seed=7, table_placement=placement)
    if fmt != gnsscorr.GC_IQ_F32:
        gen.set_output_scale(32.0)
    for _ in range(args.warm):
        gen.generate(FS)
    ring.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        gen.generate(FS)
    ring.synchronize()
    dt = (time.perf_counter() - t0) / args.reps
    gen.close()
    ring.close()
    return dt


def time_torch_expression(args, ctx, gnsscorr, n_sats, noise):
    """examples/receiver_bench.py:39-56 for the same scene, then its round trip: to pinned host memory and back into a ring in 16 ms
    blocks."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.Generator(np.random.PCG64(2024))
    truth = [dict(doppler=float(rng.uniform(-4500, 4500)), delay=int(rng.integers(0, N)), cn0=float(rng.uniform(47, 51))) for _ in range(n_sats)]
    n, n_ms = FS, 1000
    ring = gnsscorr.IqStream(ctx, CAPACITY, 2 * N)
    block = 16 * N

    def once():
        t = torch.arange(n, device=dev, dtype=torch.float64)
        gen = torch.Generator(device=dev)
        gen.manual_seed(7)
        if noise:
            x = torch.complex(torch.randn(n, device=dev, generator=gen), torch.randn(n, device=dev, generator=gen)) * (0.5 ** 0.5)
        else:
            x = torch.zeros(n, device=dev, dtype=torch.complex64)
        for s, tr in enumerate(truth):
            code = torch.from_numpy(gnsscorr.gps_l1_ca_code_gen_float(s % 32 + 1)).to(dev)
            rate = 1.023e6 * (1 + tr["doppler"] / 1575.42e6) / FS
            ph = (1023.0 - tr["delay"] * 1.023e6 / FS) + t * rate
            chip = torch.remainder(torch.floor(ph), 1023).long()
            bits = torch.from_numpy(rng.integers(0, 2, n_ms // 20 + 2) * 2.0 - 1.0).to(dev)
            sym = bits[torch.clamp((torch.floor(ph / 1023.0) // 20).long(), 0, bits.numel() - 1)]
            amp = (10 ** (tr["cn0"] / 10) / FS) ** 0.5
            phase = torch.remainder(tr["doppler"] * t / FS, 1.0) * (2 * np.pi)
            x += (amp * code[chip] * sym) * torch.complex(torch.cos(phase), torch.sin(phase)).to(torch.complex64)
        host = torch.view_as_real(x.to(torch.complex64)).cpu().pin_memory()
        del x, t
        torch.cuda.synchronize()
        t_made = time.perf_counter()
        for first in range(0, n, block):
            ring.push_pinned(host.data_ptr() + 8 * first, min(block, n - first))
        ring.synchronize()
        return t_made

    for _ in range(max(1, args.warm - 1)):
        once()
    made, total = [], []
    for _ in range(max(2, args.reps // 2)):
        t0 = time.perf_counter()
        t_made = once()
        t1 = time.perf_counter()
        made.append(t_made - t0)
        total.append(t1 - t0)
    ring.close()
    return float(np.median(made)), float(np.median(total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating timed rounds of each placement; the median is reported")
    ap.add_argument("--sats", type=int, nargs="*", default=[1, 8, 32])
    ap.add_argument("--no-torch", action="store_true", help="skip the torch expression")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import gnsscorr
    ctx = gnsscorr.Context(0)
    rows = []
    for n_sats in args.sats:
        sats = scene(gnsscorr, n_sats)
        fits_lds = n_sats * 1023 <= 15360
        for noise in (False, True):
            for fmt_name, fmt, elem in (("GC_IQ_F32", gnsscorr.GC_IQ_F32, 8), ("GC_IQ_I8", gnsscorr.GC_IQ_I8, 2)):
                placements = ["hbm", "lds"] if fits_lds else ["hbm"]
                times = {p: [] for p in placements}
                for _ in range(args.rounds):
                    for p in placements:
                        times[p].append(time_generator(args, ctx, gnsscorr, sats, noise, fmt, p))
                row = {"sats": n_sats, "noise": noise, "ring": fmt_name}
                for p in placements:
                    med = float(np.median(times[p]))
                    row[p + "_ms"] = 1e3 * med
                    row[p + "_ms_min_max"] = [1e3 * min(times[p]), 1e3 * max(times[p])]
                    row[p + "_samples_per_s"] = FS / med
                    row[p + "_store_roofline_fraction"] = (FS * elem / STORE_BYTES_PER_S) / med
                if fits_lds:
                    row["lds_over_hbm"] = row["lds_ms"] / row["hbm_ms"]
                rows.append(row)
                print(json.dumps(row), flush=True)
            if not args.no_torch:
                made, total = time_torch_expression(args, ctx, gnsscorr, n_sats, noise)
                row = {"sats": n_sats, "noise": noise, "torch_expression_ms": 1e3 * made, "torch_expression_and_round_trip_ms": 1e3 * total}
                rows.append(row)
                print(json.dumps(row), flush=True)
    out = {"command": "python3 profiles/tools/siggen_time.py --warm %d --reps %d --rounds %d" % (args.warm, args.reps, args.rounds), "fs": FS,
        "seconds_per_call": 1.0, "rows": rows}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
