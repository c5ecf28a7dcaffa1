"""Kernel time of the signal conditioner per raw format on one MI355X ("Real IF samples"): the three complex
formats and the four real ones, in one process, in two configurations --

  (a) 25 Msps, IF = fs / 4, D = 5, T = 64 (the headline rate);   (b) 25 Msps, no mixer, D = 1, T = 33.

Every format pushes the same number of SAMPLES per block (1 048 576, from page-locked memory), the formats alternate inside every
round, and a warm-up round comes first.  Kernel times come from the kernel trace of a profiler, not from the host clock:

  rocprofv3 --kernel-trace --stats -d OUT -o cond -- python profiles/tools/conditioner_real_timing.py --rounds 20
  python profiles/tools/conditioner_real_timing.py --summarise OUT/.../cond_kernel_stats.csv --rounds 20

--summarise turns the profiler's per-kernel totals into microseconds per million input samples (the FMT template argument in a
kernel's name is the format's number; the warm-up round is part of the totals and of the divisor).  The profiled process launches
nothing but those rounds, so every cond_fir_decim_kernel in the statistics belongs to the divisor.

  python profiles/tools/conditioner_real_timing.py --one-second

is a run of its own, without the profiler: from the host clock and without a gate, the wall time of pushing 1 s of a 25 Msps stream
(25 blocks of 1 000 000 samples, back to back, one synchronise at the end; D = 5, T = 64, IF = fs / 4) as GC_RAW_REAL_2BIT and as
complex64 through push_pinned."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))

FS_IN = 25e6
BLOCK = 1 << 20
CONFIGS = {"a_D5_T64_IF_fs4": (5, 64, FS_IN / 4), "b_D1_T33_no_mixer": (1, 33, 0.0)}
#          name: (format number, bytes per sample)
FORMATS = {"IQ_F32": (0, 8.0), "IQ_I16": (1, 4.0), "IQ_I8": (2, 2.0), "REAL_F32": (16, 4.0), "REAL_I16": (17, 2.0), "REAL_I8": (18, 1.0), "REAL_2BIT": (19, 0.25)}


def taps(T, D):
    k = np.arange(T) - (T - 1) / 2.0
    h = np.sinc(k * 0.8 / D) * np.hamming(T)
    return (h / h.sum()).astype(np.float32)


def pinned_block():
    """8 MiB of page-locked int8 in 1 .. 100: a block of 1 048 576 samples in any format (as float32 the bytes are finite values)."""
    import torch
    rng = np.random.Generator(np.random.PCG64(3))
    return torch.from_numpy(rng.integers(1, 101, 8 * BLOCK, dtype=np.int64).astype(np.int8)).pin_memory()


def run(args):
    import gnsscorr
    ctx = gnsscorr.Context(0)  # no GPU: this raises; a timing without the device means nothing
    pinned = pinned_block()
    legs = {}
    for cname, (D, T, f) in CONFIGS.items():
        for fname, (fmt, _) in FORMATS.items():
            ring = gnsscorr.IqStream(ctx, 4 * BLOCK, 4096, gnsscorr.GC_IQ_F32)
            legs[(cname, fname)] = (ring, gnsscorr.Conditioner(ctx, ring, FS_IN, f, D, taps(T, D), fmt))
    for _ in range(args.rounds + 1):  # the first round is the warm-up
        for ring, cond in legs.values():
            cond.push_pinned(pinned.data_ptr(), BLOCK)
        for ring, _ in legs.values():
            ring.synchronize()
    for ring, cond in legs.values():
        cond.close()
        ring.close()
    ctx.close()
    print(json.dumps({"block_samples": BLOCK, "rounds": args.rounds + 1, "samples_per_leg": (args.rounds + 1) * BLOCK}))


def one_second(args):
    import gnsscorr
    ctx = gnsscorr.Context(0)
    pinned = pinned_block()
    res = {"one_second_push_ms": {}}
    for fname in ("REAL_2BIT", "IQ_F32"):
        times = []
        for rep in range(4):
            ring = gnsscorr.IqStream(ctx, 6_000_000, 4096, gnsscorr.GC_IQ_F32)
            cond = gnsscorr.Conditioner(ctx, ring, FS_IN, FS_IN / 4, 5, taps(64, 5), FORMATS[fname][0])
            cond.push_pinned(pinned.data_ptr(), 1_000_000)
            ring.synchronize()
            t0 = time.perf_counter()
            for _ in range(25):
                cond.push_pinned(pinned.data_ptr(), 1_000_000)
            ring.synchronize()
            times.append(round((time.perf_counter() - t0) * 1e3, 3))
            cond.close()
            ring.close()
        res["one_second_push_ms"][fname] = times
    ctx.close()
    print(json.dumps(res))


def summarise(args):
    by_name = {v[0]: k for k, v in FORMATS.items()}
    rows = {}
    with open(args.summarise) as fh:
        for r in csv.DictReader(fh):
            m = re.search(r"cond_fir_decim_kernel<\(?(?:int\))?(\d+), (\d+), (true|false)>", r["Name"])
            if not m:
                continue
            key = ("a_D5_T64_IF_fs4" if m.group(3) == "true" else "b_D1_T33_no_mixer", by_name[int(m.group(1))])
            rows[key] = rows.get(key, 0.0) + float(r["TotalDurationNs"])
    samples = (args.rounds + 1) * BLOCK
    out = {"%s %s" % k: round(ns / 1e3 / (samples / 1e6), 2) for k, ns in sorted(rows.items())}
    print(json.dumps({"kernel_us_per_million_input_samples": out}, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--summarise", help="kernel stats CSV of the profiler run")
    ap.add_argument("--one-second", action="store_true", help="the wall-time leg alone (run it without the profiler)")
    a = ap.parse_args()
    summarise(a) if a.summarise else one_second(a) if a.one_second else run(a)
