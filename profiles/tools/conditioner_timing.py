"""Timings of the signal conditioner on one MI355X (DESIGN.md, section "Signal conditioner"):

  (a) one 16 ms block of a 25 Msps cshort stream (400 000 samples, 1.6 MB): a conditioned push (D = 5, 64 taps, IF 4.3 MHz) next to
      a plain gc_stream_push of the same raw block, from page-locked and from pageable memory;
  (b) the 32-channel GPS L1 C/A open-loop batch (3 taps) on the 5 Msps conditioned ring against the same batch on the 25 Msps raw
      cshort ring: time per step and bytes read per step.

Host clock around work that ends in a synchronise; warm-up in front of every timed window; the two sides of a comparison alternate
inside one process and the rounds are printed one by one, so the spread is visible.

python profiles/tools/conditioner_timing.py [--reps 200] [--rounds 5] [--epochs 64] [--steps 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))

FS_IN, D, T, F_IF = 25e6, 5, 64, 4.3e6
BLOCK = 400_000  # 16 ms at 25 Msps


def taps64():
    k = np.arange(T) - (T - 1) / 2.0
    h = np.sinc(k * 0.8 / D) * np.hamming(T)
    return (h / h.sum()).astype(np.float32)


def timed(fn, sync, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e6


def push_timing(gnsscorr, torch, ctx, args):
    rng = np.random.Generator(np.random.PCG64(1))
    raw = np.round(rng.standard_normal((BLOCK, 2)) * 45.0).astype(np.int16)
    pinned = torch.from_numpy(raw.copy()).pin_memory()
    # rings of 32 blocks: nothing reads them, so no push waits for a reader
    plain = gnsscorr.IqStream(ctx, 32 * BLOCK, 25000, gnsscorr.GC_IQ_I16)
    ring = gnsscorr.IqStream(ctx, 32 * BLOCK // D, 5000, gnsscorr.GC_IQ_F32)
    cond = gnsscorr.Conditioner(ctx, ring, FS_IN, F_IF, D, taps64(), gnsscorr.GC_IQ_I16)
    legs = {
        "plain_push_pinned": (lambda: plain.push_pinned(pinned.data_ptr(), BLOCK), plain.synchronize),
        "conditioned_push_pinned": (lambda: cond.push_pinned(pinned.data_ptr(), BLOCK), ring.synchronize),
        "plain_push_pageable": (lambda: plain.push(raw), plain.synchronize),
        "conditioned_push_pageable": (lambda: cond.push(raw), ring.synchronize),
    }
    # one push at a time, each followed by a synchronise: the latency of a block; and back to back: the sustained cost per block
    out = {name: {"each_synchronised_us": [], "back_to_back_us": []} for name in legs}
    for name, (fn, sync) in legs.items():
        timed(fn, sync, 10)  # warm-up: code object, staging slots, first touch of the ring
    for _ in range(args.rounds):
        for name, (fn, sync) in legs.items():
            out[name]["each_synchronised_us"].append(round(timed(lambda: (fn(), sync()), sync, args.reps // 4), 2))
            out[name]["back_to_back_us"].append(round(timed(fn, sync, args.reps), 2))
    cond.close()
    ring.close()
    plain.close()
    return {"block_samples": BLOCK, "block_bytes": int(raw.nbytes), "outputs_per_block": BLOCK // D, "decimation": D, "taps": T, "legs": out}


def batch_timing(gnsscorr, torch, ctx, args):
    n_ch, n_taps, E = 32, 3, args.epochs
    rng = np.random.Generator(np.random.PCG64(2))
    raw = np.round(rng.standard_normal((E * 25000, 2)) * 45.0).astype(np.int16)
    rings = {
        "raw_25Msps_cshort": (gnsscorr.IqStream(ctx, 2 * E * 25000, 25000, gnsscorr.GC_IQ_I16), 25e6, 25000, gnsscorr.GC_IQ_I16, 4),
        "conditioned_5Msps_float": (gnsscorr.IqStream(ctx, 2 * E * 5000, 5000, gnsscorr.GC_IQ_F32), 5e6, 5000, gnsscorr.GC_IQ_F32, 8),
    }
    cond = gnsscorr.Conditioner(ctx, rings["conditioned_5Msps_float"][0], FS_IN, F_IF, D, taps64(), gnsscorr.GC_IQ_I16)
    for k in range(0, len(raw), BLOCK):
        rings["raw_25Msps_cshort"][0].push(raw[k:k + BLOCK])
        cond.push(raw[k:k + BLOCK])
    shifts = np.array([-0.5, 0.0, 0.5], np.float32)
    legs = {}
    for name, (ring, fs, n, fmt, elem) in rings.items():
        ring.synchronize()
        b = gnsscorr.TrackingBatch(ctx, n_ch, n_taps, 1023)
        b.set_input_format(fmt)
        recs = []
        for ch in range(n_ch):
            b.set_code(ch, gnsscorr.gps_l1_ca_code_gen_float(ch + 1), shifts)
            b.set_input_stream(ch, ring)
            fd = -4000.0 + 250.0 * ch
            recs.append([gnsscorr.epoch_params(e * n, 0.1 * ch, 2 * np.pi * fd / fs, -10.25 * ch, 1.023e6 * (1 + fd / 1575.42e6) / fs, n) for e in range(E)])
        b.set_nominal_length(n)
        d_params = torch.from_numpy(gnsscorr.epoch_params_array(recs).view(np.uint8)).cuda()
        d_out = torch.zeros(n_ch * E * n_taps, 2, device="cuda", dtype=torch.float32)
        legs[name] = (b, d_params, d_out, n_ch * E * n * elem)
    out = {name: {"bytes_read_per_step": legs[name][3], "ms_per_step": []} for name in legs}
    for name, (b, d_params, d_out, _) in legs.items():
        timed(lambda: b.run_dev(E, d_params.data_ptr(), d_out.data_ptr()), ctx.synchronize, 5)
    for _ in range(args.rounds):
        for name, (b, d_params, d_out, _) in legs.items():
            out[name]["ms_per_step"].append(round(timed(lambda: b.run_dev(E, d_params.data_ptr(), d_out.data_ptr()), ctx.synchronize, args.steps) / 1e3, 4))
    for name, (b, _, d_out, nbytes) in legs.items():
        ms = float(np.median(out[name]["ms_per_step"]))
        out[name]["median_ms_per_step"] = ms
        out[name]["logical_read_GB_per_s"] = round(nbytes / ms / 1e6, 1)
        out[name]["channel_epochs_per_s"] = round(n_ch * E / ms * 1e3)
        assert float(d_out.abs().max()) > 0.0
        b.close()
    cond.close()
    for ring, *_ in rings.values():
        ring.close()
    return {"channels": n_ch, "taps": n_taps, "epochs_per_step": E, "stream_bytes_resident": {"raw_25Msps_cshort": E * 25000 * 4, "conditioned_5Msps_float": E * 5000 * 8},
        "legs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", help="also write the JSON here")
    args = ap.parse_args()
    import torch
    import gnsscorr
    ctx = gnsscorr.Context(0)  # no GPU: this raises; a timing without the device means nothing
    res = {"push": push_timing(gnsscorr, torch, ctx, args), "batch": batch_timing(gnsscorr, torch, ctx, args)}
    ctx.close()
    txt = json.dumps(res)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
