"""Timings of the conditioner's output formats on one MI355X ("Integer output rings"), for ONE shape: a
25 Msps cshort stream, IF 4.3 MHz, D = 5, 64 taps, blocks of 400 000 raw samples (16 ms, 80 000 outputs):

  (a) a conditioned push of one block from page-locked memory into a GC_IQ_F32, a GC_IQ_I16 and a GC_IQ_I8 ring, back to back: the
      H2D copy of 1.6 MB and the conditioner kernel on the ring's copy stream.  The copy is the same in every leg, so a difference
      between legs is the kernel's (its store epilogue);
  (b) one launch of the 32-channel GPS L1 C/A open-loop tracking batch (3 taps, 64 epochs of 5000 samples) reading each of the
      three conditioned rings: time per launch and bytes read per launch.

Host clock around work that ends in a synchronise; warm-up in front of every timed window; the legs alternate inside one process
and the rounds are printed one by one, so the spread is visible.  A library that refuses an integer output ring (a checkout from
before they existed) runs the float legs alone: --tree points the tool at such a checkout, to compare its float leg with this one's.

python profiles/tools/cond_out_formats.py [--tree PATH] [--reps 200] [--rounds 7] [--steps 50] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FS_IN, D, T, F_IF = 25e6, 5, 64, 4.3e6
BLOCK = 400_000
N_CH, N_TAPS, EPOCHS, N_EPOCH = 32, 3, 64, 5000


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="root of the checkout whose library is measured (default: this one)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", help="also write the JSON here")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), "gnss-sdr-1_amd"))
    import torch
    import gnsscorr
    ctx = gnsscorr.Context(0)  # no GPU: this raises; a timing without the device means nothing
    rng = np.random.Generator(np.random.PCG64(1))
    n_blocks = EPOCHS * N_EPOCH * D // BLOCK  # 4 blocks fill the 64 epochs the batch reads
    raw = np.round(rng.standard_normal((n_blocks * BLOCK, 2)) * 45.0).astype(np.int16)
    pinned = torch.from_numpy(raw.copy()).pin_memory()
    legs, skipped = {}, {}
    for name, fmt, elem in (("float", gnsscorr.GC_IQ_F32, 8), ("cshort", gnsscorr.GC_IQ_I16, 4), ("cbyte", gnsscorr.GC_IQ_I8, 2)):
        # a ring of 32 blocks: nothing reads it while the pushes are timed, so no push waits for a reader
        ring = gnsscorr.IqStream(ctx, 32 * BLOCK // D, N_EPOCH, fmt)
        try:
            if fmt != gnsscorr.GC_IQ_F32:
                ring.accept_quantised_output()
            cond = gnsscorr.Conditioner(ctx, ring, FS_IN, F_IF, D, taps64(), gnsscorr.GC_IQ_I16)
        except (gnsscorr.GnsscorrError, AttributeError) as e:
            skipped[name] = str(e)
            ring.close()
            continue
        legs[name] = dict(ring=ring, cond=cond, fmt=fmt, elem=elem, push_us=[], batch_ms=[])
    push = {name: (lambda leg=leg: leg["cond"].push_pinned(pinned.data_ptr(), BLOCK)) for name, leg in legs.items()}
    for name, leg in legs.items():
        timed(push[name], leg["ring"].synchronize, 10)  # warm-up: code object, first touch of the ring
    for _ in range(args.rounds):
        for name, leg in legs.items():
            leg["push_us"].append(round(timed(push[name], leg["ring"].synchronize, args.reps), 2))
    # (b): fresh rings holding the 64 epochs from output 0 on, one batch per ring
    shifts = np.array([-0.5, 0.0, 0.5], np.float32)
    for name, leg in legs.items():
        leg["cond"].close()
        leg["ring"].close()
        ring = gnsscorr.IqStream(ctx, 2 * EPOCHS * N_EPOCH, N_EPOCH, leg["fmt"])
        if leg["fmt"] != gnsscorr.GC_IQ_F32:
            ring.accept_quantised_output()
        cond = gnsscorr.Conditioner(ctx, ring, FS_IN, F_IF, D, taps64(), gnsscorr.GC_IQ_I16)
        for k in range(n_blocks):
            cond.push_pinned(pinned.data_ptr() + k * BLOCK * 4, BLOCK)
        ring.synchronize()
        b = gnsscorr.TrackingBatch(ctx, N_CH, N_TAPS, 1023)
        b.set_input_format(leg["fmt"])
        recs = []
        for ch in range(N_CH):
            b.set_code(ch, gnsscorr.gps_l1_ca_code_gen_float(ch + 1), shifts)
            b.set_input_stream(ch, ring)
            fd = -4000.0 + 250.0 * ch
            recs.append([gnsscorr.epoch_params(e * N_EPOCH, 0.1 * ch, 2 * np.pi * fd / (FS_IN / D), -10.25 * ch, 1.023e6 * (1 + fd / 1575.42e6) / (FS_IN / D), N_EPOCH)
                for e in range(EPOCHS)])
        b.set_nominal_length(N_EPOCH)
        d_params = torch.from_numpy(gnsscorr.epoch_params_array(recs).view(np.uint8)).cuda()
        d_out = torch.zeros(N_CH * EPOCHS * N_TAPS, 2, device="cuda", dtype=torch.float32)
        leg.update(ring=ring, cond=cond, batch=b, run=(lambda b=b, p=d_params, o=d_out: b.run_dev(EPOCHS, p.data_ptr(), o.data_ptr())), keep=(d_params, d_out))
        timed(leg["run"], ctx.synchronize, 5)
    for _ in range(args.rounds):
        for name, leg in legs.items():
            leg["batch_ms"].append(round(timed(leg["run"], ctx.synchronize, args.steps) / 1e3, 4))
    res = {"shape": dict(fs_in=FS_IN, decimation=D, taps=T, translate_hz=F_IF, block_samples=BLOCK, outputs_per_block=BLOCK // D, channels=N_CH,
        batch_taps=N_TAPS, epochs=EPOCHS, samples_per_epoch=N_EPOCH), "tree": os.path.abspath(args.tree), "skipped": skipped, "legs": {}}
    for name, leg in legs.items():
        assert float(leg["keep"][1].abs().max()) > 0.0
        nbytes = N_CH * EPOCHS * N_EPOCH * leg["elem"]
        ms = float(np.median(leg["batch_ms"]))
        res["legs"][name] = dict(push_us_per_block=leg["push_us"], push_us_median=float(np.median(leg["push_us"])), push_us_spread=round(max(leg["push_us"]) - min(leg["push_us"]), 2),
            ring_bytes_per_block=BLOCK // D * leg["elem"], batch_ms_per_launch=leg["batch_ms"], batch_ms_median=ms, batch_bytes_read_per_launch=nbytes,
            batch_logical_read_GB_per_s=round(nbytes / ms / 1e6, 1))
        leg["batch"].close()
        leg["cond"].close()
        leg["ring"].close()
    ctx.close()
    txt = json.dumps(res)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
