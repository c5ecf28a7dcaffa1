"""Cost of pulse blanking in the signal conditioner on one MI355X ("Pulse blanking"):

the synchronised push of one 16 ms block of a 25 Msps cshort stream (400 000 samples, 1.6 MB; D = 5, 64 taps, IF 4.3 MHz) from
page-locked memory, WITH pulse blanking at the reference adapter's default parameters (pfa 0.04, length 32, segments_est 12500,
segments_reset 5000000) and WITHOUT, on two conditioners of the same process.  The stream is noise (sigma 45 LSB) with DME-like
pulse pairs; the first blocks (warm-up) carry the blanked conditioner through its 12500-segment estimate (exactly one block), so the
timed pushes run the steady 64-segments-per-step decisions.

Host clock around push + synchronise; warm-up in front of every timed window; the two legs alternate inside one process and every
round is printed, so the spread is visible.  The difference is taken round by round (same box, same minute).

python profiles/tools/blanking_timing.py [--reps 100] [--rounds 7] [--design DESIGN.md]"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))

FS_IN, D, T, F_IF = 25e6, 5, 64, 4.3e6
BLOCK = 400_000  # 16 ms at 25 Msps
BEGIN, END = "<!-- blanking_timing:begin -->", "<!-- blanking_timing:end -->"


def taps64():
    k = np.arange(T) - (T - 1) / 2.0
    h = np.sinc(k * 0.8 / D) * np.hamming(T)
    return (h / h.sum()).astype(np.float32)


def block_with_pulses(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((BLOCK, 2)) * 45.0
    # pulse pairs of 3.5 us (88 samples), 12 us apart, about 2700 pairs per second: 43 per block
    for start in rng.integers(0, BLOCK - 500, 43):
        for off in (0, 300):
            k = np.arange(88)
            env = 2000.0 * np.exp(-0.5 * ((k - 44) / 18.0) ** 2)
            ph = 2 * np.pi * 0.12 * k
            x[start + off:start + off + 88, 0] += env * np.cos(ph)
            x[start + off:start + off + 88, 1] += env * np.sin(ph)
    return np.clip(np.round(x), -32767, 32767).astype(np.int16)


def timed(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", help="also write the JSON here")
    ap.add_argument("--design", help="DESIGN.md to update between the blanking_timing markers")
    args = ap.parse_args()
    import torch
    import gnsscorr
    ctx = gnsscorr.Context(0)  # no GPU: this raises; a timing without the device means nothing
    raw = block_with_pulses(1)
    pinned = torch.from_numpy(raw.copy()).pin_memory()
    legs = {}
    for name in ("without_blanking", "with_blanking"):
        ring = gnsscorr.IqStream(ctx, 32 * BLOCK // D, 5000, gnsscorr.GC_IQ_F32)  # nothing reads it: no push waits for a reader
        cond = gnsscorr.Conditioner(ctx, ring, FS_IN, F_IF, D, taps64(), gnsscorr.GC_IQ_I16)
        if name == "with_blanking":
            cond.set_pulse_blanking()  # the reference adapter's defaults
        legs[name] = (cond, ring)

    def push(name):
        cond, ring = legs[name]
        cond.push_pinned(pinned.data_ptr(), BLOCK)
        ring.synchronize()

    for name in legs:
        timed(lambda: push(name), 10)  # warm-up: code objects, first touch, and the whole noise-floor estimate
    state = legs["with_blanking"][0].blanking_info()
    assert state["n_segments"] >= 12500 and state["segments_decided"] == 10 * BLOCK // 32, state
    out = {name: [] for name in legs}
    for _ in range(args.rounds):
        for name in legs:
            out[name].append(round(timed(lambda: push(name), args.reps), 2))
    state = legs["with_blanking"][0].blanking_info()
    for cond, ring in legs.values():
        cond.close()
        ring.close()
    ctx.close()
    diff = [round(a - b, 2) for a, b in zip(out["with_blanking"], out["without_blanking"])]
    res = {"block_samples": BLOCK, "block_bytes": int(raw.nbytes), "decimation": D, "taps": T, "reps": args.reps,
        "blanking": {"pfa": 0.04, "length": 32, "segments_est": 12500, "segments_reset": 5000000, "segments_per_block": BLOCK // 32,
            "blanked_fraction": round(state["segments_blanked"] / state["segments_decided"], 4)},
        "synchronised_push_us": out, "difference_us": diff,
        "median_us": {"without_blanking": float(np.median(out["without_blanking"])), "with_blanking": float(np.median(out["with_blanking"])),
            "difference": float(np.median(diff))}}
    txt = json.dumps(res)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    if args.design:
        m = res["median_us"]
        lines = [BEGIN,
            "Synchronised push of one 16 ms block (400 000 cshort samples, `D = 5`, 64 taps, page-locked), median of %d rounds of %d pushes:" % (args.rounds, args.reps),
            "without blanking **%.1f us** (rounds: %s), with blanking **%.1f us** (rounds: %s), difference **%.1f us** (round by round: %s);" % (
                m["without_blanking"], ", ".join("%.1f" % v for v in out["without_blanking"]), m["with_blanking"],
                ", ".join("%.1f" % v for v in out["with_blanking"]), m["difference"], ", ".join("%.1f" % v for v in diff)),
            "%d segments per block, %.2f %% of them blanked." % (BLOCK // 32, 100.0 * res["blanking"]["blanked_fraction"]),
            END]
        with open(args.design) as f:
            doc = f.read()
        doc, n = re.subn(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: "\n".join(lines), doc, flags=re.S)
        assert n == 1, "DESIGN.md has no blanking_timing markers"
        with open(args.design, "w") as f:
            f.write(doc)


if __name__ == "__main__":
    main()
