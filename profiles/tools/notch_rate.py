"""Cost of the notch filter ring stage on one MI355X ("Notch filter"): one synchronised update() after a 16 ms
push of a 25 Msps gr_complex stream (400 000 samples, 12 500 segments of 32), for

(a) RingNotch with no segment flagged (unit noise, linear floor, threshold 1000): every output is copied,
(b) RingNotch with every segment flagged (a tone 30 dB above the noise behind the first block, which is the estimate), full mode,
    and the same in lite mode with a coefficient per segment,
(c) the comparison partner in the same run: RingDecimator with one tap and decimation 1 -- the same framework doing a copy.

The push itself is synchronised before the clock starts.  Host clock; warm-up in front of every timed window; every round is printed,
so the spread is visible.  Each leg runs in a child process of its own under a time limit, and nothing further starts after a leg
that failed.

python profiles/tools/notch_rate.py [--reps 30] [--rounds 5] [--out FILE]

The figures recorded in DESIGN.md come from the defaults."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))

FS = 25_000_000
BLOCK = 400_000  # 16 ms at 25 Msps: the default segments_est = 12500 segments of 32
BLOCK_US = 16000.0
LEGS = ("pass", "filter", "filter_lite", "decimator")
LEG_LIMIT_S = 120


def leg(name, reps, rounds):
    """One leg in this process: prints {"leg", "rounds_us", "outputs", "segments_filtered"}."""
    import torch
    import gnsscorr
    ctx = gnsscorr.Context(0)  # no GPU: this raises; a timing without the device means nothing
    rng = np.random.Generator(np.random.PCG64(1))
    noise = ((rng.standard_normal(BLOCK) + 1j * rng.standard_normal(BLOCK)) * np.sqrt(0.5)).astype(np.complex64)
    tone = (noise + np.sqrt(1000.0) * np.exp(2j * np.pi * 0.0837 * np.arange(BLOCK))).astype(np.complex64)  # 400 000 * 0.0837 is whole: blocks join
    first = torch.from_numpy(noise.view(np.float32).copy()).pin_memory()
    later = torch.from_numpy((tone if name.startswith("filter") else noise).view(np.float32).copy()).pin_memory()
    src = gnsscorr.IqStream(ctx, 8 * BLOCK, 25_000)
    out = gnsscorr.IqStream(ctx, 8 * BLOCK, 25_000)
    if name == "decimator":
        dev = gnsscorr.RingDecimator(ctx, src, 1, np.ones(1, np.float32), out)
    else:
        dev = gnsscorr.RingNotch(ctx, src, out, mode="lite" if name == "filter_lite" else "full", noise_floor="linear", threshold=1000.0)
    made = []

    def push_update(block):
        src.push_pinned(block.data_ptr(), BLOCK)
        src.synchronize()
        t0 = time.perf_counter()
        made.append(dev.update()[1])
        out.synchronize()
        return time.perf_counter() - t0

    estimate_us = push_update(first) * 1e6  # the notch estimates its floor on this block
    for _ in range(10):
        push_update(later)
    before = dev.state()["segments_filtered"] if name != "decimator" else 0
    rounds_us = [round(float(np.mean([push_update(later) for _ in range(reps)])) * 1e6, 2) for _ in range(rounds)]
    filtered = dev.state()["segments_filtered"] - before if name != "decimator" else 0
    for h in (dev, out, src):
        h.close()
    ctx.close()
    print(json.dumps({"leg": name, "rounds_us": rounds_us, "outputs": int(np.median(made)), "first_block_us": round(estimate_us, 1),
        "segments_filtered_per_block": filtered / float(reps * rounds)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg", choices=LEGS, help="run one leg in this process (what the tool starts for each leg)")
    ap.add_argument("--out", help="also write the JSON here")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.reps, args.rounds)
        return
    got = {}
    for name in LEGS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, "--reps", str(args.reps), "--rounds", str(args.rounds)],
            capture_output=True, text=True, timeout=LEG_LIMIT_S)
        sys.stderr.write(p.stderr)
        if p.returncode != 0:
            sys.exit("leg %s failed with status %d: nothing further is started" % (name, p.returncode))
        got[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(got[name]))
    med = {name: float(np.median(got[name]["rounds_us"])) for name in LEGS}
    result = {"fs": FS, "block_samples": BLOCK, "reps": args.reps, "legs": got, "median_us": med,
        "times_real_time": {name: BLOCK_US / med[name] for name in LEGS}, "ratio_to_decimator": {name: med[name] / med["decimator"] for name in LEGS}}
    txt = json.dumps(result)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
