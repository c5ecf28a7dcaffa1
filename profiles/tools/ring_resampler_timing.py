"""Cost of the ring resampler on one MI355X ("Ring resampler"): one synchronised update() after a 16 ms push
of a 25 Msps cshort stream (400 000 samples), for

(a) RingResampler, direct mode, 25 -> 10 Msps (160 000 cshort outputs),
(b) RingResampler, polyphase mode, 25 -> 10 Msps with resampler_design(25e6, 10e6, 32) (160 000 gr_complex outputs),
(c) the comparison partner in the same run: RingDecimator at D = 5 with the taps of gc_acq_resampler_plan(25e6, 5e6) (80 000 outputs).

The push itself is synchronised before the clock starts.  Host clock; warm-up in front of every timed window; the legs alternate and
every round is printed, so the spread is visible.  Each leg runs in a child process of its own under a time limit, and nothing
further starts after a leg that failed.

python profiles/tools/ring_resampler_timing.py [--reps 30] [--rounds 5] [--design DESIGN.md]

The figures recorded in DESIGN.md come from the defaults."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))

FS_IN, FS_OUT, PHASES, DECIMATION = 25_000_000, 10_000_000, 32, 5
BLOCK = 400_000  # 16 ms at 25 Msps
BLOCK_US = 16000.0
LEGS = ("direct", "polyphase", "decimator")
BEGIN, END = "<!-- ring_resampler_timing:begin -->", "<!-- ring_resampler_timing:end -->"
LEG_LIMIT_S = 120


def leg(name, reps, rounds):
    """One leg in this process: prints {"leg", "rounds_us", "outputs", "taps"}."""
    import torch
    import gnsscorr
    ctx = gnsscorr.Context(0)  # no GPU: this raises; a timing without the device means nothing
    rng = np.random.Generator(np.random.PCG64(1))
    raw = np.clip(np.round(rng.standard_normal((BLOCK, 2)) * 45.0), -32767, 32767).astype(np.int16)
    pinned = torch.from_numpy(raw.copy()).pin_memory()
    src = gnsscorr.IqStream(ctx, 8 * BLOCK, 25_000, gnsscorr.GC_IQ_I16)
    if name == "direct":
        out = gnsscorr.IqStream(ctx, 8 * BLOCK * 2 // 5, 10_000, gnsscorr.GC_IQ_I16)
        dev, taps = gnsscorr.RingResampler(ctx, src, FS_IN, FS_OUT, out, "direct"), 0
    elif name == "polyphase":
        bank = gnsscorr.resampler_design(FS_IN, FS_OUT, PHASES)
        out = gnsscorr.IqStream(ctx, 8 * BLOCK * 2 // 5, 10_000, gnsscorr.GC_IQ_F32)
        dev, taps = gnsscorr.RingResampler(ctx, src, FS_IN, FS_OUT, out, "polyphase", bank), int(bank.shape[1])
    else:
        D, rfs, h, _ = gnsscorr.acq_resampler_plan(FS_IN, FS_IN // DECIMATION)
        assert D == DECIMATION
        out = gnsscorr.IqStream(ctx, 8 * BLOCK // D, 5_000, gnsscorr.GC_IQ_F32)
        dev, taps = gnsscorr.RingDecimator(ctx, src, D, h, out), len(h)
    made = []

    def push_update():
        src.push_pinned(pinned.data_ptr(), BLOCK)
        src.synchronize()
        t0 = time.perf_counter()
        made.append(dev.update()[1])
        out.synchronize()
        return time.perf_counter() - t0

    for _ in range(10):
        push_update()
    rounds_us = [round(float(np.mean([push_update() for _ in range(reps)])) * 1e6, 2) for _ in range(rounds)]
    for h in (dev, out, src):
        h.close()
    ctx.close()
    print(json.dumps({"leg": name, "rounds_us": rounds_us, "outputs": int(np.median(made)), "taps": taps}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg", choices=LEGS, help="run one leg in this process (what the tool starts for each leg)")
    ap.add_argument("--out", help="also write the JSON here")
    ap.add_argument("--design", help="DESIGN.md to update between the ring_resampler_timing markers")
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
    result = {"fs_in": FS_IN, "fs_out": FS_OUT, "block_samples": BLOCK, "reps": args.reps, "legs": got, "median_us": med,
        "share_of_16ms": {name: med[name] / BLOCK_US for name in LEGS}}
    txt = json.dumps(result)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(txt + "\n")
    if args.design:
        def row(name, what):
            return "%s: **%.1f us**, %.2f %% of the 16 ms (rounds: %s)." % (what, med[name], 100.0 * med[name] / BLOCK_US,
                ", ".join("%.1f" % v for v in got[name]["rounds_us"]))
        lines = [BEGIN,
            "Synchronised `update()` after a 16 ms push (400 000 cshort samples at 25 Msps), median of %d rounds of %d, host clock:" % (args.rounds, args.reps),
            "",
            "- " + row("direct", "direct 25 -> 10 Msps (%d cshort outputs)" % got["direct"]["outputs"]),
            "- " + row("polyphase", "polyphase 25 -> 10 Msps, `P = %d`, `T = %d` (%d gr_complex outputs)" % (PHASES, got["polyphase"]["taps"], got["polyphase"]["outputs"])),
            "- " + row("decimator", "`gc_ring_decimator_update`, `D = %d`, `T = %d` (%d gr_complex outputs), the comparison partner" % (DECIMATION, got["decimator"]["taps"],
                got["decimator"]["outputs"])),
            END]
        with open(args.design) as f:
            doc = f.read()
        doc, n = re.subn(re.escape(BEGIN) + ".*?" + re.escape(END), lambda _: "\n".join(lines), doc, flags=re.S)
        assert n == 1, "DESIGN.md has no ring_resampler_timing markers"
        with open(args.design, "w") as f:
            f.write(doc)


if __name__ == "__main__":
    main()
