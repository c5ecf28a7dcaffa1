"""One GPU's closed-loop share of BASELINE configs[4] (16 GPS L1 C/A + 8 Galileo E1, 5 taps, 4 ms + 8 BeiDou B1I, 25 Msps, 64 ms of
signal) timed in two forms, alternated in one process:
  (a) three engines on three HIP streams (the shape bench.py's closed_loop_cfg5_share times);
  (b) ONE mixed engine (gc_trk_loop_set_mixed) on one stream: the Galileo slots fill 16 of their 64 records.
Also a mixed engine holding only the 16 GPS channels against the homogeneous 16-GPS engine (what the union kernel's registers cost).
Prints one JSON line.  The process environment is left as found: GPU_MAX_HW_QUEUES is reported, never set, and bench.py is not
imported (importing it sets the variable).  Kernel times: run this under rocprofv3 --kernel-trace --stats in a separate run.

    python profiles/tools/loop_mixed_share.py [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "gnss-sdr-1_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import gnsscorr  # noqa: E402

FS, N = 25_000_000, 25000
MS = 64
N_STREAMS = 32
# (channels, replica samples, samples per chip, veml, chip rate, vector length, period, E-L spacing, VE-VL spacing, ms per period)
SPECS = [(16, 1023, 1, 0, 1.023e6, N, 0.001, 0.5, 0.0, 1), (8, 8184, 2, 1, 1.023e6, 4 * N, 0.004, 0.15, 0.6, 4),
    (8, 2046, 1, 0, 2.046e6, N, 0.001, 0.5, 0.0, 1)]


def conf(L, spc, veml, chip_rate, vlen, period, el, vel):
    c = gnsscorr.LoopConf()
    for k, v in dict(fs_in=float(FS), signal_carrier_freq_hz=1575.42e6, code_chip_rate_hz=chip_rate, code_period_s=period, carrier_lock_th=0.85,
            code_length_chips=L // spc, code_samples_per_chip=spc, vector_length=vlen, pull_in_time_s=2, veml=veml, pll_filter_order=3,
            dll_filter_order=2, cn0_samples=20, cn0_min=25, max_lock_fail=50, pll_bw_hz=40.0, dll_bw_hz=2.0, fll_bw_hz=35.0,
            early_late_space_chips=el, very_early_late_space_chips=vel, acq_delay_samples=0.0, acq_doppler_hz=1000.0).items():
        setattr(c, k, v)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = gnsscorr.Context(0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    n_stream = (MS + 1) * N
    streams = [torch.randn(2 * n_stream, generator=g, device=dev, dtype=torch.float32) * 0.7071 for _ in range(N_STREAMS)]
    rng = np.random.Generator(np.random.PCG64(1005))
    codes = [np.sign(rng.standard_normal(s[1])).astype(np.float32) for s in SPECS]
    confs = [conf(*s[1:9]) for s in SPECS]
    side = [torch.cuda.Stream(device=dev) for _ in range(3)]

    # (a) three engines, one per signal, one HIP stream each
    three = []
    for k, s in enumerate(SPECS):
        eng = gnsscorr.TrackingLoop(ctx, s[0], s[1])
        n_per = MS // s[9]
        three.append((eng, k, n_per, torch.zeros(s[0] * n_per * gnsscorr.LOOP_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)))
    # (b) one mixed engine: slots 0-15 GPS, 16-23 Galileo, 24-31 BeiDou; n_epochs sized for the shortest period
    n_all = sum(s[0] for s in SPECS)
    mixed = gnsscorr.TrackingLoop(ctx, n_all, max(s[1] for s in SPECS), mixed=True)
    mixed_recs = torch.zeros(n_all * MS * gnsscorr.LOOP_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    # GPS alone: homogeneous engine vs mixed engine
    gps_h = gnsscorr.TrackingLoop(ctx, 16, 1023)
    gps_m = gnsscorr.TrackingLoop(ctx, 16, 1023, mixed=True)
    gps_recs = torch.zeros(16 * MS * gnsscorr.LOOP_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def slots():
        # (signal k, channel of the signal, input stream index): bench.py's mapping of channels to streams
        for k, s in enumerate(SPECS):
            for ch in range(s[0]):
                yield k, ch, (k * 8 + ch) % N_STREAMS

    def run_three():
        for eng, k, n_per, recs in three:
            for kk, ch, si in slots():
                if kk == k:
                    eng.set_input_dev(ch, streams[si].data_ptr(), n_stream)
                    eng.start(ch, confs[k], codes[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for eng, k, n_per, recs in three:
            eng.run_dev(n_per, recs.data_ptr(), side[k].cuda_stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def run_mixed():
        for slot, (k, ch, si) in enumerate(slots()):
            mixed.set_input_dev(slot, streams[si].data_ptr(), n_stream)
            mixed.start(slot, confs[k], codes[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mixed.run_dev(MS, mixed_recs.data_ptr(), side[0].cuda_stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def run_gps(eng):
        for ch in range(16):
            eng.set_input_dev(ch, streams[ch].data_ptr(), n_stream)
            eng.start(ch, confs[0], codes[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run_dev(MS, gps_recs.data_ptr(), side[0].cuda_stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    run_three(), run_mixed(), run_gps(gps_h), run_gps(gps_m)  # warm-up: code objects loaded, LDS attributes set
    t = {"three": [], "mixed": [], "gps_h": [], "gps_m": []}
    for _ in range(args.reps):
        t["three"].append(run_three())
        t["mixed"].append(run_mixed())
        t["gps_h"].append(run_gps(gps_h))
        t["gps_m"].append(run_gps(gps_m))
    recs = np.frombuffer(mixed_recs.cpu().numpy().tobytes(), gnsscorr.LOOP_RECORD_DTYPE).reshape(n_all, MS)
    valid = recs["valid"].sum(axis=1)
    for e in three:
        e[0].close()
    mixed.close()
    gps_h.close()
    gps_m.close()
    ctx.close()

    def form(v):
        return {"ms_min": min(v), "ms_median": statistics.median(v), "realtime_factor": MS / min(v), "realtime_factor_median": MS / statistics.median(v),
            "runs_ms": [round(x, 4) for x in v]}
    out = {"tool": "loop_mixed_share", "ms_of_signal": MS, "channels": {"gps_l1_ca": 16, "galileo_e1_5tap": 8, "beidou_b1i": 8}, "fs": FS,
        "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "reps": args.reps,
        "three_engines_three_streams": form(t["three"]), "one_mixed_engine": form(t["mixed"]),
        "mixed_valid_records": {"gps": [int(v) for v in valid[:16]], "galileo": [int(v) for v in valid[16:24]], "beidou": [int(v) for v in valid[24:]]},
        "gps_only": {"homogeneous": form(t["gps_h"]), "mixed": form(t["gps_m"]),
            "mixed_over_homogeneous": statistics.median(t["gps_m"]) / statistics.median(t["gps_h"])},
        "timing": "host wall time of the run_dev calls of one form (launch-inclusive), inputs and channel starts outside the interval"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
