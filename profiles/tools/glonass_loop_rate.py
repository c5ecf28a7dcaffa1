"""GLONASS L1 C/A closed-loop tracking at 6.625 Msps, time per channel-period in two forms:
  (a) the device loop (gc_trk_loop_start_glonass): 32 and 256 channels x 64 periods in ONE launch;
  (b) the host-loop adapter path (hip_glonass_ca_dll_pll_tracking): one HipMulticorrelator call -- input copy, launch, result
      copy -- per channel-period, driven from Python with the period's window and NCO scalars; the block's loop maths between two
      calls (a few dozen flops) is not counted, which favours (b).
The channels read 8 noise streams with frequency channels -4..+3; on noise the lock detector needs more than 64 periods to give up
(max_lock_fail = 50, one estimate per 21 periods), so every record of (a) is a tracked period.  Prints one JSON line.

    python profiles/tools/glonass_loop_rate.py [--reps 7]
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

FS, VL, PERIODS, N_STREAMS = 6_625_000, 6625, 64, 8


def conf(k, doppler):
    c = gnsscorr.GlonassLoopConf()
    for name, v in dict(fs_in=float(FS), band_carrier_freq_hz=1.602e9, channel_offset_hz=0.5625e6 * k, carrier_lock_th=0.85, acq_delay_samples=100.5,
            acq_doppler_hz=doppler, acq_samplestamp_samples=0, sample_counter=0, vector_length=VL, cn0_samples=20, cn0_min=25, max_lock_fail=50,
            pll_bw_hz=50.0, dll_bw_hz=2.0, early_late_space_chips=0.5).items():
        setattr(c, name, v)
    return c


def device_loop(ctx, streams, n_stream, n_channels, reps):
    dev = streams[0].device
    loop = gnsscorr.TrackingLoop(ctx, n_channels, 511)
    recs = torch.zeros(n_channels * PERIODS * gnsscorr.LOOP_RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    times = []
    for rep in range(reps + 1):  # the first run warms up: code object loaded
        for ch in range(n_channels):
            loop.set_input_dev(ch, streams[ch % N_STREAMS].data_ptr(), n_stream)
            loop.start_glonass(ch, conf(ch % 8 - 4, 100.0 * (ch % 50) - 2500.0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop.run_dev(PERIODS, recs.data_ptr(), side.cuda_stream)
        torch.cuda.synchronize()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    r = np.frombuffer(recs.cpu().numpy().tobytes(), gnsscorr.LOOP_RECORD_DTYPE).reshape(n_channels, PERIODS)
    loop.close()
    tracked = int(r["valid"].sum())
    return {"channels": n_channels, "periods": PERIODS, "tracked_records": tracked, "ms_min": min(times), "ms_median": statistics.median(times),
        "us_per_channel_period": 1e3 * statistics.median(times) / (n_channels * PERIODS), "realtime_factor": PERIODS / statistics.median(times),
        "runs_ms": [round(x, 4) for x in times]}


def host_loop(ctx, host_streams, n_channels, reps):
    """n_channels correlators (one per channel, as each block owns one), PERIODS calls each, channel after channel within a period."""
    ccode = gnsscorr.glonass_l1_ca_code_gen_float().astype(np.complex64)
    shifts = np.array([-0.5, 0.0, 0.5], np.float32)
    mcs, outs = [], []
    for ch in range(n_channels):
        mc = gnsscorr.HipMulticorrelator(ctx)
        mc.init(2 * VL, 3)
        mc.set_local_code_and_taps(511, ccode, shifts)
        mcs.append(mc)
        outs.append(np.zeros(3, np.complex64))
    step = float(np.float32(0.511e6 / FS))
    times = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        for p in range(PERIODS):
            for ch in range(n_channels):
                x = host_streams[ch % N_STREAMS]
                mcs[ch].set_input_output_vectors(outs[ch], x[p * VL:p * VL + 2 * VL])
                mcs[ch].Carrier_wipeoff_multicorrelator_resampler(0.1, 2 * np.pi * (0.5625e6 * (ch % 8 - 4)) / FS, 0.25, step, VL)
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    for mc in mcs:
        mc.close()
    return {"channels": n_channels, "periods": PERIODS, "ms_min": min(times), "ms_median": statistics.median(times),
        "us_per_channel_period": 1e3 * statistics.median(times) / (n_channels * PERIODS), "realtime_factor": PERIODS / statistics.median(times),
        "runs_ms": [round(x, 3) for x in times]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = gnsscorr.Context(0)
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    n_stream = (PERIODS + 3) * VL
    streams = [torch.randn(2 * n_stream, generator=g, device=dev, dtype=torch.float32) * 0.7071 for _ in range(N_STREAMS)]
    host_streams = [np.ascontiguousarray(s.cpu().numpy()).view(np.complex64) for s in streams]
    out = {"tool": "glonass_loop_rate", "fs": FS, "vector_length": VL, "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"), "reps": args.reps,
        "device_loop": [device_loop(ctx, streams, n_stream, n, args.reps) for n in (32, 256)],
        "host_loop": host_loop(ctx, host_streams, 32, max(2, args.reps // 2)),
        "timing": "host wall time, launch-inclusive; (a) one run_dev per measurement, channel starts outside the interval; (b) all calls of 64 periods"}
    d32, h = out["device_loop"][0], out["host_loop"]
    out["host_over_device_per_channel_period_32ch"] = h["us_per_channel_period"] / d32["us_per_channel_period"]
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
