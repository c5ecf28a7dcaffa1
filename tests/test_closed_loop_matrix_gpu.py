"""Every reachable instantiation of the closed-loop kernel, trk_closed_loop_kernel<taps {3, 5}, threads {1024, 512, 256} or the
high-dynamics 256, format {F32, I16, I8}, data tap {no, yes}>, in both LDS code-image modes trk_loop_plan() chooses between (the
resident doubled image and the per-period window), and the mixed kernel that dispatches the same bodies per channel -- against the CPU
restatement of the loop (tests/closed_loop_ref.py).  The cases (signals, configurations, engine shapes) are
tests/closed_loop_matrix_cases.py's; tests/test_closed_loop_matrix_inputs.py checks them on the CPU.

1. Anchors: for each (taps, pilot, high_dyn, format, LDS mode) the F32 engine at 1024 threads (high dynamics: 256) on the format's
   samples cast to float, against the restatement through _compare at its fixed-scenario gates (tol 3e-3, abs_tol 0).
2. Every other instantiation against its anchor on the same samples: 512 and 256 threads, and the I16 / I8 engines fed the integers the
   anchor saw as floats.  Block boundaries, state and flags equal; corr, accu and prompt_data within 2e-5 of max |corr|; Doppler
   within 0.02 Hz (the gates of test_closed_loop_workgroup_sizes_agree and the int8 test).  One sample is about 2e-3 of the prompt
   here, so a dropped, doubled or mis-extended sample misses the gate by two orders of magnitude.
3. Mixed engines of four kinds (3 / 5 taps x data / pilot), per format x {1024, 512, 256 threads, high dynamics}, on the resident
   and on the window image: byte-identical to the plain engines of check 2.

Before any launch the launch plan (tests/loop_plan_selftest.cpp, with this GPU's CU count) must give every engine shape the intended
(threads, resident): a case that drifted into the other mode would test nothing."""
import os
import subprocess

import numpy as np
import pytest

import closed_loop_matrix_cases as M
from test_loop_sync_gpu import _compare, _conf, _stream, _sync  # noqa: F401  (_stream: through closed_loop_matrix_cases.build)
from test_mixed_loop_gpu import _same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EQUAL_FIELDS = ("sample_counter", "current_prn_length_samples", "state", "valid", "integrating")
SUM_FIELDS = ("corr", "accu", "prompt_data")
SUM_GATE, DOPPLER_GATE_HZ = 2e-5, 0.02


def _ids(v):
    return "".join(str(v).split())


@pytest.fixture(scope="module")
def n_cus(gctx):
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def plans(tmp_path_factory, n_cus):
    """argument tuple -> (threads, resident) of every engine shape of the matrix, from the launch plan itself; asserted here, before
    any test of this file launches."""
    exe = str(tmp_path_factory.mktemp("loop_plan") / "loop_plan_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"),
        os.path.join(ROOT, "tests", "loop_plan_selftest.cpp"), "-o", exe])
    want = M.all_plan_tuples(n_cus)
    out = subprocess.run([exe] + list(want), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert len(lines) == len(want)
    got = {}
    for engine, line in zip(want, lines):
        threads, _floats, resident, _bytes = (int(v) for v in line.split())
        got[engine] = (threads, resident)
        assert got[engine] == want[engine], "engine %s: plan (threads, resident) %r, the matrix intends %r" % (engine, got[engine], want[engine])
    return got


@pytest.fixture(scope="module")
def bench(gctx, plans, n_cus):
    """Runs engines and keeps what the tests share: device copies of the sample streams, the records of every plain engine run so
    far (never modified) and the worst ratio against each gate."""
    import gnsscorr
    import torch
    fmt_id = {"f32": gnsscorr.GC_IQ_F32, "i16": gnsscorr.GC_IQ_I16, "i8": gnsscorr.GC_IQ_I8}

    class Bench:
        def __init__(self):
            self.dev, self.recs, self.worst = {}, {}, {}

        def tensor(self, key, sample_fmt, engine_fmt):
            """The samples of `sample_fmt` on the device, as the engine of `engine_fmt` reads them (F32: cast to float)."""
            k = (key, sample_fmt, engine_fmt)
            if k not in self.dev:
                q, f = M.samples(key, sample_fmt)
                host = f.view(np.float32) if engine_fmt == "f32" else q
                self.dev[k] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
            return self.dev[k]

        def start(self, loop, ch, key, sample_fmt, engine_fmt):
            c = M.build(key)
            loop.set_input_dev(ch, self.tensor(key, sample_fmt, engine_fmt).data_ptr(), c["x"].size)
            loop.set_sync(ch, _sync(gnsscorr, c["sync"]) if c["sync"] else None, c["data_code"])
            loop.start(ch, _conf(gnsscorr, **c["conf"]), c["code"])

        def plain(self, key, sample_fmt, engine_fmt, threads, mode):
            """Records of the plain engine <engine_fmt, threads (0: high dynamics)> in `mode` on the samples of `sample_fmt`."""
            k = (key, sample_fmt, engine_fmt, threads, mode)
            if k not in self.recs:
                channels, max_len, resident = M.engine_shape(mode, key, n_cus)
                assert plans[M.plan_tuple(mode, key, threads, n_cus)] == (threads or 256, resident)
                loop = gnsscorr.TrackingLoop(gctx, channels, max_len)
                loop.set_input_format(fmt_id[engine_fmt])
                if threads:
                    loop.set_geometry(threads_per_workgroup=threads, slices_per_channel=1)
                self.start(loop, 0, key, sample_fmt, engine_fmt)
                rec = loop.run(M.N_EP)
                loop.close()
                assert np.all(rec[1:].view(np.uint8) == 0), (k, "standby slots must give all-zero records")
                self.recs[k] = rec[0]
                self.recs[k].flags.writeable = False
            return self.recs[k]

        def mixed(self, hd, image, fmt, threads):
            keys = M.mixed_keys(hd, image)
            channels, max_len, resident = M.mixed_shape(image, n_cus)
            assert plans[M.mixed_plan_tuple(hd, image, threads, n_cus)] == (threads or 256, resident)
            loop = gnsscorr.TrackingLoop(gctx, channels, max_len, mixed=True)
            loop.set_input_format(fmt_id[fmt])
            if threads:
                loop.set_geometry(threads_per_workgroup=threads, slices_per_channel=1)
            for ch, key in enumerate(keys):
                self.start(loop, ch, key, fmt, fmt)
            rec = loop.run(M.N_EP)
            loop.close()
            assert np.all(rec[len(keys):].view(np.uint8) == 0), "standby slots must give all-zero records"
            return keys, rec

        def note(self, gate, fmt, threads, ratio):
            k = (gate, fmt, threads or "hd256")
            self.worst[k] = max(self.worst.get(k, 0.0), ratio)

    b = Bench()
    yield b
    for (gate, fmt, threads), ratio in sorted(b.worst.items(), key=str):
        print("closed-loop matrix, worst over the cases run: %-34s %-3s %-5s %.3g of the gate" % (gate, fmt, threads, ratio))
    b.dev.clear()


def _anchor_threads(key):
    return 0 if M.shape(key)[2] else 1024


CASE_MODES = [(key, mode) for key in M.REFERENCED for mode in M.modes_of(key)]


@pytest.mark.parametrize("key,mode", CASE_MODES, ids=_ids)
def test_anchor_equals_the_cpu_restatement(bench, oracle, key, mode):
    """Check 1: the F32 engine at 1024 threads (high dynamics: 256) on each format's samples cast to float, in this LDS mode."""
    taps, pilot = M.shape(key)[:2]
    for fmt in M.FORMATS:
        ref = M.reference(oracle, key, fmt)
        rec = bench.plain(key, fmt, "f32", _anchor_threads(key), mode)
        assert len(ref) == M.N_EP and np.all(rec["valid"] == 1) and np.all(rec["state"] == (4 if pilot else 2)), (key, mode, fmt)
        worst = max(np.max(np.abs((rec[k]["corr"][0:2 * taps:2] + 1j * rec[k]["corr"][1:2 * taps:2]) - ref[k]["corr"])) / abs(ref[k]["corr"][taps // 2])
            for k in range(M.N_EP))
        print("%s %s %s: anchor against the restatement, worst tap error %.3g of the prompt (gate 3e-3)" % (_ids(key), mode, fmt, worst))
        bench.note("anchor corr vs restatement (3e-3)", fmt, _anchor_threads(key), worst / 3e-3)
        try:
            _compare(rec, ref, taps)
        except AssertionError as e:
            raise AssertionError("%s %s %s: %s" % (_ids(key), mode, fmt, e)) from e


@pytest.mark.parametrize("key,mode", CASE_MODES + [("large_hd", "resident")], ids=_ids)
def test_every_instantiation_equals_its_anchor(bench, key, mode):
    """Check 2: <512>, <256> and the I16 / I8 engines, on the samples their anchor saw as floats."""
    for fmt in M.FORMATS:
        base = bench.plain(key, fmt, "f32", _anchor_threads(key), mode)
        top = float(np.max(np.abs(base["corr"])))
        assert np.all(base["valid"] == 1) and top > 0.5 * M.AMP * M.N * M.SCALE[fmt]
        for threads in M.thread_counts(key):
            if fmt == "f32" and threads == _anchor_threads(key):
                continue  # the anchor itself
            r = bench.plain(key, fmt, fmt, threads, mode)
            for f in EQUAL_FIELDS:
                assert np.array_equal(r[f], base[f]), (key, mode, fmt, threads, f)
            err = max(float(np.max(np.abs(r[f] - base[f]))) for f in SUM_FIELDS) / top
            dop = float(np.max(np.abs(r["carrier_doppler_hz"] - base["carrier_doppler_hz"])))
            print("%s %s %s %s threads: sums %.3g of max |corr| (gate %g), Doppler %.3g Hz (gate %g)" % (_ids(key), mode, fmt, threads or "hd 256", err,
                SUM_GATE, dop, DOPPLER_GATE_HZ))
            bench.note("sums vs anchor (2e-5 of max |corr|)", fmt, threads, err / SUM_GATE)
            bench.note("Doppler vs anchor (0.02 Hz)", fmt, threads, dop / DOPPLER_GATE_HZ)
            assert err <= SUM_GATE, (key, mode, fmt, threads, err)
            assert dop < DOPPLER_GATE_HZ, (key, mode, fmt, threads, dop)


@pytest.mark.parametrize("image", ["resident", "window"])
@pytest.mark.parametrize("hd", [False, True], ids=["plain", "high_dyn"])
def test_mixed_engine_equals_the_plain_engines(bench, hd, image):
    """Check 3: 3 / 5 taps x data / pilot in one mixed engine, per format and workgroup size, byte for byte the plain engines of check 2
    (a plain engine's records do not depend on its LDS mode: the resident ones are compared).  The window image takes a fifth slot, the
    large pilot row, in an engine of more slots than CUs: a mixed engine sizes its image by its started channels, not by max_code_len."""
    for fmt in M.FORMATS:
        for threads in ([0] if hd else [1024, 512, 256]):
            keys, rec = bench.mixed(hd, image, fmt, threads)
            for ch, key in enumerate(keys):
                want = bench.plain(key, fmt, fmt, threads, "resident")
                assert np.all(want["valid"] == 1), (key, fmt, threads)
                assert _same_bytes(rec[ch], want), (key, image, fmt, threads or "hd 256")


def test_plain_engine_records_do_not_depend_on_the_lds_mode(bench):
    """What check 3 leans on: the per-period window addresses the same chips in the same order as the resident image."""
    for key in M.MATRIX:
        for fmt in M.FORMATS:
            th = _anchor_threads(key)
            a, b = (bench.plain(key, fmt, fmt, th, mode) for mode in M.modes_of(key))
            assert _same_bytes(a, b), (key, fmt)
