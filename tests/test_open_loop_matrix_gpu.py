"""Every reachable instantiation of the open-loop multicorrelator, trk_multicorrelator_kernel<taps 1..8, (plain, high-dynamics
resampler, high-dynamics, complex chips) x (F32, I16, I8) or the 16-bit mode>, against the float64 restatement of the operation
(tests/open_loop_ref.py) on the inputs of tests/open_loop_matrix_cases.py, which tests/test_open_loop_matrix_inputs.py checks on the CPU:
88 instantiations, none left to the draw of a seed.

Per (mode, format), tap counts 1..8 inside:
* the matrix launch -- 2 channels x 11 epochs, every record different, windows that reach each branch of trk_loop, poison around
  every window -- with 1 and with 3 slices;
* every output finite; float modes within the fuzz test's bar of the restatement (1e-4 max_t |ref[t]| + 3e-5 scale sqrt(n), 6e-5 for
  complex chips; an empty window gives exact zeros); the 16-bit mode within test_16sc_gpu.py's MAX_LSB of the compiled oracle;
* 1 slice and 3 slices within the bar of each other (16-bit mode: integer sums, equal);
* every launch twice: the same bytes.
Smaller tables (open_loop_matrix_cases.py): the carrier re-synchronisation at chunk 64, the launch whose LDS is below the code table
(window, and lookups in global memory, real and complex chips), the 31-chip code whose window wraps more than twice, and the level-1
objects with every overload -- the only way to the high-dynamics resampler with the plain rotator.

The worst error / bar per (mode, format) is printed; the figures of the last MI355X run are in open_loop_matrix_cases.py's docstring."""
import numpy as np
import pytest

import open_loop_matrix_cases as M
from test_16sc_gpu import MAX_LSB

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bench(gctx, oracle):
    """Runs launches and keeps what the tests share: the device copies of the sample streams and the worst ratio per (mode, format)."""
    import gnsscorr
    import torch
    fmt_id = {"f32": gnsscorr.GC_IQ_F32, "i16": gnsscorr.GC_IQ_I16, "i8": gnsscorr.GC_IQ_I8}

    class Bench:
        def __init__(self):
            self.dev, self.worst = {}, {}

        def tensor(self, launch):
            key = (launch.stream, M.stream_fmt(launch), launch.mode in M.HD and launch.stream == "matrix")
            if key not in self.dev:
                q = M.samples(oracle, launch.stream, M.stream_fmt(launch), launch.mode in M.HD)[0]
                self.dev[key] = torch.from_numpy(q).cuda()
                # the case table counts a window's alignment from the allocation
                assert self.dev[key].data_ptr() % (M.ALIGN * 2 * q.itemsize) == 0
            return self.dev[key]

        def batch(self, launch, n_slices):
            """The launch's batch, run twice: the outputs of the first run, [channel][epoch][tap] (16-bit mode: [...][2])."""
            d = self.tensor(launch)
            n_ch, n_ep = len(launch.recs), len(launch.recs[0])
            b = gnsscorr.TrackingBatch(gctx, n_ch, launch.n_taps, launch.max_code_len, high_dyn=(launch.mode == "hd_full"))
            if launch.mode == "complex":
                b.set_complex_codes(True)
            if launch.mode == "sc16":
                b.set_16sc(True)
            elif launch.fmt != "f32":
                b.set_input_format(fmt_id[launch.fmt])
            for ch in range(n_ch):
                setter = {"complex": b.set_code_complex, "sc16": b.set_code_16sc}.get(launch.mode, b.set_code)
                setter(ch, launch.codes[ch], launch.shifts)
                b.set_input_dev(ch, d.data_ptr() + launch.binds[ch] * 2 * d.element_size(), launch.n_iq[ch])
            b.set_slices(n_slices)
            params = gnsscorr.epoch_params_array([[r.params for r in recs] for recs in launch.recs])
            if launch.on_device:
                b.set_nominal_length(max(r.n for recs in launch.recs for r in recs))
                d_par = torch.from_numpy(params.view(np.uint8)).cuda()
                d_out = [torch.zeros(n_ch * n_ep * launch.n_taps, 2, dtype=torch.float32, device="cuda") for _ in range(2)]
                torch.cuda.synchronize()
                for o in d_out:
                    b.run_dev(n_ep, d_par.data_ptr(), o.data_ptr())
                gctx.synchronize()
                torch.cuda.synchronize()
                out = [o.cpu().numpy().view(np.complex64).reshape(n_ch, n_ep, launch.n_taps) for o in d_out]
            else:
                out = [b.run(n_ep, params) for _ in range(2)]
            b.close()
            assert out[0].tobytes() == out[1].tobytes(), (launch.table, launch.mode, launch.fmt, launch.n_taps, n_slices, "two runs differ")
            return out[0]

        def check(self, launch, out, what):
            """`out` against the launch's reference at the bar; returns the bars (float modes)."""
            where = (launch.table, launch.mode, launch.fmt, launch.n_taps, what)
            key = (launch.mode, launch.fmt)
            if launch.mode == "sc16":
                ref, exact = M.compiled(oracle, launch)
                assert np.array_equal(ref.astype(np.int32), exact), where  # (asserted on the CPU too: nothing saturates on the way)
                d = np.abs(np.asarray(out).astype(np.int32).reshape(exact.shape) - exact)
                assert d.max() <= MAX_LSB, where + (int(d.max()),)
                self.worst[key] = max(self.worst.get(key, 0), int(d.max()))
                return None
            assert np.all(np.isfinite(np.asarray(out).view(np.float32))), where
            ref, bar = M.reference(oracle, launch), M.bars(oracle, launch)
            for ch, recs in enumerate(launch.recs):
                for k, r in enumerate(recs):
                    err = float(np.max(np.abs(out[ch][k] - ref[ch][k])))
                    assert err <= bar[ch][k], where + (ch, k, r.tag, r.n, err, bar[ch][k], out[ch][k], ref[ch][k])
                    if r.n:
                        self.worst[key] = max(self.worst.get(key, 0.0), err / bar[ch][k])
            return bar

        def report(self, mode, fmt):
            w = self.worst.get((mode, fmt))
            if w is not None:
                print(("device against oracle, worst LSB difference, %-12s %s: %d" if mode == "sc16" else "device against restatement, worst error / bar, %-12s %s: %.3f") % (mode, fmt, w))

    return Bench()


@pytest.mark.parametrize("mode,fmt", M.BATCH, ids=["%s-%s" % k for k in M.BATCH])
def test_matrix_launch_every_tap_count(bench, oracle, mode, fmt):
    for n_taps in M.TAPS:
        launch = M.matrix_launch(oracle, mode, fmt, n_taps)
        outs = {}
        for n_slices in launch.slicings:
            outs[n_slices] = bench.batch(launch, n_slices)
            bar = bench.check(launch, outs[n_slices], "%d slices" % n_slices)
        one, three = outs[1], outs[3]
        if mode == "sc16":
            assert np.array_equal(one, three), (n_taps, "integer sums: slicing cannot change them")
        else:
            assert np.all(np.max(np.abs(one - three), axis=2) <= bar), (mode, fmt, n_taps, "1 slice against 3 slices")
    bench.report(mode, fmt)


@pytest.mark.parametrize("mode,fmt", M.RESYNC, ids=["%s-%s" % k for k in M.RESYNC])
def test_carrier_resynchronisation_at_chunk_64(bench, oracle, mode, fmt):
    launch = M.resync_launch(oracle, mode, fmt)
    bench.check(launch, bench.batch(launch, 1), "resync")
    bench.report(mode, fmt)


@pytest.mark.parametrize("mode,fmt,n_taps", M.TABLE_PATHS, ids=["%s-%s-%d" % k for k in M.TABLE_PATHS])
def test_launch_with_less_lds_than_the_code_table(bench, oracle, mode, fmt, n_taps):
    """(test_open_loop_matrix_inputs.py asserts, through the launch plan, that the LDS is below the table and which record goes where.)"""
    launch = M.table_launch(oracle, mode, fmt, n_taps)
    bench.check(launch, bench.batch(launch, 2), "table paths")
    bench.report(mode, fmt)


@pytest.mark.parametrize("mode,fmt", M.TINY, ids=["%s-%s" % k for k in M.TINY])
def test_tiny_code_window_wraps_more_than_twice(bench, oracle, mode, fmt):
    launch = M.tiny_launch(oracle, mode, fmt)
    bench.check(launch, bench.batch(launch, 1), "tiny code")


@pytest.mark.parametrize("mode", M.LEVEL1_MODES)
def test_level1_objects_every_tap_count(bench, gctx, oracle, mode):
    import gnsscorr
    cls = {"complex": gnsscorr.HipMulticorrelator, "sc16": gnsscorr.HipMulticorrelator16sc}.get(mode, gnsscorr.HipMulticorrelatorRealCodes)
    for n_taps in M.TAPS:
        mc = cls(gctx)
        if cls is gnsscorr.HipMulticorrelatorRealCodes:
            mc.set_high_dynamics_resampler(mode in M.HD)
        mc.init(M.N_CLEAN, n_taps)
        for n in M.LEVEL1_N:
            launch = M.level1_call(oracle, mode, n_taps, n)
            r = launch.recs[0][0]
            q, clean = M.samples(oracle, "clean", M.stream_fmt(launch))
            base = q if mode == "sc16" else clean
            assert base.ctypes.data % 16 == 0 and r.offset == 1  # the view starts at an odd sample of an aligned array
            shifts, a = launch.shifts.copy(), r.args
            outs = []
            for _ in range(2):
                out = np.zeros((n_taps, 2), np.int16) if mode == "sc16" else np.zeros(n_taps, np.complex64)
                mc.set_local_code_and_taps(launch.code_len, launch.codes[0], shifts)
                mc.set_input_output_vectors(out, base[r.offset:])
                if mode in ("complex", "sc16"):
                    mc.Carrier_wipeoff_multicorrelator_resampler(a["rem_carr"], a["pstep"], a["rem_code"], a["cstep"], n)
                elif mode == "hd_resampler":  # the 6-argument overload with the flag set
                    mc.Carrier_wipeoff_multicorrelator_resampler(a["rem_carr"], a["pstep"], a["rem_code"], a["cstep"], a["crate"], n)
                else:
                    mc.Carrier_wipeoff_multicorrelator_resampler(a["rem_carr"], a["pstep"], a["prate"], a["rem_code"], a["cstep"], a["crate"], n)
                outs.append(out)
            assert outs[0].tobytes() == outs[1].tobytes(), (mode, n_taps, n, "two calls differ")
            bench.check(launch, outs[0][None, None], "level 1, N = %d" % n)
        mc.free()
        mc.close()
    bench.report(mode, "i16" if mode == "sc16" else "f32")
