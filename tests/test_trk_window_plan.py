"""CPU tests of the multicorrelator's window plan (gnss-sdr-1_amd/csrc/trk_window_plan.h): what trk_epoch / trk_loop decide from
integers and the code NCO's scalars -- the chunks of a (window, slice), which of them may be fetched whole, the samples and chips a
slice touches and where the loop finds them.  tests/trk_window_plan_selftest.cpp compiles the header the kernels include with g++
(-ffp-contract=off, like the kernels).

The sweep: N 0..1100, a 0..15, 1..4 slices, the window 0, 1, 5, 15, 16 or 600 samples into the buffer, 0, 1, 511, 512, 513 or 100000
samples of it behind the window, plain buffers and rings, chunks of 512.  Conditions, not measurements:
  * the slices' [c0, c1) partition [0, n_chunks) in order (a slice past the last chunk is empty);
  * every sample n of [0, N) lies in exactly one chunk, at v = n + a;
  * a chunk is full exactly when all 512 of its positions lie in [a, V);
  * a chunk that loadable() admits and that is not full lies in the buffer: off - a + c * 512 >= 0 and off - a + (c + 1) * 512 <= end
    -- the memory safety of the whole-chunk fetch of a window's ragged ends;
  * without WHOLE, loadable() is chunk_is_full();
  * n_lo <= n_hi, both in [0, max(N - 1, 0)] for every slice that has chunks (a slice without chunks runs no loop; the formulas give
    it n_lo = n_hi = c0 * 512 - a, past the window) and, in the high-dynamics form, for every slice.

The header states trk_epoch's formulas; the kernels call its chip-index helpers and take lc0 / lc1 from it (trk_whole_first /
trk_whole_end, which the swept trk_chunk_plan calls too), and trk_epoch keeps its own copy of the rest (calling all of the header
from it moved the closed-loop kernels' register allocation: DESIGN.md 3.1).  So three statements exist -- trk_epoch, this
header, epoch_path -- held together by this test and, for trk_epoch, by the device results of test_open_loop_matrix_gpu.py.
The restatement: tests/open_loop_matrix_cases.py::epoch_path states the same decisions independently, in Python, and
test_open_loop_matrix_inputs.py asserts with it that every window of the matrix takes the branch it is there for.  Here every record
of every launch of that file, at every slicing its tests use, gives the same a, n_chunks, full[], lc0, lc1 and per slice c0, c1 and
table path through the compiled header."""
import os
import subprocess

import pytest

import open_loop_matrix_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build(directory, flags):
    exe = os.path.join(str(directory), "trk_window_plan_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-Wextra", "-ffp-contract=off"] + flags + ["-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"),
        os.path.join(ROOT, "tests", "trk_window_plan_selftest.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_sweep_of_the_chunk_geometry(tmp_path_factory, flags):
    exe = build(tmp_path_factory.mktemp("trk_window_plan"), flags)
    out = subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    # 2 buffer kinds x 6 offsets x 6 tails x 1101 lengths x 16 alignments x (1 + 2 + 3 + 4) slices, less the ring of no samples
    assert out.stdout.split() == ["sweep", "ok", str(2 * 6 * 6 * 1101 * 16 * 10 - 16 * 10)]


def _launches(oracle):
    yield from M.all_float_launches(oracle)
    for t in M.TAPS:
        yield M.matrix_launch(oracle, "sc16", "i16", t)
        for n in M.LEVEL1_N:
            yield M.level1_call(oracle, "sc16", t, n)
    yield M.resync_launch(oracle, "sc16", "i16")


def test_python_restatement_equals_the_compiled_header(oracle, tmp_path_factory):
    directory = tmp_path_factory.mktemp("trk_window_plan_records")
    exe, plan_exe = build(directory, []), M.build_selftest(directory)
    lines, want, tables = [], [], set()
    for launch in _launches(oracle):
        words = 2 if launch.mode == "complex" else 1
        level1 = launch.table == "level1"
        for n_slices in launch.slicings:
            # a level-1 call: its own launch, the 16-byte chunk grid, the whole table's worth of LDS
            lds = words * (launch.max_code_len + M.LDS_MARGIN) if level1 else M.plan(plan_exe, launch, n_slices)[1]
            align = 2 if level1 else M.ALIGN
            for ch, recs in enumerate(launch.recs):
                for k, r in enumerate(recs):
                    p = r.params
                    # the allocation is aligned to the chunk grid: the address of the first sample, in samples, is bind + offset
                    lines.append(" ".join(["%d" % v for v in (launch.n_taps, launch.mode in M.HD, words, lds, launch.code_len, launch.binds[ch] + r.offset,
                        align // 2, r.offset, launch.n_iq[ch], 0, r.n, n_slices)] + ["%.9g" % float(v) for v in (p.code_phase_step_chips, p.rem_code_phase_chips,
                        p.code_phase_rate_step_chips) + tuple(launch.shifts)]))
                    want.append((launch.table, launch.mode, launch.fmt, launch.n_taps, ch, k, n_slices, M.epoch_path(launch, ch, k, n_slices, lds, align=align)))
                    tables.add(launch.table)
    assert tables == {"matrix", "resync", "table", "tiny", "level1"} and len(lines) > 3000
    out = subprocess.run([exe, "records"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(want)
    seen = set()
    for line, w in zip(got, want):
        f, p = line.split(), w[-1]
        have = dict(a=int(f[0]), n_chunks=int(f[1]), lc0=int(f[2]), lc1=int(f[3]), full=[] if f[4] == "-" else [c == "1" for c in f[4]],
            slices=[(int(s.split(":")[0]), int(s.split(":")[1]), s.split(":")[2]) for s in f[5:]])
        assert have == p, (w[:-1], have, p)
        seen |= {s[2] for s in have["slices"]}
    assert seen == {"window", "window_mod", "lds_table", "global_table", "none"}  # every path an open-loop launch can take
