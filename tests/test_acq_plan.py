"""CPU tests of the acquisition planner (gnss-sdr-1_amd/csrc/acq_plan.h): the Python restatement tests/acq_plan_ref.py equals the
compiled planner (tests/acq_plan_selftest.cpp) for every FFT size the acquisition suites search, and the size matrix of
tests/test_acquisition_matrix_gpu.py reaches every instance of the column kernel -- 17 column sizes, both store mappings of the
forward epilogues -- and every reachable row kernel.  Which instance a size runs is the planner's choice alone: when its
preferences change, the guard fails and the sizes of acq_plan_ref.MATRIX have to be picked again."""
import os
import subprocess

import pytest

import acq_plan_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(n, rpw_cap=0):
    p = P.plan(n)
    if p is None:
        return "%d none" % n
    n1, n2, fac, perm = p
    rows = P.row_kernel(n, rpw_cap)
    if rows != P.GENERAL_ROWS:
        rows = "%s/%d" % (_stages(rows), P.rows2_config(n2, fac, rpw_cap)[0])
    return "%d %d %d %s %d %s" % (n, n1, n2, "x".join(str(r) for r in fac) or "1", int(perm), rows)


def _stages(stages):
    return ",".join("%dx%d" % ri for ri in stages)


def _run(selftest, *args):
    out = subprocess.run([selftest] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("acq_plan") / "acq_plan_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"),
        os.path.join(ROOT, "tests", "acq_plan_selftest.cpp"), "-o", exe])
    return exe


def test_python_planner_equals_the_compiled_planner(selftest):
    """Every size of the matrix, the long-row sizes, the sizes of test_acquisition_gpu.py, and sizes around them that the planner
    treats differently: no candidate divides (primes), nothing fits the LDS, N = 1, more stages than a plan holds; then every size
    up to the matrix's largest.  Each line carries the row kernel and its rows per workgroup as well."""
    sizes = sorted(set(P.MATRIX_SIZES + P.LONG_ROW_SIZES + P.EXISTING_SIZES + (1, 2, 7, 1000, 10007, 20479, 20483, 10241, 512000, 512050,
        3 ** 13, 2 * 3 ** 12, 999983, 1 << 20)))
    assert _run(selftest, *sizes) == [_line(n) for n in sizes]
    assert _run(selftest, "--range", 1, P.MATRIX_MAX_N) == [_line(n) for n in range(1, P.MATRIX_MAX_N + 1)]


def test_column_sizes_equal_the_source(selftest):
    assert _run(selftest, "--n1") == [str(n1) for n1 in P.N1_CANDIDATES]


def test_registry_data_equals_the_source(selftest):
    assert _run(selftest, "--registry") == [_stages(e) for e in P.ROWS2_REGISTRY]


def test_rows_per_workgroup_cap_selects_the_unreachable_list(selftest):
    """Two rows of 1000 points per workgroup leave a thread one butterfly per stage: the list no uncapped size runs."""
    assert P.row_kernel(25000, 2) == P.ROWS2_UNREACHABLE[0] == ((10, 1), (10, 1), (10, 1))
    assert _run(selftest, "--rpw-cap", 2, 25000) == [_line(25000, 2)] == ["25000 25 1000 10x10x10 1 10x1,10x1,10x1/2"]


def test_matrix_reaches_every_column_kernel_and_both_store_mappings():
    """If this fails the planner (or the matrix) changed: re-pick sizes so that every N1 is run with the plain mapping and, where
    the mapping exists (N1 > 1: 256 / N1 >= 4 for every instantiated N1), with perm_map."""
    assert tuple(P.MATRIX) == P.N1_CANDIDATES and len(P.N1_CANDIDATES) == 17
    for n1, (plain, perm) in P.MATRIX.items():
        assert plain, "no plain-mapping size for N1 = %d" % n1
        assert perm or n1 == 1, "no perm_map size for N1 = %d" % n1
        assert P.ACQ_THREADS // n1 >= 4
        for n in plain + perm:
            assert n <= P.MATRIX_MAX_N
            got = P.plan(n)
            assert got is not None and (got[0], got[3]) == (n1, n in perm), "N = %d runs N1 = %s, perm_map %s: pick another size" % (n, got[0], got[3])
    assert all(not P.cols_perm_map(1, n2, (n2 + 255) // 256) for n2 in (256, 1024, 1023))


def test_matrix_reaches_every_row_kernel():
    """Every entry of ACQ_ROWS2_LIST and the general row kernel: the matrix runs all that a size up to 64000 can reach (checked
    against all of them), LONG_ROW_SIZES the rest, but for the one list the product build cannot select."""
    reached = {P.row_kernel(n) for n in P.MATRIX_SIZES}
    assert P.GENERAL_ROWS in reached
    reachable = {P.row_kernel(n) for n in range(1, P.MATRIX_MAX_N + 1) if P.plan(n)}
    assert reached == reachable, "row kernels the matrix misses: %s" % sorted(map(str, reachable - reached))
    long_rows = {P.row_kernel(n) for n in P.LONG_ROW_SIZES}
    assert reached | long_rows == (set(P.ROWS2_REGISTRY) - set(P.ROWS2_UNREACHABLE)) | {P.GENERAL_ROWS}
    assert not long_rows & reached, "a long-row size runs a kernel the matrix already runs"
    # the unreachable list: only 1000-point rows factor as 10 x 10 x 10, and their configuration is 2 butterflies per thread
    assert P.factor_rows(1000) == [10, 10, 10] and P.rows2_config(1000, [10, 10, 10]) == (5, [2, 2, 2])
    # the general kernel with radices outside the packed kernel's set, as the matrix promises
    primes = {r for n in P.MATRIX_SIZES for r in P.plan(n)[2] if r not in (2, 3, 4, 5, 8, 10, 16)}
    assert primes >= {7, 11, 17, 31}


def test_dwell_sizes_take_one_size_per_column_kernel():
    assert sorted(P.plan(n)[0] for n in P.DWELL_SIZES) == list(P.N1_CANDIDATES)
