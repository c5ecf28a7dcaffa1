"""The acquisition planner in Python: which kernel instances an FFT size runs (gnss-sdr-1_amd/csrc/acq_plan.h: acq_plan_make and
the row-kernel choice acq_rows_plan_make), and the size matrix of tests/test_acquisition_matrix_gpu.py.

tests/test_acq_plan.py holds plan(), row_kernel() and the two lists to the compiled planner (tests/acq_plan_selftest.cpp) and
guards what MATRIX covers."""

ACQ_THREADS = 256
ACQ_MAX_FACTORS = 12
LDS_LIMIT_BYTES = 160 * 1024      # gc_acq_create
ACQ_ROWS2_POINTS = 20
ACQ_ROWS2_LDS_BYTES = 40000
N1_CANDIDATES = (1, 2, 3, 4, 5, 6, 8, 9, 10, 12, 15, 16, 20, 25, 32, 40, 50)  # the instantiated column sizes (ACQ_N1_LIST)

# ACQ_ROWS2_LIST: the instantiated stage lists of the packed row kernel as (radix, butterflies per thread)
ROWS2_REGISTRY = (
    ((10, 2), (10, 2), (10, 2)),
    ((10, 1), (10, 1), (10, 1)),
    ((16, 1), (16, 1), (4, 4)),
    ((10, 2), (5, 4), (5, 4), (5, 4)),
    ((16, 1), (16, 1), (5, 4)),
    ((16, 1), (16, 1), (8, 2)),
    ((16, 1), (10, 2), (10, 2)),
    ((16, 1), (5, 4), (5, 4), (5, 4)),
    ((16, 1), (16, 1), (10, 1)),
    ((16, 1), (16, 1), (16, 1)),
    ((16, 1), (10, 2), (5, 4), (5, 4)),
    ((16, 1), (10, 2), (3, 4), (2, 8)),
    ((16, 1), (10, 2), (10, 2), (2, 8)),
)
GENERAL_ROWS = "general"  # acq_rows_kernel: any radix, one row per workgroup


def factor_rows(n2):
    """Radices of the N2-point row FFT in stage order, or None (more than ACQ_MAX_FACTORS stages)."""
    n, fac = n2, []
    while n > 1:
        r = 0
        for p in (16, 10, 8, 5, 4, 3, 2):
            if n % p == 0:
                r = p
                break
        if not r:
            p = 7
            while p * p <= n:
                if n % p == 0:
                    r = p
                    break
                p += 2
            if not r:
                r = n
        if len(fac) >= ACQ_MAX_FACTORS:
            return None
        fac.append(r)
        n //= r
    return fac


def cols_perm_map(n1, n2, n_xblk):
    """acq_cols_perm_map: whether the forward epilogues take columns N1 j + r and store runs of 256 / N1 elements."""
    pj = ACQ_THREADS // n1
    return n1 > 1 and pj >= 4 and n2 % (n1 * pj) == 0 and n_xblk * (n1 * pj) == n2


def plan(n, lds_limit_bytes=LDS_LIMIT_BYTES):
    """acq_plan_make: (N1, N2, radices, perm_map) or None."""
    if n < 1:
        return None
    best, best_cost = 0, -1
    for n1 in N1_CANDIDATES:
        if n % n1:
            continue
        n2 = n // n1
        if 2 * n2 * 8 > lds_limit_bytes:
            continue
        if factor_rows(n2) is None:
            continue
        cost = abs(n2 - 1024)
        if best_cost < 0 or cost < best_cost:
            best_cost, best = cost, n1
    if not best:
        return None
    n2 = n // best
    n_xblk = (n2 + ACQ_THREADS - 1) // ACQ_THREADS  # acq_cols_blocks
    return best, n2, factor_rows(n2), cols_perm_map(best, n2, n_xblk)


def rows2_config(n2, fac, rpw_cap=0):
    """acq_rows2_config: (rows per workgroup, butterflies per thread of every stage) or None.  rpw_cap: the experiment build's cap."""
    if any(r not in (2, 3, 4, 5, 8, 10, 16) for r in fac):
        return None
    if n2 * 8 > 64 * 1024:
        return None
    rpw = min(max(ACQ_ROWS2_LDS_BYTES // (n2 * 8), 1), 16)
    if rpw_cap > 0:
        rpw = min(rpw, rpw_cap)
    while rpw >= 1:
        iters = []
        for r in fac:
            need = (rpw * (n2 // r) + ACQ_THREADS - 1) // ACQ_THREADS
            it = 1
            while it < need:
                it *= 2
            if it * r > ACQ_ROWS2_POINTS or it > 8:
                break
            iters.append(it)
        else:
            return rpw, iters
        rpw -= 1
    return None


def row_kernel(n, rpw_cap=0):
    """The row kernel acq_rows_plan_make picks for FFT size n: an entry of ROWS2_REGISTRY, or GENERAL_ROWS."""
    _, n2, fac, _ = plan(n)
    cfg = rows2_config(n2, fac, rpw_cap) if len(fac) <= 4 else None
    if cfg:
        stages = tuple(zip(fac, cfg[1]))
        if stages in ROWS2_REGISTRY:
            return stages
    return GENERAL_ROWS


# N1 -> (sizes stored with the plain column mapping, sizes stored with perm_map); every size at most 64000 samples
MATRIX = {
    1: ((1024, 1023), ()),
    2: ((2046,), (2048,)),
    3: ((3000, 3072), (3060,)),
    4: ((4000,), (4096,)),
    5: ((5000,), (5100,)),
    6: ((6000, 6138), (6048,)),
    8: ((8000,), (8192,)),
    9: ((9000, 9216), (9072,)),
    10: ((10230, 10240), (10000,)),
    12: ((12000,), (12096,)),
    15: ((15000, 18750), (15300,)),
    16: ((16000, 16368), (16384,)),
    20: ((20000, 20460), (19200,)),
    25: ((24000,), (25000, 31250)),
    32: ((32000,), (32768,)),
    40: ((40000,), (38400,)),
    50: ((64000,), (50000, 62500)),
}
MATRIX_MAX_N = 64000
MATRIX_SIZES = tuple(sorted(n for plain, perm in MATRIX.values() for n in plain + perm))
# one size per N1 for the dwell epilogues: the first plain-mapping one, the perm_map one where there is none
DWELL_SIZES = tuple((plain + perm)[0] for plain, perm in MATRIX.values())
# The stage lists of the packed row kernel that no size up to MATRIX_MAX_N reaches: rows of 1600 to 4096 points under the 50-point
# column pass.  65536 / 80000 / 100000 are sizes tests/test_acquisition_gpu.py runs as well; the other four run nowhere else
LONG_ROW_SIZES = (65536, 80000, 100000, 128000, 131072, 160000, 200000)
# (10, 1) x 3 is the 1000-point list at no more than 2 rows per workgroup: acq_rows2_config starts at 5 rows, which fit, so only
# the experiment build's cap on the rows per workgroup can select it
ROWS2_UNREACHABLE = (((10, 1), (10, 1), (10, 1)),)
# the sizes tests/test_acquisition_gpu.py searches (known answers, bit-transition, the size list, the GLONASS capture)
EXISTING_SIZES = (4000, 16000, 25000, 6625, 8000, 2048, 5456, 6250, 8184, 12000, 24000, 30000, 32000, 32768, 40000, 50000, 64000, 65536,
    80000, 100000, 256000, 400000)
