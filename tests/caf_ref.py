"""numpy restatement of the E5a non-coherent I/Q acquisition with CAF filter (galileo_e5a_noncoherent_iq_acquisition_caf_cc.cc:234-282,
:285-333, :461-785) on complex64 input: the yardstick of tests/test_caf_gpu.py.  float32 wipe-off with the oracle's running phase
and float64 transforms (oracle.fft) for the planes; the selection, the keep rule and the CAF filter are the block's, the filter in
float32 step by step.  Both arithmetic modes of the engine: REFERENCE is the block as written (nQB read from the IB plane at :523,
unsigned differences without abs() in three of the filter's six sums), EXACT the block as meant."""
import numpy as np

from quicksync_ref import doppler_bins, wipeoffs  # the same inclusive grid and the same wipe-off rows

REFERENCE, EXACT = 0, 1
F32 = np.float32


def replicas(code_i, code_q, both, hyp, spc):
    """Slots of one satellite in the engine's order IA, QA, IB, QB: B is A with samples [0, spc) negated (:258-280)."""
    out = []
    for h in range(hyp):
        for c in ([code_i, code_q] if both else [code_i]):
            r = np.array(c, np.complex64)
            if h == 1:
                r[:spc] = -r[:spc]
            out.append(r)
    return out


def names(both, hyp):
    return [n for n in ("IA", "QA", "IB", "QB") if (both or n[0] == "I") and (hyp == 2 or n[1] == "A")]


def _weight(wf, d, i, wraps):
    dist = np.uint32((d - i) & 0xFFFFFFFF) if wraps else np.uint32(abs(d - i))
    return F32(1) - wf * F32(dist)


def caf_at(caf_i, caf_q, H, d, arithmetic):
    """CAF[d] (:695-765): float32 running sums in index order, the section's denominator, I part + Q part."""
    n = len(caf_i)
    ref = arithmetic == REFERENCE
    wf = F32(0.5) / F32(H)
    tri = wf * F32(H) * F32(H + 1) / F32(2)
    if d < H:
        lo, hi = 0, H + d + 1
        den = F32(1 + H + d) - tri - wf * F32(d) * F32(d + 1) / F32(2)
        wraps_i, wraps_q = ref, False
    elif d < n - H:
        lo, hi = d - H, d + H + 1
        den = F32(1 + 2 * H) - F32(2) * wf * F32(H) * F32(H + 1) / F32(2)
        wraps_i, wraps_q = ref, ref
    else:
        lo, hi = d - H, n
        r = n - d - 1
        den = F32(1 + H + r) - tri - wf * F32(r) * F32(r + 1) / F32(2)
        wraps_i, wraps_q = False, False
    with np.errstate(over="ignore", invalid="ignore"):
        acc = F32(0)
        for i in range(lo, hi):
            acc = acc + F32(caf_i[i]) * _weight(wf, d, i, wraps_i)
        acc = acc / den
        if caf_q is not None:
            q = F32(0)
            for i in range(lo, hi):
                q = q + F32(caf_q[i]) * _weight(wf, d, i, wraps_q)
            acc = acc + q / den
    return F32(acc)


def caf_filter(caf_i, caf_q, H, arithmetic):
    assert H >= 1 and len(caf_i) >= 2 * H + 1
    return np.array([caf_at(caf_i, caf_q, H, d, arithmetic) for d in range(len(caf_i))], np.float32)


def first_max(v):
    """volk_gnsssdr_32f_index_max_32u: the first maximum; NaN never wins."""
    v = np.asarray(v)
    if np.all(np.isnan(v)):
        return 0
    return int(np.nanargmax(v))


class Dwell:
    """What one dwell leaves: planes {name: [bins][N]}, choice [bins] (bit 0: I took B, bit 1: Q took B), margins [(bin, 'I' | 'Q',
    |nXA - nXB| / max)], caf_i, caf_q, caf (zeros without a filter), caf_margin, grid [bins][N], row_max [(value, index)], mag (d_mag),
    input_power, test_statistics (the kept statistic), indext, doppler_index, doppler_hz, acq_delay_samples, and cell = (indext,
    doppler_index) of d_mag in THIS dwell (None when no cell won)."""


def search(oracle, x, codes, fs, N, doppler_max, doppler_step, both, hyp, window_hz=0, arithmetic=REFERENCE, samples_per_code=None,
        bit_transition=False, n_dwells=1):
    """n_dwells consecutive blocks of N samples of x for every (code_i, code_q) in `codes` (N samples each; code_q None without
    `both`).  Returns a list (per satellite) of lists (per dwell) of Dwell."""
    spc = int(samples_per_code if samples_per_code is not None else N)
    bins = doppler_bins(doppler_max, doppler_step)
    assert doppler_step > 0
    w = wipeoffs(oracle, fs, bins, N)
    fnf = F32(N) * F32(N)
    fnf4 = fnf * fnf
    H = window_hz // (2 * doppler_step)
    nm = names(both, hyp)
    X, power = [], []
    for d in range(n_dwells):
        xb = np.ascontiguousarray(x[d * N:(d + 1) * N], np.complex64)
        assert xb.size == N
        power.append(float(np.mean(np.abs(xb.astype(np.complex128)) ** 2)))
        X.append([oracle.fft((xb * wb).astype(np.complex64)) for wb in w])
    out = []
    for code_i, code_q in codes:
        reps = replicas(code_i[:N], None if code_q is None else code_q[:N], both, hyp, spc)
        Cs = [np.conj(oracle.fft(r)) for r in reps]
        recs = []
        kept = F32(0)
        last = (0, 0, 0, 0)
        for d in range(n_dwells):
            r = Dwell()
            r.planes = {n: np.stack([np.abs(oracle.fft(Xb * C, inverse=True)) ** 2 for Xb in X[d]]) for n, C in zip(nm, Cs)}
            r.choice, r.margins = np.zeros(len(bins), np.uint8), []
            r.caf_i, r.caf_q = np.zeros(len(bins), np.float32), np.zeros(len(bins), np.float32)
            grid = np.zeros((len(bins), N))
            for b in range(len(bins)):
                k = {n: first_max(r.planes[n][b]) for n in nm}
                m = {n: F32(r.planes[n][b][k[n]]) for n in nm}
                nrm = {n: m[n] / fnf4 for n in nm}
                if "QB" in nm and arithmetic == REFERENCE:
                    nrm["QB"] = F32(r.planes["IB"][b][k["QB"]]) / fnf4  # :523
                pick_i, pick_q = "IA", "QA"
                if hyp == 2:
                    if not nrm["IA"] >= nrm["IB"]:
                        pick_i = "IB"
                        r.choice[b] |= 1
                    r.margins.append((b, "I", float(abs(nrm["IA"] - nrm["IB"]) / max(nrm["IA"], nrm["IB"]))))
                    if both:
                        if not nrm["QA"] >= nrm["QB"]:
                            pick_q = "QB"
                            r.choice[b] |= 2
                        r.margins.append((b, "Q", float(abs(nrm["QA"] - nrm["QB"]) / max(nrm["QA"], nrm["QB"]))))
                r.caf_i[b] = m[pick_i]
                row = r.planes[pick_i][b]
                if both:
                    r.caf_q[b] = m[pick_q]  # QB's own maximum under REFERENCE as well (:560)
                    row = row + r.planes[pick_q][b]
                grid[b] = row
            r.grid = grid
            r.row_max = []
            mag, cell = F32(0), None
            for b, row in enumerate(grid):
                k = first_max(row)
                r.row_max.append((float(row[k]), k))
                magt = F32(row[k]) / fnf4
                if mag < magt:
                    mag, cell = magt, (k, b)
            r.cell = cell
            r.input_power = power[d]
            if cell is not None:
                stat = mag / F32(power[d])
                if not bit_transition or kept < stat:
                    kept = stat
                    last = (cell[0], cell[1], bins[cell[1]], cell[0] % spc)
            r.mag = float(mag)
            r.test_statistics = float(kept)
            r.indext, r.doppler_index, r.doppler_hz, r.acq_delay_samples = last
            r.caf = np.zeros(len(bins), np.float32)
            r.caf_margin = None
            if H > 0:
                r.caf = caf_filter(r.caf_i, r.caf_q if both else None, H, arithmetic)
                d_caf = first_max(r.caf)
                top = np.sort(r.caf[~np.isnan(r.caf)].astype(np.float64))[-2:]
                r.caf_margin = float((top[1] - top[0]) / abs(top[1])) if top.size == 2 and top[1] != 0 else 0.0
                r.doppler_index, r.doppler_hz = d_caf, bins[d_caf]  # :768-770, in every dwell
            recs.append(r)
        out.append(recs)
    return out
