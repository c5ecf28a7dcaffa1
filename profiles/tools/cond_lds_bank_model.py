"""Bank behaviour of the LDS writes of the conditioner's real front end (cond_front_real, csrc/cond_kernels.hip), by arithmetic --
a model, not a counter reading; it needs no GPU.  DESIGN.md section 3.3 ("Real IF samples") quotes its table.

A ds_write_b64 of a wave is served 16 consecutive lanes at a time over 32 banks of 4 bytes, so the 16 lanes of a pass are
conflict-free when their float2 indices differ mod 16; k lanes on one bank pair cost k LDS cycles.  Lane l works on the S samples
[S l, S l + S) of the tile (S = samples in a 16-byte vector: 4, 8, 16 or 64) and, at step t, writes tile index
i = S l + (e0(l) + t) % S to float2 index (i % D) * rowlen + i / D, rowlen = (tile + (T - 1) / D) | 1.

  plain:   e0 = 0                                           every lane starts at the first sample of its vector
  skewed:  e0 = l % S (S >= 16), l % 16 * S / 16 (S < 16)   what the kernel does

For every (S, D) the script prints the largest and the mean number of lanes on one bank pair over all passes and steps.

python profiles/tools/cond_lds_bank_model.py [--tile 1024]"""
import argparse
import collections


def ways(U, D, T, tile, skew):
    rowlen = (tile + (T - 1) // D) | 1
    worst, total, passes = 0, 0, 0
    for first in range(0, 64, 16):
        for t in range(U):
            hits = collections.Counter()
            for lane in range(first, first + 16):
                e0 = 0 if not skew else (lane & (U - 1)) if U >= 16 else ((lane & 15) * U) >> 4
                i = lane * U + (e0 + t) % U
                hits[((i % D) * rowlen + i // D) % 16] += 1
            w = max(hits.values())
            worst, total, passes = max(worst, w), total + w, passes + 1
    return worst, total / passes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=1024)
    args = ap.parse_args()
    print("| samples per vector | walk | " + " | ".join("D = %d" % D for D in (1, 2, 4, 5, 8)) + " |")
    print("|---|---|" + "---|" * 5)
    for U in (4, 8, 16, 64):
        for skew in (False, True):
            cells = []
            for D in (1, 2, 4, 5, 8):
                T = 33 if D == 1 else 64
                tile = args.tile
                while D * ((tile + (T - 1) // D) | 1) > 8192:
                    tile //= 2
                worst, mean = ways(U, D, T, tile, skew)
                cells.append("%d (%.2f)" % (worst, mean))
            print("| %d | %s | " % (U, "skewed" if skew else "plain") + " | ".join(cells) + " |")


if __name__ == "__main__":
    main()
