// cond_fir_accum.h -- the accumulation every FIR decimator of the library shares (cond_kernels.hip: from the conditioner's raw ring;
// ring_decim_kernels.hip: from a gc_stream ring).  A tile's inputs lie in LDS in polyphase order -- input i of the tile (i = 0 is
// the oldest, absolute sample m0 D - (T - 1)) at row i % D, column i / D, rows `rowlen` float2 long.  Output j of the tile, tap k
// reads input j D + (T - 1 - k): row (T - 1 - k) % D, the same for every lane, column j + (T - 1 - k) / D, so the 64 lanes of a wave
// read 64 consecutive float2.  Taps come through uniform (scalar) loads.  Every output is h[0] x first, then one fmaf per tap in the
// order k = 1 .. T-1, in float32: its bits are a function of its T inputs and the taps alone, whichever kernel, tile or lane makes it.
#ifndef COND_FIR_ACCUM_H
#define COND_FIR_ACCUM_H
#include <hip/hip_runtime.h>

// rows are an odd number of float2 long: the D rows a wave's samples are written to spread over the banks
static inline int cond_fir_rowlen(int decimation, int n_taps, int tile) { return (tile + (n_taps - 1) / decimation) | 1; }

template <int R>
static __device__ __forceinline__ void cond_fir_accumulate(const float2* lds, const int rowlen, const int D, const int T, const float* taps,
    const int (&j)[R], float2 (&acc)[R])
{
    int row = (T - 1) % D, q = (T - 1) / D;
    {
        const float h = taps[0];
        const float2* p = lds + row * rowlen + q;
#pragma unroll
        for (int r = 0; r < R; r++)
            {
                const float2 x = p[j[r]];
                acc[r] = float2{h * x.x, h * x.y};
            }
    }
    for (int k = 1; k < T; k++)
        {
            if (--row < 0)
                {
                    row = D - 1;
                    q--;
                }
            const float h = taps[k];
            const float2* p = lds + row * rowlen + q;
#pragma unroll
            for (int r = 0; r < R; r++)
                {
                    const float2 x = p[j[r]];
                    acc[r].x = fmaf(h, x.x, acc[r].x);
                    acc[r].y = fmaf(h, x.y, acc[r].y);
                }
        }
}

#endif
