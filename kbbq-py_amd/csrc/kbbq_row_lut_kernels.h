// kbbq_row_lut_kernels.h -- the int8 LUTs K2 stages for the rows of one launch, written from the canonical int16 LUT in front of it:
// narrowed to a pitch (one read per row) and the mate-pair form (their geometry is K2's and the host's: kbbq_kernels_v3.h).
#pragma once
#include "kbbq_kernels_v3.h"

// The full LUT narrowed to the cycle columns rows of one pitch can reach (K2 on one-read-per-row planes): a read in a
// row of `pitch` bytes has at most Sb = min(pitch, S2) bases, so of a model row's S2 cycle entries only [0, Sb) (first
// in pair) and [S2 - Sb, S2) (second in pair: column S2 - 1 - pos) are ever indexed.  Same geometry as the full LUT with
// Sb in place of S2 (full_lut_width / full_lut_row_bytes): W = Sb + 16, [0, W) forward, [W, 2W) mirrored, 25 contexts at
// 2W.  A length band of a mixed-length input (tables of 600 columns, rows of 48 bytes) stages 12 KB instead of 96 KB:
// the LDS then holds several workgroups per CU again, and the short-lived K2 (kbbq_k2_tile.h) can afford the staging.
struct RowLutParams { const int16_t* lut16; int rs16; int R; int Qt; int S2; int Sb; int minscore; int8_t* out; };

__global__ __launch_bounds__(256) void k3_fill_row_lut(RowLutParams p)
{
    const int rb = full_lut_row_bytes(p.Sb), W = full_lut_width(p.Sb);
    const int NR = 33 + p.Qt;
    const int row = blockIdx.x;                       // r * NR + qb
    const int r = row / NR, qb = row - r * NR;
    const bool model = qb >= 33 + p.minscore;
    const int16_t* src = p.lut16 + ((size_t)r * p.Qt + (qb >= 33 ? qb - 33 : 0)) * p.rs16;
    int8_t* dst = p.out + (size_t)row * rb;
    for (int x = threadIdx.x; x < rb; x += blockDim.x) {
        int v = 0;
        if (!model) {
            if (x < 2 * W) v = qb == 0 ? -33 : qb - 33;                   // padding -> 0 ; uncounted -> unchanged
        } else {
            if (x < p.Sb) v = src[x];
            else if (x >= W && x < W + p.Sb) v = src[p.S2 - 1 - (x - W)];   // second in pair: column S2 - 1 - pos
            else if (x >= 2 * W && x < 2 * W + 25) v = src[p.S2 + (x - 2 * W)];
        }
        dst[x] = (int8_t)v;                            // the blob's flags said every value fits (FAST mode only)
    }
}

struct PairLutParams {
    const int16_t* lut16; int rs16; int R; int Qt; int S2; int minscore;
    int twins;                       // rows of two first-in-pair reads: the second half looks up the forward columns too
    int8_t* out;
};

// one workgroup per row (read group, raw quality byte) of the pair LUT
__global__ __launch_bounds__(256) void k3_fill_pair_lut(PairLutParams p)
{
    const int rb = pair_lut_row_bytes(p.S2), cyc = pair_pitch(p.S2), S = p.S2 >> 1;
    const int NR = 33 + p.Qt;
    const int row = blockIdx.x;
    const int r = row / NR, qb = row - r * NR;
    const bool model = qb >= 33 + p.minscore;
    const int16_t* src = p.lut16 + ((size_t)r * p.Qt + (qb >= 33 ? qb - 33 : 0)) * p.rs16;
    int8_t* dst = p.out + (size_t)row * rb;
    for (int x = threadIdx.x; x < rb; x += blockDim.x) {
        int v = 0;
        if (!model) {
            if (x < cyc) v = qb == 0 ? -33 : qb - 33;                     // padding -> 0 ; uncounted -> unchanged
        } else {
            if (x < S) v = src[x];                                        // mate 1: column = position
            else if (x > S && x <= p.S2) v = src[p.twins ? x - S - 1 : p.S2 - 1 - (x - S - 1)]; // mate 2, position i = x-S-1: column 2S-1-i (twins: i)
            else if (x >= cyc && x < cyc + 25) v = src[p.S2 + (x - cyc)];
        }
        dst[x] = (int8_t)v;
    }
}
