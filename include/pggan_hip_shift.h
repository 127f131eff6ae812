/*
 * pggan_hip_shift.h — C-ABI of the shift-invariant nearest-window search over device-resident spectrogram STRIPS
 * (csrc/shift_search.hip): for every query and every segment of start columns, the smallest exact squared L2 distance between the
 * query and the S x S windows at EVERY start column of the segment, and where it is -- without the per-start distances ever
 * existing in memory.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged, and the
 * strips are those of include/pggan_hip_crop.h (one flat buffer, a table of PG_CROP_TABLE_WORDS int64 per strip, pitches and
 * offsets held to PG_CROP_PITCH_ALIGN).  The binding parses this header into tables of its own (_lib.SHIFT_SIGNATURES /
 * SHIFT_CONSTANTS); the wrapper is ops.shift_l2min_u8.
 */
#ifndef PGGAN_HIP_SHIFT_H
#define PGGAN_HIP_SHIFT_H

#include "pggan_hip.h"
#include "pggan_hip_crop.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bits of a key below the distance: the start column relative to its segment.  A segment holds at most 1 << PG_SHIFT_POS_BITS starts. */
#define PG_SHIFT_POS_BITS 16
/* Queries of one pass over the strips (as PG_NN_MAX_QUERIES). */
#define PG_SHIFT_MAX_QUERIES 64
/* Consecutive start columns of one strip that a workgroup owns: the unit of the grid mapping in `segtab`. */
#define PG_SHIFT_TILE 128
/* int64 words per strip of `segtab`: (first segment of the strip, first tile of the strip). */
#define PG_SHIFT_SEGTAB_WORDS 2

/* pg_shift_l2min_u8:  src / table [M][PG_CROP_TABLE_WORDS] are one stored level of strips as pg_crop_batch_u8 takes them: strip m is
 *                     (byte offset, row pitch, columns T_m >= S), laid out [C][S rows][pitch].  queries [K][C][S][S] uint8.
 *                         d[k, m, u] = sum_{c, r, j} (strip_m[c, r, u + j] - q_k[c, r, j])^2        u = 0 .. T_m - S    (exact)
 *                     The starts of a strip are cut into segments of `seg` consecutive starts; segment g of strip m covers
 *                     u in [g seg, min((g + 1) seg, T_m - S + 1)), segments are numbered strip-major, G in all.
 *                         key[k][g] = min_u ( d[k, m, u] << PG_SHIFT_POS_BITS  |  u - g seg )
 *                     so the minimum is by (distance, start): of equal distances the lower start wins.
 *                     segtab [M + 1][PG_SHIFT_SEGTAB_WORDS] int64 on the device: (first segment, first tile) of strip m, a tile being
 *                     PG_SHIFT_TILE consecutive starts of one strip; row M holds (G, tiles).  `tiles` and `G` repeat row M for the
 *                     host.  key [K][G] int64 is preset here and every element is written.
 *                     C in {1, 2, 3}, S a power of two in 4 .. 1024, 1 <= K <= PG_SHIFT_MAX_QUERIES, 1 <= seg <= 1 << PG_SHIFT_POS_BITS
 *                     (PG_E_ARG otherwise); src and queries 16-byte aligned, table, segtab and key 8-byte aligned (PG_E_ALIGN
 *                     otherwise).  Padding bytes (columns .. pitch of a row) may be read and never influence a result; nothing outside
 *                     [offset, offset + C S pitch) of the addressed strip is read.  Nothing is allocated.  The tiles of a segment
 *                     combine with a 64-bit integer atomic minimum: the result does not depend on the order and is the same bits
 *                     from run to run.  The tables are NOT checked on the device. */
int pg_shift_l2min_u8(const uint8_t* src, const int64_t* table, int64_t M, int C, int S, const uint8_t* queries, int K, int seg,
                      const int64_t* segtab, int64_t tiles, int64_t G, int64_t* key, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_SHIFT_H */
