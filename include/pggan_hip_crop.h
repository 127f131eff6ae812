/*
 * pggan_hip_crop.h — C-ABI of the real-image batch cut from device-resident spectrogram STRIPS (csrc/real_batch.hip): a training
 * batch whose images are windows at arbitrary time offsets of recordings of arbitrary length, in one launch.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.CROP_SIGNATURES / CROP_CONSTANTS); the wrapper is ops.crop_batch_u8.
 */
#ifndef PGGAN_HIP_CROP_H
#define PGGAN_HIP_CROP_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* int64 words per strip of the table, and the multiple every byte offset and every row pitch of a level buffer is held to. */
#define PG_CROP_TABLE_WORDS 3
#define PG_CROP_PITCH_ALIGN 16

/* pg_crop_batch_u8:  src is ONE flat uint8 buffer with the strips of one stored level; table [M][PG_CROP_TABLE_WORDS] int64 on the
 *                    device describes strip m as (byte offset, row pitch in bytes, columns), laid out [C][S rows][pitch].  Every
 *                    pitch is a multiple of PG_CROP_PITCH_ALIGN and at least the column count, every offset a multiple of
 *                    PG_CROP_PITCH_ALIGN.  Padding bytes (columns .. pitch of a row) may be read and never influence a result;
 *                    nothing outside [offset, offset + C S pitch) of the addressed strip is read.
 *                    The source window of output image j is columns [u, u + S) of strip idx[j], u = pos[j] >> shift: pos is the
 *                    start column at full resolution, shift = log2(full-resolution columns per stored column).  That S x S window
 *                    is treated exactly as pg_real_batch_u8 (include/pggan_hip.h) treats image idx[j] of a stack [M][C][S][S]:
 *                    pyramid level for depthdiff > 0 (bytes clipped to [min_in, max_in]), mirror of the LEVEL image where
 *                    flip[j] != 0 (flip may be NULL), fade for alpha < 1, range change; fp64 without contraction, rounded once
 *                    to fp32.  Bit-identical to pg_real_batch_u8 / pg_real_batch_2ch_u8 on the same windows materialised as a
 *                    stack [n][C][S][S] with idx = 0 .. n - 1.
 *                    idx [n] int64, pos [n] int64 and flip [n] uint8 on the device; out [n][C][r][r] fp32, r = S >> depthdiff.
 *                    C in {1, 2, 3}, 0 <= shift <= 30 (PG_E_ARG otherwise); S a power of two, r >= 2, 16-byte aligned src and out
 *                    (PG_E_ALIGN otherwise).  One launch, no atomics, nothing allocated, one writer per output element.
 *                    The table and the values of idx and pos are NOT checked on the device: every idx[j] must be in [0, M) and
 *                    every pos[j] >> shift in [0, columns of strip idx[j] - S]. */
int pg_crop_batch_u8(const uint8_t* src, const int64_t* table, int64_t M, int C, int S, int shift, int depthdiff,
                     const int64_t* idx, const int64_t* pos, const uint8_t* flip, int n, float* out,
                     double alpha, double min_in, double max_in, double min_out, double max_out, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_CROP_H */
