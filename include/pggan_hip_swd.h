/*
 * pggan_hip_swd.h — C-ABI of the sliced Wasserstein distance for C = 1 .. PG_SWD_MAX_CHANNELS image channels (csrc/swd.hip): the
 * descriptor side of the metric -- gather, per-channel statistics, normalisation, projection -- with the channel count as an argument.
 * The pyramid (pg_lap_down / pg_lap_up_sub), the sort (pg_swd_sort_rows) and the L1 (pg_swd_l1) of include/pggan_hip.h never see a
 * channel and serve every C as they are.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.SWD_SIGNATURES / SWD_CONSTANTS); the wrappers are ops.swd_gather_c,
 * ops.swd_normalize_c_ and ops.swd_project_c.
 *
 * A descriptor is the C x 7 x 7 neighbourhood of a pyramid level around a centre: PG_SWD_PATCH * C floats (49, 98, 147, 196) in
 * (channel, dy, dx) order.  With C = 3 every entry point here runs the kernel instantiation that its namesake without the suffix in
 * include/pggan_hip.h runs (PG_SWD_DESC = 147): the results are equal bit for bit.  C outside 1 .. PG_SWD_MAX_CHANNELS is PG_E_ARG.
 * No atomics, nothing allocated, one writer per output element.
 */
#ifndef PGGAN_HIP_SWD_H
#define PGGAN_HIP_SWD_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* floats of one channel of a descriptor (7 x 7), and the most channels a descriptor has */
#define PG_SWD_PATCH 49
#define PG_SWD_MAX_CHANNELS 4

/* pg_swd_gather_c:  level [ndesc / P][C][S][S], centres [ndesc][2] int32 of (x, y) -> rows row_offset .. row_offset + ndesc of
 *                   out [out_rows][PG_SWD_PATCH * C]; descriptor j belongs to image j / P.  Centres are clamped to [3, S - 4] on the
 *                   device, so no read leaves the level.  S >= 7, 0 <= row_offset, row_offset + ndesc <= out_rows (PG_E_ARG). */
int pg_swd_gather_c(const float* level, const int32_t* centres, float* out, int64_t ndesc, int P, int C, int S,
                    int64_t row_offset, int64_t out_rows, pg_stream_t stream);

/* pg_swd_channel_stats_c:  desc [M][PG_SWD_PATCH * C] -> stats [2 C]: the C means, then the C population standard deviations, of
 *                          every channel over all M * PG_SWD_PATCH of its values (fp64 sums, two stages, no atomics).
 *                          partials: PG_SWD_REDUCE_BLOCKS * 2 C doubles of scratch. */
int pg_swd_channel_stats_c(const float* desc, int64_t M, int C, double* partials, float* stats, pg_stream_t stream);

/* pg_swd_normalize_c:  desc[m][c][.] = (desc[m][c][.] - stats[c]) / stats[C + c], in place. */
int pg_swd_normalize_c(float* desc, int64_t M, int C, const float* stats, pg_stream_t stream);

/* pg_swd_project_c:  out [K][M] = (desc [M][PG_SWD_PATCH * C] x dirs [PG_SWD_PATCH * C][K]) transposed, fp32 on
 *                    v_mfma_f32_32x32x2_f32 (an odd descriptor length is padded with one zero on both operands).
 *                    PG_E_UNSUP when K > 65535 * 128. */
int pg_swd_project_c(const float* desc, const float* dirs, float* out, int64_t M, int C, int K, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_SWD_H */
