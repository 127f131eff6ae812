/*
 * pggan_hip_prd.h — C-ABI of the k-NN-ball half of libpggan_hip.so (csrc/prd.hip): improved precision and recall (Kynkaanniemi et
 * al. 2019) and density and coverage (Naeem et al. 2020) between two sets of uint8 images, in pixel space.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.PRD_SIGNATURES / PRD_CONSTANTS); the wrappers are ops.prd_kth_u8 / prd_ball_u8.
 *
 * Definition (restated for the CPU in tests/prd_ref.py).  Integer arithmetic throughout: exact, independent of
 * the order of the sums, the same bits from run to run.
 *   images      uint8 vectors of D = C r^2 bytes, D a multiple of 16;  d2(x, y) = sum_d (x_d - y_d)^2 in int64;
 *   radius      for a set X of N >= k + 1 images, rad_k(X)[i] = the k-th smallest of { d2(X[i], X[j]) : j != i }.  The exclusion is
 *               by INDEX, not by value: a duplicate of image i at another index counts, with distance 0.  1 <= k <= PG_NN_MAX_TOPK;
 *   inside      probe p is inside the ball of centre c iff d2(p, c) <= rad[c]: a probe on the boundary is inside.
 * With reals R (Nr) and fakes G (Ng):
 *   precision = #{g : g inside at least one real ball} / Ng            (radii rad_k(R))
 *   density   = sum_g #{real balls g is inside} / (k Ng)
 *   coverage  = #{r : the ball of r holds at least one fake} / Nr
 *   recall    = #{r : r inside at least one fake ball} / Nr              (radii rad_k(G))
 */
#ifndef PGGAN_HIP_PRD_H
#define PGGAN_HIP_PRD_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Columns of one candidate block of pg_prd_kth_u8 (and both sides of a workgroup's tile). */
#define PG_PRD_TILE 128

/* Both entry points run one tile kernel: a workgroup owns PG_PRD_TILE rows x PG_PRD_TILE columns of the pair matrix, walks ALL of D
 * with both operands staged through LDS (no split of D: the epilogue needs the complete distance) and reduces in its epilogue, so no
 * distance is written to memory.  Rows and columns past the end of a set re-read its last image; their results are neither written
 * nor counted.  16-byte pieces at or past D are never loaded.
 *
 * pg_prd_kth_u8:  x [N][D] uint8; cand [N][G][k] int64, G = ceil(N / PG_PRD_TILE): cand[i][g][.] = the k smallest d2(x[i], x[j]) over
 *                 the columns j of block g (g PG_PRD_TILE <= j < min(N, (g + 1) PG_PRD_TILE)) with j != i, ascending, padded with
 *                 INT64_MAX where the block has fewer than k such columns.  Every element of cand is written; no atomics.
 *                 rad_k(x)[i] is then the k-th value of pg_topk_smallest_i64 over cand read as [N][G k].
 *                 N <= k or k outside 1 .. PG_NN_MAX_TOPK: PG_E_ARG.  D not a multiple of 16, x not 16-byte or cand not 8-byte
 *                 aligned: PG_E_ALIGN.
 * pg_prd_ball_u8: a [Na][D], b [Nb][D] uint8; rad_a [Na], rad_b [Nb] int64 or NULL.  One pass over the Na x Nb pairs (p, c) with
 *                 inside_b = d2(a[p], b[c]) <= rad_b[c] and inside_a = d2(a[p], b[c]) <= rad_a[p]:
 *                     a_cnt[p] = #{c : inside_b}    b_hit[c] = #{p : inside_b}        (int32 [Na], int32 [Nb]; need rad_b)
 *                     b_cnt[c] = #{p : inside_a}    a_hit[p] = #{c : inside_a}        (int32 [Nb], int32 [Na]; need rad_a)
 *                 A NULL radius vector skips its two outputs (their pointers may then be NULL); both NULL is PG_E_ARG.  The call
 *                 zeroes the outputs it writes; a tile adds one 32-bit integer atomic per row and per column with a non-zero count
 *                 (order-independent).  1 <= Na, Nb < 2^31.  Alignment as above, radii 8-byte, outputs 4-byte: PG_E_ALIGN.          */
int pg_prd_kth_u8(const uint8_t* x, int64_t N, int64_t D, int k, int64_t* cand, pg_stream_t stream);
int pg_prd_ball_u8(const uint8_t* a, int64_t Na, const uint8_t* b, int64_t Nb, int64_t D, const int64_t* rad_a, const int64_t* rad_b,
                   int* a_cnt, int* a_hit, int* b_cnt, int* b_hit, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_PRD_H */
