/*
 * pggan_hip_cluster.h — C-ABI of the k-means half of libpggan_hip.so (csrc/cluster.hip): the bins of NDB/k and its JS divergence
 * (Richardson & Weiss 2018, "On GANs and GMMs"), fitted over the uint8 image stack that DeviceImageDataset keeps in HBM.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.CLUSTER_SIGNATURES / CLUSTER_CONSTANTS); the wrappers are in cluster.py.
 *
 * Definition (restated for the CPU in tests/ndb_ref.py).  Integer arithmetic throughout: exact, independent of
 * the order of the sums, the same bits from run to run.
 *   data        X [M][D] uint8, D = C r^2 a multiple of 16 (pg_l2dist_u8's contract), 1 <= M <= PG_CLUSTER_MAX_IMAGES,
 *               centroids c [K][D] uint8, 2 <= K <= PG_NN_MAX_QUERIES;
 *   assignment  label[m] = argmin_k sum_d (X[m][d] - c[k][d])^2 ; of equal distances the LOWER k wins (two equal centroids leave
 *               the higher one empty): pg_l2dist_u8 followed by pg_cluster_argmin_i64;
 *   update      over the members of bin k (the fit set; held-out images are not members), sums[k][d] = sum X[m][d] in int32
 *               (255 * 2^23 < 2^31: the bound on M) and n_k their number;  c[k][d] = (2 sums + n_k) / (2 n_k) rounded down, i.e.
 *               the mean rounded half up, evaluated in 64 bits (2 sums reaches 2^32); a bin with n_k = 0 keeps its centroid.
 */
#ifndef PGGAN_HIP_CLUSTER_H
#define PGGAN_HIP_CLUSTER_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Most images a fit takes: an int32 sum of 2^23 bytes of 255 is 2 139 095 040 < 2^31. */
#define PG_CLUSTER_MAX_IMAGES (1 << 23)

/* pg_cluster_argmin_i64: dist [K][M] int64 as pg_l2dist_u8 writes it -> label [M] int32 = the row of the column's smallest value (the
 *                        lower row of equal values), best [M] int64 = that value.  1 <= K <= PG_NN_MAX_QUERIES, 1 <= M < 2^31
 *                        (PG_E_ARG otherwise).  One thread per column: a wave reads 512 contiguous bytes of every row.  No atomics.
 * pg_cluster_sums_u8:    stack [M][D] uint8; order [n] int32: image indices grouped by bin; offsets [K+1] int32, ascending: the
 *                        members of bin k are order[offsets[k]] .. order[offsets[k+1] - 1].  Entries of order before offsets[0] and
 *                        from offsets[K] on belong to no bin.  sums [K][D] int32, every element written: sums[k][d] = sum over the
 *                        members of stack[order[i]][d].  Every member image's bytes are read once, 16 per load, at the 64-bit offset
 *                        order[i] * D; images that are not members are not read.  A workgroup owns (a slice of up to 1 KiB of D) x
 *                        (one bin) x (one share of the bin's member list); when member lists are shared the call zeroes sums
 *                        and the shares add with 32-bit integer atomics (order-independent), otherwise they store.
 *                        1 <= M <= PG_CLUSTER_MAX_IMAGES, 1 <= n <= M, 1 <= K <= PG_NN_MAX_QUERIES (PG_E_ARG otherwise); D a multiple
 *                        of 16, stack and sums 16-byte aligned (PG_E_ALIGN otherwise).  offsets outside [0, n] are clipped and an
 *                        index outside [0, M) is skipped on the device: nothing outside the stack is read.
 * pg_cluster_centroids_u8: centroids [K][D] uint8 IN PLACE: element (k, d) becomes (2 sums[k][d] + counts[k]) / (2 counts[k]) in
 *                        64-bit integers when counts[k] > 0 and is left as it is otherwise.  counts [K] int64.  sums holds sums of
 *                        counts[k] bytes (a quotient above 255 is stored as 255).  D a multiple of 16, sums and centroids 16-byte
 *                        aligned (PG_E_ALIGN otherwise).  No [K][D] 64-bit temporary exists.                                    */
int pg_cluster_argmin_i64(const int64_t* dist, int K, int64_t M, int* label, int64_t* best, pg_stream_t stream);
int pg_cluster_sums_u8(const uint8_t* stack, int64_t M, int64_t D, const int* order, int64_t n, const int* offsets, int K,
                       int* sums, pg_stream_t stream);
int pg_cluster_centroids_u8(const int* sums, const int64_t* counts, uint8_t* centroids, int K, int64_t D, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_CLUSTER_H */
