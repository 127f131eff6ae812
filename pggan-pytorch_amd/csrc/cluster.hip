// k-means over the uint8 image stack in HBM: the bins of NDB/k (include/pggan_hip_cluster.h).
//   pg_cluster_argmin_i64   : the column argmin of pg_l2dist_u8's [K][M] int64 distances, the lower k of equal values
//   pg_cluster_sums_u8      : per-bin sums of the member images' bytes, the second HBM-bound pass of an iteration
//   pg_cluster_centroids_u8 : the mean rounded half up, in place
// Everything is integer arithmetic: exact, order-independent, the same bits from run to run.
//
// pg_cluster_sums_u8.  An image is D / 16 pieces of 16 bytes.  A workgroup of 256 threads owns a SLICE of P = min(D / 16, 64) pieces
// (a wave's load of one image is then up to 1 KiB contiguous), one bin, and one share of the bin's member list; its threads form
// R = 256 / P rows (thread t: piece t % P of row t / P; the 256 - R P threads left over idle), row r takes the share's members r, r + R,
// ... -- UNROLL of them in flight per thread -- and every thread keeps 16 int32 sums, one per byte of its piece.  The rows are added
// through LDS and the workgroup writes its P x 16 sums once: with a store when the bin's list is not shared, else with 32-bit integer
// atomics into the output the call has zeroed, 64 consecutive ints (256 contiguous bytes) per wave instruction.
// Shares.  Slices x bins alone do not fill the device at small D (1x64x64 and K = 50: 200 workgroups), so a bin's list is cut into
// S shares, the same S for every bin (the host does not know the bins' sizes: offsets is on the device): S = TARGET_WORKGROUPS /
// (slices x bins), but no more than leaves an average share MIN_ROWS_PER_SHARE members per row.  A share of bin k is
// ceil(n_k / S) members rounded up to a multiple of R, so bins of different sizes end together only as far as their sizes agree; a
// share past the end of its list returns (its sums are the zeros of the zeroing launch).
// Bounds.  A sum is at most 255 x 2^23 < 2^31 (PG_CLUSTER_MAX_IMAGES); the byte offset order[i] * D is 64-bit.  offsets are clipped to
// [0, n] and an index outside [0, M) is skipped, so a malformed member list reads nothing outside the stack.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_cluster.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_PIECES = 64;             // pieces of 16 bytes per slice: one wave's load of one image is 1 KiB
constexpr int UNROLL = 4;                  // member images in flight per thread
constexpr int TARGET_WORKGROUPS = 2048;    // 8 per CU
constexpr int MIN_ROWS_PER_SHARE = 8;      // a shorter share is all epilogue (16 KiB through LDS and up to 4 KiB of atomics)
constexpr int LDS_STRIDE = 17;             // 16 sums of a thread + 1: threads fall on different banks

__device__ __forceinline__ void add16(int (&acc)[16], const uint4& v)
{
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[4 * j + 0] += (int)(w[j] & 0xffu);
        acc[4 * j + 1] += (int)((w[j] >> 8) & 0xffu);
        acc[4 * j + 2] += (int)((w[j] >> 16) & 0xffu);
        acc[4 * j + 3] += (int)(w[j] >> 24);
    }
}

__global__ __launch_bounds__(THREADS) void cluster_sums_u8_kernel(const uint8_t* __restrict__ stack, const int* __restrict__ order,
                                                                  const int* __restrict__ offsets, int* __restrict__ sums,
                                                                  long long M, long long D, int n, int P, int R, int store)
{
    __shared__ int lds[THREADS * LDS_STRIDE];
    const int tid = threadIdx.x;
    const int k = blockIdx.y;
    int begin = offsets[k], end = offsets[k + 1];
    begin = begin < 0 ? 0 : (begin > n ? n : begin);
    end = end < begin ? begin : (end > n ? n : end);
    const int nk = end - begin;
    const int S = gridDim.z;
    int share = (nk + S - 1) / S;
    share = (share + R - 1) / R * R;                                         // (nk <= 2^23, R <= 256: no overflow)
    const long long first = (long long)begin + (long long)blockIdx.z * share;
    if (!store && first >= end) return;                                      // uniform: before any barrier
    const long long last = first + share < end ? first + share : end;

    const int p = tid % P, r = tid / P;
    const long long piece = (long long)blockIdx.x * P + p;                   // of the image, in 16-byte units
    const bool active = r < R && piece * 16 < D;
    int acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0;
    if (active) {
        const uint8_t* base = stack + piece * 16;
        for (long long i = first + r; i < last; i += (long long)UNROLL * R) {
            int idx[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const long long iu = i + (long long)u * R;
                idx[u] = iu < last ? order[iu] : -1;
            }
            uint4 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                v[u] = make_uint4(0u, 0u, 0u, 0u);
                if (idx[u] >= 0 && idx[u] < M) v[u] = *reinterpret_cast<const uint4*>(base + (long long)idx[u] * D);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) add16(acc, v[u]);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) lds[tid * LDS_STRIDE + e] = acc[e];
    __syncthreads();
    // output o = 16 p + e of the slice: consecutive threads, consecutive ints of sums
    const long long row = (long long)k * D + (long long)blockIdx.x * P * 16;
    for (int o = tid; o < P * 16; o += THREADS) {
        const int op = o >> 4, e = o & 15;
        if (((long long)blockIdx.x * P + op) * 16 >= D) continue;
        int s = 0;
        for (int rr = 0; rr < R; ++rr) s += lds[(rr * P + op) * LDS_STRIDE + e];
        if (store) sums[row + o] = s;
        else atomicAdd(sums + row + o, s);
    }
}

__global__ __launch_bounds__(THREADS) void zero_i32x4_kernel(int4* __restrict__ p, long long n4)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
        p[i] = make_int4(0, 0, 0, 0);
}

// one thread per column; UNROLL_K rows in flight
constexpr int UNROLL_K = 4;

__global__ __launch_bounds__(THREADS) void cluster_argmin_i64_kernel(const long long* __restrict__ dist, int* __restrict__ label,
                                                                     long long* __restrict__ best, long long M, int K)
{
    const long long m = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (m >= M) return;
    long long bv = dist[m];
    int bk = 0;
    for (int k0 = 1; k0 < K; k0 += UNROLL_K) {
        long long v[UNROLL_K];
#pragma unroll
        for (int u = 0; u < UNROLL_K; ++u) v[u] = k0 + u < K ? dist[(long long)(k0 + u) * M + m] : bv;
#pragma unroll
        for (int u = 0; u < UNROLL_K; ++u)
            if (k0 + u < K && v[u] < bv) { bv = v[u]; bk = k0 + u; }          // strictly less, ascending k: the lower k keeps a tie
    }
    label[m] = bk;
    best[m] = bv;
}

// four elements per thread (D is a multiple of 16: a group of four never crosses a bin)
__global__ __launch_bounds__(THREADS) void cluster_centroids_u8_kernel(const int4* __restrict__ sums, const long long* __restrict__ counts,
                                                                       uint32_t* __restrict__ centroids, long long D4, long long n4)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long nk = counts[i / D4];
        if (nk <= 0) continue;                                               // an empty bin keeps its centroid
        const int4 s = sums[i];
        const int in[4] = {s.x, s.y, s.z, s.w};
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            long long q = (2 * (long long)in[j] + nk) / (2 * nk);
            q = q < 0 ? 0 : (q > 255 ? 255 : q);
            out |= (uint32_t)q << (8 * j);
        }
        centroids[i] = out;
    }
}

inline int grid_for(long long total, int block = THREADS, int cap = 4096)
{
    long long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

extern "C" int pg_cluster_argmin_i64(const int64_t* dist, int K, int64_t M, int* label, int64_t* best, pg_stream_t stream)
{
    if (!dist || !label || !best || K < 1 || K > PG_NN_MAX_QUERIES || M < 1 || M > 0x7fffffffLL) return PG_E_ARG;
    hipLaunchKernelGGL(cluster_argmin_i64_kernel, dim3((unsigned)((M + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const long long*>(dist), label, reinterpret_cast<long long*>(best), (long long)M, K);
    return (int)hipGetLastError();
}

extern "C" int pg_cluster_sums_u8(const uint8_t* stack, int64_t M, int64_t D, const int* order, int64_t n, const int* offsets, int K,
                                  int* sums, pg_stream_t stream)
{
    if (!stack || !order || !offsets || !sums || M < 1 || M > PG_CLUSTER_MAX_IMAGES || n < 1 || n > M || K < 1 || K > PG_NN_MAX_QUERIES
        || D < 1) return PG_E_ARG;
    if (D % 16 || (uintptr_t)stack % 16 || (uintptr_t)sums % 16) return PG_E_ALIGN;
    const long long pieces = D / 16;
    const int P = pieces < MAX_PIECES ? (int)pieces : MAX_PIECES;
    const int R = THREADS / P;
    const long long slices = (pieces + P - 1) / P;
    if (slices > 0x7fffffffLL) return PG_E_UNSUP;                            // gridDim.x (D >= 2 TiB per image)
    long long S = (TARGET_WORKGROUPS + slices * K - 1) / (slices * K);
    const long long most = n / ((long long)K * R * MIN_ROWS_PER_SHARE);
    if (S > most) S = most;
    if (S < 1) S = 1;
    if (S > 65535) S = 65535;                                                // gridDim.z
    const int store = S == 1;
    if (!store)
        hipLaunchKernelGGL(zero_i32x4_kernel, dim3(grid_for((long long)K * D / 4)), dim3(THREADS), 0, (hipStream_t)stream,
                           reinterpret_cast<int4*>(sums), (long long)K * D / 4);
    hipLaunchKernelGGL(cluster_sums_u8_kernel, dim3((unsigned)slices, (unsigned)K, (unsigned)S), dim3(THREADS), 0, (hipStream_t)stream,
                       stack, order, offsets, sums, (long long)M, (long long)D, (int)n, P, R, store);
    return (int)hipGetLastError();
}

extern "C" int pg_cluster_centroids_u8(const int* sums, const int64_t* counts, uint8_t* centroids, int K, int64_t D, pg_stream_t stream)
{
    if (!sums || !counts || !centroids || K < 1 || K > PG_NN_MAX_QUERIES || D < 1) return PG_E_ARG;
    if (D % 16 || (uintptr_t)sums % 16 || (uintptr_t)centroids % 16 || (uintptr_t)counts % 8) return PG_E_ALIGN;
    const long long n4 = (long long)K * D / 4;
    hipLaunchKernelGGL(cluster_centroids_u8_kernel, dim3(grid_for(n4)), dim3(THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const int4*>(sums), reinterpret_cast<const long long*>(counts),
                       reinterpret_cast<uint32_t*>(centroids), (long long)(D / 4), n4);
    return (int)hipGetLastError();
}
