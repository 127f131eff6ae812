// Nearest training images of generated samples, where the training set already is (DeviceImageDataset's uint8 stack in HBM):
//   pg_quantize_u8       : fp32 samples -> the 0..255 levels of the saved image (pg_image_grid_u8's arithmetic, bit for bit)
//   pg_l2dist_u8         : exact squared L2 distance of every (query, stack image) pair on v_mfma_i32_32x32x32_i8, int64
//   pg_topk_smallest_i64 : the k <= 16 smallest of every row, ascending by (value, index)
// Everything is integer arithmetic: the results are exact and the same from run to run.
//
// pg_l2dist_u8.  With x' = x - 128 and q' = q - 128 (one XOR 0x80808080 per dword turns four uint8 into four int8)
//     sum_d (x_d - q_d)^2 = sum x'^2 - 2 sum x' q' + sum q'^2 ;
// the cross term is a [K x D] . [D x M] product on the i8 MFMA (queries = A operand / rows, stack images = B operand / columns, so
// that a register of the 32x32 result is 32 consecutive images of one query: 256 contiguous bytes of the int64 output), the two norms
// are v_dot4_i32_i8 of the dwords that are in registers for the product anyway -- the stack is read from HBM once per launch and no
// norm pass exists.
//
// Work: a workgroup of 4 waves owns TILE_M = 128 stack images (32 per wave) x all queries of the launch (<= PG_NN_MAX_QUERIES = 64, two
// 32-query tiles) x one slice of D; it walks the slice in chunks of CHUNK = 128 bytes of every image.  Lane (c, h) = (lane & 31,
// lane >> 5) of a wave reads the 64 bytes [64 h, 64 h + 64) of the chunk of ITS image as four 16-byte loads -- a wave's four loads
// cover 32 rows x 128 bytes, whole cache lines, each fetched once -- and 16-byte piece i is its operand of the chunk's MFMA i.  The
// queries of a chunk (64 x 128 bytes) are staged through LDS once per workgroup, already shifted, in fragment order (slot
// [tile][i][lane]: a wave's ds_read_b128 reads 64 consecutive 16-byte slots); lane (r, h) takes bytes [64 h + 16 i, + 16) of query r.
// Both operands of MFMA i therefore hold the same 32 values of d -- lane half h element j is d = 64 h + 16 i + j on both sides -- which is
// all the product needs: the order of k inside an instruction is free as long as A and B agree.  Rows and columns are NOT free:
// A's row and B's column are lane & 31, the result's column is lane & 31 and its row (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//
// Bounds.  |x' q'| <= 2^14, an MFMA adds 32 products to an element, a chunk 128: <= 2^21 per chunk.  A slice is at most
// MAX_SLICE_CHUNKS = 512 chunks = 65536 terms <= 2^30 < 2^31 in the int32 accumulator (it would hold 131072 terms); it is widened to int64
// when the slice ends and everything after that is 64-bit.  A lane's norm partial of a chunk is <= 64 * 2^14 = 2^20 in int32 and is
// added to an int64 every chunk.
// Tail.  D is a multiple of 16 (16 {1,3} 4^j), not always of 128: a 16-byte piece at or past D is never loaded and is ZERO IN THE SHIFTED
// domain (raw zero bytes would become -128 under the XOR and add 16384 per element to the norms).  Images >= M and queries >= K read
// the last valid one instead (their results are not written).
// Slices combine with 64-bit integer atomicAdd into a zeroed output (integer addition is associative: the result does not depend on the
// order); a launch with one slice stores.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip.h"
#include "u8l2.h"

namespace {

using namespace u8l2;                      // v4i, v16i, SHIFT, I64_MAX, shifted, sumsq16, load16, grid_for

constexpr int CHUNK = 128;                 // bytes of every image per step: 4 MFMAs of 32
constexpr int TILE_M = 128;                // stack images per workgroup (4 waves x 32)
constexpr int MAX_SLICE_CHUNKS = 512;      // 65536 terms per int32 accumulator lifetime (see Bounds)
constexpr int MIN_SLICE_CHUNKS = 32;       // a slice shorter than 4 KiB per image is all epilogue
constexpr int TARGET_WORKGROUPS = 1024;    // 4 per CU (768 = the 3 per CU the 64-query form admits measured the same)

template <int KT>
__global__ __launch_bounds__(256) void l2dist_u8_kernel(const uint8_t* __restrict__ stack, const uint8_t* __restrict__ queries,
                                                        long long* __restrict__ out, long long M, int K, long long D,
                                                        int slice_chunks, int nchunks, int store)
{
    __shared__ v4i qlds[KT * 4 * 64];                                        // [tile][piece i][lane]: KT * 4 KiB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5;
    const long long m0 = (long long)blockIdx.x * TILE_M + wave * 32;        // first image of this wave
    const bool wave_active = m0 < M;                                         // (uniform per wave; idle waves still stage queries)
    const long long m_row = m0 + c < M ? m0 + c : M - 1;
    const uint8_t* xrow = stack + m_row * D + 64 * h;
    // staging: thread -> (query of the tile, 16-byte piece of the chunk)
    const int sq = tid >> 3, sp = tid & 7;
    const uint8_t* qrow[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
        const int q = 32 * t + sq < K ? 32 * t + sq : K - 1;
        qrow[t] = queries + (long long)q * D + 16 * sp;
    }
    const int slot = (sp & 3) * 64 + (sp >> 2) * 32 + sq;                     // piece sp = 4 h + i of query sq -> [i][h * 32 + sq]

    const int j0 = blockIdx.y * slice_chunks;
    const int j1 = j0 + slice_chunks < nchunks ? j0 + slice_chunks : nchunks;

    v16i acc[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0;
    long long nx = 0, nq[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) nq[t] = 0;

    uint4 gx[4], gq[KT];
    {
        const long long k0 = (long long)j0 * CHUNK;
#pragma unroll
        for (int i = 0; i < 4; ++i) gx[i] = load16(xrow + k0 + 16 * i, wave_active && k0 + 64 * h + 16 * i < D);
#pragma unroll
        for (int t = 0; t < KT; ++t) gq[t] = load16(qrow[t] + k0, k0 + 16 * sp < D);
    }
    for (int j = j0; j < j1; ++j) {
        __syncthreads();                                                     // the previous chunk's fragments have been read
#pragma unroll
        for (int t = 0; t < KT; ++t) qlds[t * 256 + slot] = shifted(gq[t]);
        v4i b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = shifted(gx[i]);
        __syncthreads();
        if (j + 1 < j1) {                                                    // next chunk: in flight during this one's MFMAs
            const long long k0 = (long long)(j + 1) * CHUNK;
#pragma unroll
            for (int i = 0; i < 4; ++i) gx[i] = load16(xrow + k0 + 16 * i, wave_active && k0 + 64 * h + 16 * i < D);
#pragma unroll
            for (int t = 0; t < KT; ++t) gq[t] = load16(qrow[t] + k0, k0 + 16 * sp < D);
        }
        if (wave_active) {
            int sx = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) sx = sumsq16(b[i], sx);
            nx += sx;
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                int s = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const v4i a = qlds[t * 256 + i * 64 + lane];
                    s = sumsq16(a, s);
                    acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[i], acc[t], 0, 0, 0);
                }
                nq[t] += s;
            }
        }
    }
    if (!wave_active) return;                                                // (no barrier follows)
    // lane (c, h) holds half of image c's norm and half of query r = c's; the result register e of tile t is query
    // 32 t + (e & 3) + 8 (e >> 2) + 4 h against image m0 + c
    nx += __shfl_xor(nx, 32);
#pragma unroll
    for (int t = 0; t < KT; ++t) nq[t] += __shfl_xor(nq[t], 32);
    const long long m = m0 + c;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = (e & 3) + 8 * (e >> 2) + 4 * h;
            const long long nqr = __shfl(nq[t], r);
            const int k = 32 * t + r;
            const long long v = nx + nqr - 2 * (long long)acc[t][e];
            if (m < M && k < K) {
                long long* p = out + (long long)k * M + m;
                if (store) *p = v;
                else atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
            }
        }
    }
}

__global__ __launch_bounds__(256) void zero_i64_kernel(long long* __restrict__ p, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = 0;
}

// four elements per thread where the tensor allows it; scale and rounding as to_level of csrc/msssim.hip, mode 2
__device__ __forceinline__ uint8_t level_of(float x, float lo, float scale)
{
    const float y = __fmul_rn(__fsub_rn(x, lo), scale);
    return (uint8_t)fminf(fmaxf(rintf(y), 0.f), 255.f);
}

__global__ __launch_bounds__(256) void quantize_u8_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, long long n,
                                                          float lo, float scale)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = level_of(in[i], lo, scale);
}

__global__ __launch_bounds__(256) void quantize_u8x4_kernel(const float4* __restrict__ in, uint32_t* __restrict__ out, long long n4,
                                                            float lo, float scale)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const float4 v = in[i];
        out[i] = (uint32_t)level_of(v.x, lo, scale) | ((uint32_t)level_of(v.y, lo, scale) << 8) |
                 ((uint32_t)level_of(v.z, lo, scale) << 16) | ((uint32_t)level_of(v.w, lo, scale) << 24);
    }
}

// ---------------------------------------------------------------------------------------------------------------- top-k
// One workgroup of 256 threads per row (TOPK = 1, 4, 8 or 16 >= k: the insert is TOPK steps and some lane of a wave inserts almost every
// element, so a short list is what a small k costs).  Thread t keeps the TOPK smallest (value, index) of elements t, t + 256, ... sorted in
// registers (compile-time indices only); then k rounds of a workgroup-wide minimum over the threads' heads, the winner dropping
// its head.  Keys are unique (the index breaks ties), so every round has exactly one winner: no atomics, no dependence on timing.
constexpr int TOPK_LOADS = 8;

__device__ __forceinline__ bool key_less(long long v, int i, long long w, int j) { return v < w || (v == w && i < j); }

template <int TOPK>
__global__ __launch_bounds__(256) void topk_smallest_i64_kernel(const long long* __restrict__ dist, long long* __restrict__ val,
                                                                long long* __restrict__ idx, int M, int k)
{
    __shared__ long long sv[4];
    __shared__ int si[4];
    const long long* row = dist + (long long)blockIdx.x * M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long v[TOPK];
    int ix[TOPK];
#pragma unroll
    for (int j = 0; j < TOPK; ++j) { v[j] = I64_MAX; ix[j] = 0x7fffffff; }
    for (int base = tid; base < M; base += 256 * TOPK_LOADS) {               // TOPK_LOADS independent loads in flight, then the inserts in index order
        long long x[TOPK_LOADS];
#pragma unroll
        for (int u = 0; u < TOPK_LOADS; ++u) x[u] = base + 256 * u < M ? row[base + 256 * u] : I64_MAX;
#pragma unroll
        for (int u = 0; u < TOPK_LOADS; ++u) {
            const int i = base + 256 * u;
            if (i < M && key_less(x[u], i, v[TOPK - 1], ix[TOPK - 1])) {
#pragma unroll
                for (int j = TOPK - 1; j >= 0; --j) {
                    const bool above = j > 0 && key_less(x[u], i, v[j > 0 ? j - 1 : 0], ix[j > 0 ? j - 1 : 0]);   // the new key goes further down
                    if (above) { v[j] = v[j - 1]; ix[j] = ix[j - 1]; }
                    else if (key_less(x[u], i, v[j], ix[j])) { v[j] = x[u]; ix[j] = i; }
                }
            }
        }
    }
    for (int round = 0; round < k; ++round) {
        long long bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const long long ov = __shfl_xor(bv, off);
            const int oi = __shfl_xor(bi, off);
            if (key_less(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
        __syncthreads();
        bv = sv[0]; bi = si[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (key_less(sv[w], si[w], bv, bi)) { bv = sv[w]; bi = si[w]; }
        __syncthreads();                                                     // sv / si are rewritten next round
        if (ix[0] == bi) {                                                   // the one winner (k <= M: bi is a real index)
#pragma unroll
            for (int j = 0; j < TOPK - 1; ++j) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
            v[TOPK - 1] = I64_MAX; ix[TOPK - 1] = 0x7fffffff;
        }
        if (tid == 0) {
            val[(long long)blockIdx.x * k + round] = bv;
            idx[(long long)blockIdx.x * k + round] = bi;
        }
    }
}

}  // namespace

extern "C" int pg_quantize_u8(const float* in, uint8_t* out, int64_t n, float lo, float hi, pg_stream_t stream)
{
    if (!in || !out || n <= 0 || !(hi > lo)) return PG_E_ARG;
    const float scale = (float)(255.0 / ((double)hi - (double)lo));
    if (n % 4 == 0 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 4 == 0)
        hipLaunchKernelGGL(quantize_u8x4_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(in), reinterpret_cast<uint32_t*>(out), (long long)(n / 4), lo, scale);
    else
        hipLaunchKernelGGL(quantize_u8_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, in, out, (long long)n, lo, scale);
    return (int)hipGetLastError();
}

extern "C" int pg_l2dist_u8(const uint8_t* stack, int64_t M, const uint8_t* queries, int K, int64_t D, int64_t* out, pg_stream_t stream)
{
    if (!stack || !queries || !out || M <= 0 || K <= 0 || K > PG_NN_MAX_QUERIES || D <= 0) return PG_E_ARG;
    if (D % 16 || (uintptr_t)stack % 16 || (uintptr_t)queries % 16 || (uintptr_t)out % 8) return PG_E_ALIGN;
    const long long mtiles = (M + TILE_M - 1) / TILE_M;
    const long long nchunks = (D + CHUNK - 1) / CHUNK;
    if (mtiles > 0x7fffffffLL || nchunks > 0x7fffffffLL) return PG_E_UNSUP;
    // slices: enough workgroups to fill the device, none shorter than MIN_SLICE_CHUNKS, none longer than MAX_SLICE_CHUNKS
    long long nslices = (TARGET_WORKGROUPS + mtiles - 1) / mtiles;
    const long long most = nchunks / MIN_SLICE_CHUNKS > 0 ? nchunks / MIN_SLICE_CHUNKS : 1;
    if (nslices > most) nslices = most;
    long long slice_chunks = (nchunks + nslices - 1) / nslices;
    if (slice_chunks > MAX_SLICE_CHUNKS) slice_chunks = MAX_SLICE_CHUNKS;
    nslices = (nchunks + slice_chunks - 1) / slice_chunks;
    if (nslices > 65535) return PG_E_UNSUP;                                  // gridDim.y (D > 4 GiB per image)
    const int store = nslices == 1;
    if (!store)
        hipLaunchKernelGGL(zero_i64_kernel, dim3(grid_for((long long)K * M)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<long long*>(out), (long long)K * M);
    const dim3 grid((unsigned)mtiles, (unsigned)nslices);
    if (K <= 32)
        hipLaunchKernelGGL(l2dist_u8_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, stack, queries,
                           reinterpret_cast<long long*>(out), (long long)M, K, (long long)D, (int)slice_chunks, (int)nchunks, store);
    else
        hipLaunchKernelGGL(l2dist_u8_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, stack, queries,
                           reinterpret_cast<long long*>(out), (long long)M, K, (long long)D, (int)slice_chunks, (int)nchunks, store);
    return (int)hipGetLastError();
}

extern "C" int pg_topk_smallest_i64(const int64_t* dist, int K, int64_t M, int k, int64_t* values, int64_t* indices, pg_stream_t stream)
{
    if (!dist || !values || !indices || K <= 0 || M <= 0 || k < 1 || k > PG_NN_MAX_TOPK || k > M) return PG_E_ARG;
    if (M > 0x7fffffffLL - 2 * 256 * TOPK_LOADS) return PG_E_UNSUP;          // (the scan's int index runs up to M + 256 TOPK_LOADS)
    const long long* d = reinterpret_cast<const long long*>(dist);
    long long* v = reinterpret_cast<long long*>(values);
    long long* i = reinterpret_cast<long long*>(indices);
    const hipStream_t s = (hipStream_t)stream;
    if (k == 1) hipLaunchKernelGGL(topk_smallest_i64_kernel<1>, dim3(K), dim3(256), 0, s, d, v, i, (int)M, k);
    else if (k <= 4) hipLaunchKernelGGL(topk_smallest_i64_kernel<4>, dim3(K), dim3(256), 0, s, d, v, i, (int)M, k);
    else if (k <= 8) hipLaunchKernelGGL(topk_smallest_i64_kernel<8>, dim3(K), dim3(256), 0, s, d, v, i, (int)M, k);
    else hipLaunchKernelGGL(topk_smallest_i64_kernel<16>, dim3(K), dim3(256), 0, s, d, v, i, (int)M, k);
    return (int)hipGetLastError();
}
