// Shift-invariant nearest training windows of generated samples, where the recordings already are (DeviceStripDataset's uint8 strips):
//   pg_shift_l2min_u8 : for every (query, segment of start columns) the smallest exact squared L2 distance between the query and the
//                       S x S windows at EVERY start column of the segment, and that start, as one int64 key (include/pggan_hip_shift.h)
// Integer arithmetic throughout: exact, and the same bits from run to run.
//
// Along one strip row the distances at all starts are a 1-D cross-correlation: a GEMM whose one operand is the Hankel matrix
// H[u][j] = s[u + j] of the row.  It is never built: the operand registers of a start are cut out of the row where it lies.  With
// x' = x - 128, q' = q - 128 (XOR 0x80808080) as in nn_search.hip,
//     d[k, u] = sum x'^2 - 2 sum x' q' + sum q'^2
// the cross term runs on v_mfma_i32_32x32x32_i8 (queries = A / rows, starts = B / columns) and both norms are v_dot4_i32_i8 of the
// operand registers a lane holds anyway: no norm pass.  (Every wave holds every query fragment; each sums a quarter of them.)
//
// Work (S >= 32).  A workgroup of 4 waves owns PG_SHIFT_TILE = 128 consecutive starts u0 .. u0 + 127 of one strip (u0 a multiple of
// 128) x all queries of the launch (KT tiles of 32) x the WHOLE contraction C S S: a key needs complete distances.  Wave w owns
// the starts u0 + w + 4 c, c = lane & 31: every start of a wave has the SAME byte offset w within a dword, so the wave reads copy w of
// the row -- the row shifted by w bytes, made once per workgroup with v_alignbyte_b32 while it is staged to LDS -- at dword
// addresses, and no lane aligns anything in the inner loop.  The contraction is walked in steps of 256 bytes of every query, which
// are contiguous in the query: RB = 256 / S whole rows for S < 256, a chunk of CH = 256 columns of one row above.  A step is
// 8 MFMAs per query tile; MFMA (rr, i) of a step takes, in lane half h, the columns chunk + h CH/2 + 16 i + [0, 16) of row rr on both
// sides (the order of k inside an instruction is free as long as A and B agree).  For the start u that is the 16 contiguous bytes at
// byte 4 c + h CH/2 + 16 i of copy w: four dword reads.  The queries of a step are staged in fragment order as in nn_search.hip.
// A row contributes CH + 128 bytes from u0 + chunk (ND = CH/4 + 31 dwords per copy, one more source dword for the shift).
//
// Bounds.  A source dword is loaded only if it lies inside the row's pitch (a multiple of 16, so dwords are whole); others read
// as zero.  A valid start u <= T - S only ever uses bytes below T, so padding and the zero fill reach invalid starts alone, whose
// keys are never written.  |x' q'| <= 2^14 and a step adds 256 products to an accumulator element: the int32 accumulators live for
// WIDEN_STEPS = 256 steps = 65536 terms <= 2^30 (nn_search.hip's bound) and are then added into int64.  A lane's norm partial of a step is
// <= 128 * 2^14 = 2^21 and is added to an int64 every step.
// Segments.  A tile that lies in one segment (always, when seg is a multiple of 128) reduces its 32 starts per wave with shuffles and
// issues one atomic per (wave, query); any other tile issues one per (start, query).  Both are 64-bit integer atomic minima into
// keys preset to INT64_MAX, above every valid key (< 2^54): order-independent.
// S < 32: a row is shorter than an MFMA k-step; those levels (at most 3 x 16 x 16 bytes per window) take a plain integer kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_shift.h"
#include "u8l2.h"

namespace {

using namespace u8l2;                      // v4i, v16i, SHIFT, I64_MAX, shifted, sumsq16, load16, grid_for

constexpr int TILE = PG_SHIFT_TILE;
constexpr int STEP = 256;                   // bytes of every query per step: 8 MFMAs of 32
constexpr int WIDEN_STEPS = 256;            // 65536 terms per int32 accumulator lifetime (see Bounds)
constexpr int XLDS_DWORDS = 8 * 4 * (32 / 4 + 31);   // the largest step: S = 32, 8 rows x 4 copies x 39 dwords

static_assert(TILE == 128, "the wave / copy mapping below is written for 4 waves x 32 starts");

// the strip whose tiles hold workgroup `tile`: the last m with segtab[m].first_tile <= tile
__device__ __forceinline__ int strip_of_tile(const int64_t* __restrict__ segtab, int M, long long tile)
{
    int lo = 0, hi = M - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segtab[PG_SHIFT_SEGTAB_WORDS * mid + 1] <= tile) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void fill_i64_kernel(long long* __restrict__ p, long long n, long long v)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) p[i] = v;
}

template <int KT>
__global__ __launch_bounds__(256) void shift_l2min_mfma_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                               const int64_t* __restrict__ segtab, int M, int C, int ls,
                                                               const uint8_t* __restrict__ queries, int K, int seg, long long G,
                                                               long long* __restrict__ key)
{
    __shared__ v4i qlds[KT * 8 * 64];                                        // [tile][MFMA of the step][lane]: KT * 8 KiB
    __shared__ unsigned xlds[XLDS_DWORDS];                                   // [row of the step][copy w][ND]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int m = strip_of_tile(segtab, M, blockIdx.x);
    const long long off = table[PG_CROP_TABLE_WORDS * m], pitch = table[PG_CROP_TABLE_WORDS * m + 1], cols = table[PG_CROP_TABLE_WORDS * m + 2];
    const long long u0 = ((long long)blockIdx.x - segtab[PG_SHIFT_SEGTAB_WORDS * m + 1]) * TILE;
    const int S = 1 << ls;
    const long long last = cols - S;                                         // the last valid start
    const int lch = ls < 8 ? ls : 8, CH = 1 << lch;                          // columns of a row per step
    const int lrb = 8 - lch, RB = 1 << lrb;                                  // rows per step
    const int lspr = ls - lch;                                               // log2(steps per row)
    const int lmi = lch - 5;                                                 // log2(MFMAs per row of a step)
    const int ND = CH / 4 + 31;                                              // dwords of one copy of a row
    const long long D = (long long)C << (2 * ls);
    const int nsteps = (int)(D >> 8);
    const uint8_t* strip = src + off + u0;

    // staging of the strip rows: thread -> up to two (row of the step, source dword n); it writes dword n of the four copies
    bool xok[2];
    int xdst[2], xn[2];
    long long xsrc[2];
#pragma unroll
    for (int z = 0; z < 2; ++z) {
        const int it = tid + 256 * z;
        xok[z] = it < RB * ND;
        const int rr = xok[z] ? it / ND : 0;
        xn[z] = xok[z] ? it - rr * ND : 0;
        xdst[z] = rr * 4 * ND + xn[z];
        xsrc[z] = rr * pitch + 4 * xn[z];
    }
    // staging of the queries: thread -> 2 KT (query of the launch, 16-byte piece of the step's 256 bytes)
    int qdst[2 * KT];
    const uint8_t* qsrc[2 * KT];
#pragma unroll
    for (int n = 0; n < 2 * KT; ++n) {
        const int p = tid + 256 * n;
        const int ql = p >> 4, x = p & 15;
        const int b = 16 * x, rr = b >> lch, cc = b & (CH - 1);
        const int hh = cc >> (lch - 1), i = (cc & (CH / 2 - 1)) >> 4;
        qdst[n] = (ql >> 5) * 512 + ((rr << lmi) + i) * 64 + hh * 32 + (ql & 31);
        qsrc[n] = queries + (long long)(ql < K ? ql : K - 1) * D + b;
    }
    const int xlane = wave * ND + c + h * (CH / 8);                          // dword of this lane's start in copy `wave`, MFMA (0, 0)

    long long tot[KT][16];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[t][e] = 0;
    long long nx = 0, nq[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) nq[t] = 0;

    unsigned g0[2], g1[2];
    uint4 gq[2 * KT];
    auto prefetch = [&](int st) {
        const long long row0 = (long long)(st >> lspr) << lrb;
        const long long chunk = (long long)(st & ((1 << lspr) - 1)) << 8;
        const uint8_t* base = strip + row0 * pitch + chunk;
#pragma unroll
        for (int z = 0; z < 2; ++z) {
            const long long col = u0 + chunk + 4 * xn[z];                    // column of the dword's first byte
            g0[z] = 0u; g1[z] = 0u;
            if (xok[z] && col + 4 <= pitch) g0[z] = *reinterpret_cast<const unsigned*>(base + xsrc[z]);
            if (xok[z] && col + 8 <= pitch) g1[z] = *reinterpret_cast<const unsigned*>(base + xsrc[z] + 4);
        }
#pragma unroll
        for (int n = 0; n < 2 * KT; ++n) gq[n] = *reinterpret_cast<const uint4*>(qsrc[n] + (long long)st * STEP);
    };
    prefetch(0);
    for (int st0 = 0; st0 < nsteps; st0 += WIDEN_STEPS) {                    // one lifetime of the int32 accumulators
    const int st1 = st0 + WIDEN_STEPS < nsteps ? st0 + WIDEN_STEPS : nsteps;
    v16i acc[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0;
    for (int st = st0; st < st1; ++st) {
        __syncthreads();                                                     // the previous step's fragments have been read
#pragma unroll
        for (int n = 0; n < 2 * KT; ++n) {
            v4i v;
            v.x = (int)(gq[n].x ^ SHIFT); v.y = (int)(gq[n].y ^ SHIFT); v.z = (int)(gq[n].z ^ SHIFT); v.w = (int)(gq[n].w ^ SHIFT);
            qlds[qdst[n]] = v;
        }
#pragma unroll
        for (int z = 0; z < 2; ++z)
            if (xok[z]) {
                xlds[xdst[z]] = g0[z] ^ SHIFT;
                xlds[xdst[z] + ND] = __builtin_amdgcn_alignbyte(g1[z], g0[z], 1) ^ SHIFT;
                xlds[xdst[z] + 2 * ND] = __builtin_amdgcn_alignbyte(g1[z], g0[z], 2) ^ SHIFT;
                xlds[xdst[z] + 3 * ND] = __builtin_amdgcn_alignbyte(g1[z], g0[z], 3) ^ SHIFT;
            }
        __syncthreads();
        if (st + 1 < nsteps) prefetch(st + 1);                               // in flight during this step's MFMAs
        int sx = 0, sq[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) sq[t] = 0;
#pragma unroll
        for (int mm = 0; mm < 8; ++mm) {
            const int o = xlane + (mm >> lmi) * 4 * ND + 4 * (mm & ((1 << lmi) - 1));
            v4i b;
            b.x = (int)xlds[o]; b.y = (int)xlds[o + 1]; b.z = (int)xlds[o + 2]; b.w = (int)xlds[o + 3];
            sx = sumsq16(b, sx);
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const v4i a = qlds[t * 512 + mm * 64 + lane];
                if ((mm & 3) == wave) sq[t] = sumsq16(a, sq[t]);                 // (a quarter of the query norms per wave)
                acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc[t], 0, 0, 0);
            }
        }
        nx += sx;
#pragma unroll
        for (int t = 0; t < KT; ++t) nq[t] += sq[t];
    }
#pragma unroll
    for (int t = 0; t < KT; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[t][e] += acc[t][e];
    }
    // lane (c, h) holds half of the norm of start u0 + wave + 4 c and half of query r = c's; result register e of tile t is query
    // 32 t + (e & 3) + 8 (e >> 2) + 4 h against that start
    // ... and a quarter of that half: wave w took the MFMAs mm = w, w + 4 of every step.  The quarters meet in LDS.
    __syncthreads();                                                         // the last step's fragments have been read
    long long* nlds = reinterpret_cast<long long*>(qlds);                    // [tile][wave][lane]: KT * 2 KiB of KT * 8
#pragma unroll
    for (int t = 0; t < KT; ++t) nlds[(t * 4 + wave) * 64 + lane] = nq[t];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < KT; ++t) nq[t] = nlds[(t * 4) * 64 + lane] + nlds[(t * 4 + 1) * 64 + lane] + nlds[(t * 4 + 2) * 64 + lane] + nlds[(t * 4 + 3) * 64 + lane];
    nx += __shfl_xor(nx, 32);
#pragma unroll
    for (int t = 0; t < KT; ++t) nq[t] += __shfl_xor(nq[t], 32);
    const long long u = u0 + wave + 4 * c;
    const bool valid = u <= last;
    const long long tile_last = u0 + TILE - 1 < last ? u0 + TILE - 1 : last;
    const long long gl0 = u0 / seg, gl = u / seg;
    const bool one_segment = gl0 == tile_last / seg;                         // (uniform over the workgroup)
    const long long gfirst = segtab[PG_SHIFT_SEGTAB_WORDS * m];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = (e & 3) + 8 * (e >> 2) + 4 * h;
            const long long nqr = __shfl(nq[t], r);
            const int k = 32 * t + r;
            const long long d = nx + nqr - 2 * tot[t][e];
            const long long kv = (d << PG_SHIFT_POS_BITS) + (u - gl * seg);
            if (one_segment) {
                long long v = valid ? kv : I64_MAX;
#pragma unroll
                for (int s = 16; s > 0; s >>= 1) {
                    const long long o = __shfl_xor(v, s);
                    v = o < v ? o : v;
                }
                if (c == 0 && k < K && v != I64_MAX) atomicMin(key + (long long)k * G + gfirst + gl0, v);
            } else if (valid && k < K) {
                atomicMin(key + (long long)k * G + gfirst + gl, kv);
            }
        }
    }
}

// S < 32: thread -> one start of the tile x every second query; byte loads, plain integer arithmetic (D <= 768: int32 holds 768 * 65025)
__global__ __launch_bounds__(256) void shift_l2min_small_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                                const int64_t* __restrict__ segtab, int M, int C, int ls,
                                                                const uint8_t* __restrict__ queries, int K, int seg, long long G,
                                                                long long* __restrict__ key)
{
    const int tid = threadIdx.x;
    const int m = strip_of_tile(segtab, M, blockIdx.x);
    const long long off = table[PG_CROP_TABLE_WORDS * m], pitch = table[PG_CROP_TABLE_WORDS * m + 1], cols = table[PG_CROP_TABLE_WORDS * m + 2];
    const int S = 1 << ls;
    const long long u = ((long long)blockIdx.x - segtab[PG_SHIFT_SEGTAB_WORDS * m + 1]) * TILE + (tid & (TILE - 1));
    if (u > cols - S) return;                                                // (no barrier follows)
    const uint8_t* win = src + off + u;
    const int rows = C << ls, D = rows << ls;
    const long long gl = u / seg;
    long long* out = key + segtab[PG_SHIFT_SEGTAB_WORDS * m] + gl;
    for (int k = tid >> 7; k < K; k += 2) {
        const uint8_t* q = queries + (long long)k * D;
        int d = 0;
        for (int row = 0; row < rows; ++row) {
            const uint8_t* x = win + row * pitch;
            for (int j = 0; j < S; ++j) {
                const int v = (int)x[j] - (int)q[(row << ls) + j];
                d += v * v;
            }
        }
        atomicMin(out + (long long)k * G, ((long long)d << PG_SHIFT_POS_BITS) + (u - gl * seg));
    }
}

}  // namespace

extern "C" int pg_shift_l2min_u8(const uint8_t* src, const int64_t* table, int64_t M, int C, int S, const uint8_t* queries, int K, int seg,
                                 const int64_t* segtab, int64_t tiles, int64_t G, int64_t* key, pg_stream_t stream)
{
    if (!src || !table || !queries || !segtab || !key || M <= 0 || M > 0x7fffffffLL || C < 1 || C > 3 || S < 4 || S > 1024 || (S & (S - 1))
        || K < 1 || K > PG_SHIFT_MAX_QUERIES || seg < 1 || seg > (1 << PG_SHIFT_POS_BITS) || tiles < M || tiles > 0x7fffffffLL || G < M
        || G > 0x7fffffffLL) return PG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(queries)) & 15) return PG_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(segtab) | reinterpret_cast<uintptr_t>(key)) & 7) return PG_E_ALIGN;
    int ls = 0;
    while ((1 << ls) < S) ++ls;
    const hipStream_t s = (hipStream_t)stream;
    long long* k64 = reinterpret_cast<long long*>(key);
    hipLaunchKernelGGL(fill_i64_kernel, dim3(grid_for((long long)K * G)), dim3(256), 0, s, k64, (long long)K * G, I64_MAX);
    const dim3 grid((unsigned)tiles);
    if (S < 32)
        hipLaunchKernelGGL(shift_l2min_small_kernel, grid, dim3(256), 0, s, src, table, segtab, (int)M, C, ls, queries, K, seg, (long long)G, k64);
    else if (K <= 32)
        hipLaunchKernelGGL(shift_l2min_mfma_kernel<1>, grid, dim3(256), 0, s, src, table, segtab, (int)M, C, ls, queries, K, seg, (long long)G, k64);
    else
        hipLaunchKernelGGL(shift_l2min_mfma_kernel<2>, grid, dim3(256), 0, s, src, table, segtab, (int)M, C, ls, queries, K, seg, (long long)G, k64);
    return (int)hipGetLastError();
}
