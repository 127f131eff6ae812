// Sliced Wasserstein distance between Laplacian-pyramid patch descriptors (Karras et al. 2018, §5 and appendix), the
// quality metric of a training run, evaluated where its inputs already are:
//   pg_lap_down / pg_lap_up_sub              : the Laplacian pyramid (5x5 binomial filter, reflect boundary without the edge sample)
//   pg_swd_gather                            : 3x7x7 neighbourhoods around given centres -> rows of 147 floats
//   pg_swd_channel_stats / pg_swd_normalize  : per-channel mean / population std over a whole descriptor set, applied in place
//   pg_swd_project                           : [M,147] x [147,K] on v_mfma_f32_32x32x2_f32, written transposed [K,M]
//   pg_swd_gather_c / pg_swd_channel_stats_c / pg_swd_normalize_c / pg_swd_project_c (include/pggan_hip_swd.h): the same four for
//                                              C = 1..4 channels, descriptors of 49 C floats.  The kernels are templates over C and the
//                                              four above are their C = 3 instantiation, so C = 3 gives the same bits through either.
//   pg_swd_sort_rows                         : every row of [K,M] ascending (bitonic runs in LDS + merge-path passes)
//   pg_swd_l1                                : mean |a - b| into one device scalar
// All fp32 on the caller's stream; the scratch each needs is an argument (nothing here uses the registered per-stream workspace).
// The reference has no metric: parity is against the published definition, restated for the CPU in tests/swd_ref.py.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "pggan_hip.h"
#include "pggan_hip_swd.h"

namespace {

constexpr int PATCH = PG_SWD_PATCH;                // 7 x 7: one channel of a descriptor; a descriptor of C channels is PATCH * C floats
static_assert(PG_SWD_DESC == 3 * PATCH, "the entry points of pggan_hip.h are the three-channel instantiation");
constexpr int RED_BLOCKS = PG_SWD_REDUCE_BLOCKS;   // most workgroups a two-stage reduction is spread over
constexpr int RUN = PG_SWD_SORT_RUN;               // elements one workgroup sorts in LDS
constexpr int SORT_THREADS = 1024;
constexpr int TILE = PG_SWD_SORT_MERGE_TILE;       // outputs one workgroup of a merge pass produces
constexpr int MERGE_THREADS = 256;
constexpr int MERGE_ITEMS = TILE / MERGE_THREADS;
constexpr int PJ_M = 128;                          // descriptors per workgroup of the projection (4 waves x 32)
constexpr int PJ_K = 128;                          // directions per workgroup (4 accumulator tiles of 32 per wave)
static_assert(PJ_M % 4 == 0 && PJ_M * PG_SWD_PATCH * PG_SWD_MAX_CHANNELS * 4 <= 160 * 1024, "a workgroup's descriptors are whole float4s and fit in LDS");
static_assert(RUN % TILE == 0, "a merge tile must not straddle two pairs of runs");
static_assert((RUN & (RUN - 1)) == 0 && TILE % MERGE_THREADS == 0, "");

inline int grid_for(long long total, int block, int cap)
{
    long long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// ------------------------------------------------------------------------------------------------- Laplacian pyramid
// index of the sample a 5-tap window sees at i in [-2, S+1]:  d c b | a b c d | c b a
__device__ __forceinline__ int reflect(int i, int S)
{
    i = i < 0 ? -i : i;
    return i >= S ? 2 * S - 2 - i : i;
}

__device__ __forceinline__ float tap(int d) { return d == 2 ? 0.375f : ((d == 1 || d == 3) ? 0.25f : 0.0625f); }   // [1,4,6,4,1]/16

// one thread per output sample: out[y][x] = sum_dy f[dy] sum_dx f[dx] in[r(2y+dy-2)][r(2x+dx-2)]
__global__ __launch_bounds__(256) void lap_down_kernel(const float* __restrict__ in, float* __restrict__ out, long long planes, int S)
{
    const int So = S >> 1;
    const long long total = planes * So * So;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % So);
        const long long r = idx / So;
        const int y = (int)(r % So);
        const float* p = in + (size_t)(r / So) * S * S;
        int xs[5];
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) xs[dx] = reflect(2 * x + dx - 2, S);
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < 5; ++dy) {
            const float* row = p + (size_t)reflect(2 * y + dy - 2, S) * S;
            float a = 0.f;
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) a += tap(dx) * row[xs[dx]];
            acc += tap(dy) * a;
        }
        out[idx] = acc;
    }
}

// one thread per sample of the fine map: out = fine - up(coarse).  up() convolves the zero-inserted coarse map with 4k = (2f)x(2f);
// reflection keeps the parity of an index (S is even), so the taps that land on a non-zero sample are those with dy == y (mod 2) and
// dx == x (mod 2): 3x3, 3x2, 2x3 or 2x2 of the 25.  The zero-inserted map is never formed.
__global__ __launch_bounds__(256) void lap_up_sub_kernel(const float* __restrict__ fine, const float* __restrict__ coarse,
                                                         float* __restrict__ out, long long planes, int S)
{
    const int Sc = S >> 1;
    const long long total = planes * S * S;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % S);
        const long long r = idx / S;
        const int y = (int)(r % S);
        const float* p = coarse + (size_t)(r / S) * Sc * Sc;
        float acc = 0.f;
        for (int dy = y & 1; dy < 5; dy += 2) {
            const float* row = p + (size_t)(reflect(y + dy - 2, S) >> 1) * Sc;
            float a = 0.f;
            for (int dx = x & 1; dx < 5; dx += 2) a += 2.f * tap(dx) * row[reflect(x + dx - 2, S) >> 1];
            acc += 2.f * tap(dy) * a;
        }
        out[idx] = fine[idx] - acc;
    }
}

// ------------------------------------------------------------------------------------------------- descriptors
// one thread per descriptor element, rows in (channel, dy, dx) order.  Centres are clamped to [3, S-4] so that no read leaves the image
// whatever the caller passes; ops.swd_gather rejects a centre outside that range before the launch.
template <int C>
__global__ __launch_bounds__(256) void swd_gather_kernel(const float* __restrict__ level, const int* __restrict__ centres,
                                                         float* __restrict__ out, long long ndesc, int P, int S, long long row_offset)
{
    constexpr int DESC = PATCH * C;
    const long long total = ndesc * DESC;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long j = idx / DESC;
        const int e = (int)(idx - j * DESC);
        const int c = e / 49, dy = (e % 49) / 7, dx = e % 7;
        const int cx = min(max(centres[2 * j], 3), S - 4), cy = min(max(centres[2 * j + 1], 3), S - 4);
        const size_t img = (size_t)(j / P);
        out[(size_t)(row_offset + j) * DESC + e] = level[((img * C + c) * S + (cy - 3 + dy)) * S + (cx - 3 + dx)];
    }
}

// ------------------------------------------------------------------------------------------------- reductions
// Sum of NV doubles per thread over a workgroup of 256: shuffles inside a wave, LDS across the four waves; thread 0 holds the result.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV])
{
    __shared__ double red[4][NV];
#pragma unroll
    for (int i = 0; i < NV; ++i)
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_down(v[i], off, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < NV; ++i) red[wave][i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0)
        for (int i = 0; i < NV; ++i) v[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// stage 1: per-workgroup fp64 partials of sum and sum of squares per channel: partials[block][2 C] (the C sums, then the C sums of
// squares).  Every value is added to every accumulator, as itself or as 0.0, so the loop has no branch on the channel.
template <int C>
__global__ __launch_bounds__(256) void swd_stats_partial_kernel(const float* __restrict__ desc, long long total, double* __restrict__ partials)
{
    constexpr int DESC = PATCH * C;
    double v[2 * C];
#pragma unroll
    for (int i = 0; i < 2 * C; ++i) v[i] = 0.0;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % DESC) / PATCH;
        const double x = (double)desc[idx], xx = x * x;
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] += c == i ? x : 0.0;
#pragma unroll
        for (int i = 0; i < C; ++i) v[C + i] += c == i ? xx : 0.0;
    }
    block_sum(v);
    if (threadIdx.x == 0)
        for (int i = 0; i < 2 * C; ++i) partials[(size_t)blockIdx.x * (2 * C) + i] = v[i];
}

// stage 2 (one workgroup): stats[0 .. C-1] = mean, stats[C .. 2C-1] = population standard deviation
template <int C>
__global__ __launch_bounds__(256) void swd_stats_final_kernel(const double* __restrict__ partials, int blocks, long long M, float* __restrict__ stats)
{
    double v[2 * C];
#pragma unroll
    for (int i = 0; i < 2 * C; ++i) v[i] = 0.0;
    for (int b = threadIdx.x; b < blocks; b += blockDim.x)
        for (int i = 0; i < 2 * C; ++i) v[i] += partials[(size_t)b * (2 * C) + i];
    block_sum(v);
    if (threadIdx.x == 0) {
        const double n = (double)M * (double)PATCH;
        for (int c = 0; c < C; ++c) {
            const double mean = v[c] / n;
            const double var = v[C + c] / n - mean * mean;
            stats[c] = (float)mean;
            stats[C + c] = (float)sqrt(var > 0.0 ? var : 0.0);
        }
    }
}

template <int C>
__global__ __launch_bounds__(256) void swd_normalize_kernel(float* __restrict__ desc, long long total, const float* __restrict__ stats)
{
    constexpr int DESC = PATCH * C;
    float mean[C], sd[C];
#pragma unroll
    for (int i = 0; i < C; ++i) { mean[i] = stats[i]; sd[i] = stats[C + i]; }
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % DESC) / PATCH;
        float m = mean[C - 1], s = sd[C - 1];
#pragma unroll
        for (int i = C - 2; i >= 0; --i) { m = c == i ? mean[i] : m; s = c == i ? sd[i] : s; }
        desc[idx] = (desc[idx] - m) / s;
    }
}

__global__ __launch_bounds__(256) void swd_l1_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                             double* __restrict__ partials)
{
    double v[1] = {0};
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (long long)gridDim.x * blockDim.x)
        v[0] += (double)fabsf(a[idx] - b[idx]);
    block_sum(v);
    if (threadIdx.x == 0) partials[blockIdx.x] = v[0];
}

__global__ __launch_bounds__(256) void swd_l1_final_kernel(const double* __restrict__ partials, int blocks, long long n, float* __restrict__ out)
{
    double v[1] = {0};
    for (int b = threadIdx.x; b < blocks; b += blockDim.x) v[0] += partials[b];
    block_sum(v);
    if (threadIdx.x == 0) out[0] = (float)(v[0] / (double)n);
}

// ------------------------------------------------------------------------------------------------- projection
// out[d][m] = sum_k desc[m][k] * dirs[k][d].  The MFMA's row index is the direction and its column index the descriptor, so one
// accumulator register of a lane half is 32 consecutive floats of an output row: the transposed store is coalesced as it stands.
//   A operand (lane l): dirs[k = 2s + (l>>5)][d = l&31]   -- read from global (the whole [49 C,K] block is at most 98 KB and stays in cache)
//   B operand (lane l): desc[m = l&31][k = 2s + (l>>5)]   -- from LDS: the workgroup's 128 rows are one contiguous span of desc, copied
//                                                            flat, so the row stride is 49 C floats.  A lane half reads 32 rows at
//                                                            one k.  Padding the even strides 98 and 196 to 99 and 197, which puts
//                                                            those rows in 32 different banks, measured the same time to 0.1 %
//                                                            (docs/experiments_swd.md): the B reads are not what the kernel waits on.
// An odd descriptor length is padded to the next even one with zeros on both operands.  A wave owns 32 descriptors x up to 128
// directions (4 accumulators).  The descriptor length is a template parameter: the k loop has a constant trip count.
typedef float f32x16 __attribute__((ext_vector_type(16)));

// The copy of a FULL workgroup's span from a 16-byte aligned address: N4 float4 per workgroup, at least eight loads in flight per thread before
// the first store (a load per iteration that is waited for before the next is what the plain loop compiles to: one memory latency per
// 256 floats).  Every trip count is a constant, so the groups unroll whole.
template <int N4>
__device__ __forceinline__ void fill_full(float* __restrict__ sd, const float* __restrict__ src)
{
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(sd);
    constexpr int IT = N4 / 256;
#pragma unroll
    for (int b = 0; b < IT; b += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (b + u < IT) v[u] = s4[(b + u) * 256 + threadIdx.x];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (b + u < IT) d4[(b + u) * 256 + threadIdx.x] = v[u];
    }
    if (N4 % 256) {
        const int i = IT * 256 + threadIdx.x;
        if (i < N4) d4[i] = s4[i];
    }
}

template <int C>
__global__ __launch_bounds__(256) void swd_project_kernel(const float* __restrict__ desc, const float* __restrict__ dirs,
                                                          float* __restrict__ out, long long M, int K)
{
    constexpr int DESC = PATCH * C;
    extern __shared__ float4 sd4[];                     // [PJ_M][DESC] floats (declared float4 for its alignment)
    float* sd = reinterpret_cast<float*>(sd4);
    const long long m0 = (long long)blockIdx.x * PJ_M;
    const int d0 = blockIdx.y * PJ_K;
    const long long left = M - m0;
    const int cnt = (int)(left < PJ_M ? left : PJ_M) * DESC;
    const float* src = desc + (size_t)m0 * DESC;
    if (left >= PJ_M && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        fill_full<PJ_M * DESC / 4>(sd, src);
    } else {                                            // the ragged last workgroup, or a base that is not 16-byte aligned
        for (int i = threadIdx.x; i < PJ_M * DESC; i += 256) sd[i] = i < cnt ? src[i] : 0.f;
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const float* brow = sd + (wave * 32 + j) * DESC;
    const int nt = min(4, (K - d0 + 31) >> 5);
    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

#pragma unroll 2
    for (int s = 0; s < (DESC + 1) / 2; ++s) {
        const int k = 2 * s + h;
        const bool kin = (DESC & 1) ? k < DESC : true;
        const float b = kin ? brow[k] : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < nt) {
                const int d = d0 + t * 32 + j;
                const float a = (kin && d < K) ? dirs[(size_t)k * K + d] : 0.f;
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[t], 0, 0, 0);
            }
        }
    }

    const long long m = m0 + wave * 32 + j;
    if (m < M) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < nt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int d = d0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    if (d < K) out[(size_t)d * M + m] = acc[t][r];
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------- sort
// Floats are compared as unsigned keys (sign bit flipped for x >= 0, all bits for x < 0): a total order with -0.0 < +0.0 and the
// key 0xffffffff (a NaN pattern, out of contract) free to pad a short run with.
__device__ __forceinline__ uint32_t to_key(float x)
{
    const uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float from_key(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// One workgroup sorts one run of up to RUN elements of one row in LDS (bitonic network over n2 = the power of two the run is padded to).
// grid (runs of the row, rows).  src == dst is allowed (hence no __restrict__): the run is loaded whole before it is written.
__global__ __launch_bounds__(SORT_THREADS) void swd_sort_runs_kernel(const float* src, float* dst, long long M, int n2)
{
    __shared__ uint32_t sk[RUN];
    const size_t base = (size_t)blockIdx.y * M + (size_t)blockIdx.x * RUN;
    const long long left = M - (long long)blockIdx.x * RUN;
    const int len = (int)(left < RUN ? left : RUN);
    for (int i = threadIdx.x; i < n2; i += SORT_THREADS) sk[i] = i < len ? to_key(src[base + i]) : 0xffffffffu;
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (n2 >> 1); t += SORT_THREADS) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;
                const uint32_t a = sk[i], b = sk[l];
                if ((a > b) == ((i & k) == 0)) { sk[i] = b; sk[l] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < len; i += SORT_THREADS) dst[base + i] = from_key(sk[i]);
}

// how many of the first d outputs of merge(A, B) come from A (ties take A first)
template <typename GetA, typename GetB>
__device__ __forceinline__ int merge_path(GetA ka, int na, GetB kb, int nb, int d)
{
    int lo = d - nb > 0 ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ka(mid) <= kb(d - 1 - mid)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One pass of the global merge: sorted runs of length L are merged in pairs into runs of 2L (the last pair may be short or lack its
// second run).  One workgroup produces TILE consecutive outputs: two threads find where the tile starts and ends in the pair's two
// runs (merge path in global memory), the workgroup loads those TILE inputs into LDS, every thread finds its own MERGE_ITEMS outputs
// there and merges them serially; the tile leaves through LDS so that the store is coalesced.  grid (tiles of the row, rows).
__global__ __launch_bounds__(MERGE_THREADS) void swd_merge_pass_kernel(const float* __restrict__ src, float* __restrict__ dst, long long M, long long L)
{
    __shared__ uint32_t sk[TILE], so[TILE];
    __shared__ int cut[2];
    const float* s = src + (size_t)blockIdx.y * M;
    float* d = dst + (size_t)blockIdx.y * M;
    const long long o0 = (long long)blockIdx.x * TILE;
    const long long base = o0 / (2 * L) * (2 * L);
    const int lenA = (int)(M - base < L ? M - base : L);
    const int lenB = (int)(M - base - lenA < L ? M - base - lenA : L);
    const float* A = s + base;
    const float* B = A + lenA;
    const int tile = (int)(M - o0 < TILE ? M - o0 : TILE);
    const int dg = (int)(o0 - base);
    if (threadIdx.x < 2)
        cut[threadIdx.x] = merge_path([&](int i) { return to_key(A[i]); }, lenA, [&](int i) { return to_key(B[i]); }, lenB,
                                      dg + (threadIdx.x ? tile : 0));
    __syncthreads();
    const int a0 = cut[0], na = cut[1] - a0, b0 = dg - a0, nb = tile - na;
    for (int i = threadIdx.x; i < tile; i += MERGE_THREADS) sk[i] = to_key(i < na ? A[a0 + i] : B[b0 + i - na]);
    __syncthreads();
    const uint32_t* sa = sk;
    const uint32_t* sb = sk + na;
    const int dd = min((int)threadIdx.x * MERGE_ITEMS, tile), de = min(dd + MERGE_ITEMS, tile);
    int ai = merge_path([&](int i) { return sa[i]; }, na, [&](int i) { return sb[i]; }, nb, dd);
    int bi = dd - ai;
    uint32_t ka = ai < na ? sa[ai] : 0xffffffffu, kb = bi < nb ? sb[bi] : 0xffffffffu;
    for (int o = dd; o < de; ++o) {
        const bool take_a = bi >= nb || (ai < na && ka <= kb);
        so[o] = take_a ? ka : kb;
        if (take_a) { ++ai; ka = ai < na ? sa[ai] : 0xffffffffu; }
        else        { ++bi; kb = bi < nb ? sb[bi] : 0xffffffffu; }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < tile; i += MERGE_THREADS) d[o0 + i] = from_key(so[i]);
}

}  // namespace

extern "C" int pg_lap_down(const float* in, float* out, int64_t planes, int S, pg_stream_t stream)
{
    if (!in || !out || planes <= 0 || S < 4 || (S & 1)) return PG_E_ARG;
    hipLaunchKernelGGL(lap_down_kernel, dim3(grid_for(planes * (S / 2) * (S / 2), 256, 65536)), dim3(256), 0, (hipStream_t)stream,
                       in, out, (long long)planes, S);
    return (int)hipGetLastError();
}

extern "C" int pg_lap_up_sub(const float* fine, const float* coarse, float* out, int64_t planes, int S, pg_stream_t stream)
{
    if (!fine || !coarse || !out || planes <= 0 || S < 4 || (S & 1)) return PG_E_ARG;
    hipLaunchKernelGGL(lap_up_sub_kernel, dim3(grid_for(planes * (long long)S * S, 256, 65536)), dim3(256), 0, (hipStream_t)stream,
                       fine, coarse, out, (long long)planes, S);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------- descriptor entry points
// One body per step, instantiated for C = 1..4; the entry points of pggan_hip.h are C = 3, those of pggan_hip_swd.h pick by argument.
namespace {

template <int C>
int gather_c(const float* level, const int32_t* centres, float* out, int64_t ndesc, int P, int S, int64_t row_offset, int64_t out_rows,
             pg_stream_t stream)
{
    if (!level || !centres || !out || ndesc <= 0 || P <= 0 || S < 7 || row_offset < 0 || row_offset + ndesc > out_rows) return PG_E_ARG;
    hipLaunchKernelGGL(swd_gather_kernel<C>, dim3(grid_for(ndesc * (PATCH * C), 256, 65536)), dim3(256), 0, (hipStream_t)stream,
                       level, centres, out, (long long)ndesc, P, S, (long long)row_offset);
    return (int)hipGetLastError();
}

template <int C>
int channel_stats_c(const float* desc, int64_t M, double* partials, float* stats, pg_stream_t stream)
{
    if (!desc || !partials || !stats || M <= 0) return PG_E_ARG;
    const long long total = (long long)M * (PATCH * C);
    const int blocks = grid_for(total, 256 * 8, RED_BLOCKS);
    hipLaunchKernelGGL(swd_stats_partial_kernel<C>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, desc, total, partials);
    hipLaunchKernelGGL(swd_stats_final_kernel<C>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, blocks, (long long)M, stats);
    return (int)hipGetLastError();
}

template <int C>
int normalize_c(float* desc, int64_t M, const float* stats, pg_stream_t stream)
{
    if (!desc || !stats || M <= 0) return PG_E_ARG;
    const long long total = (long long)M * (PATCH * C);
    hipLaunchKernelGGL(swd_normalize_kernel<C>, dim3(grid_for(total, 256, 65536)), dim3(256), 0, (hipStream_t)stream, desc, total, stats);
    return (int)hipGetLastError();
}

template <int C>
int project_c(const float* desc, const float* dirs, float* out, int64_t M, int K, pg_stream_t stream)
{
    if (!desc || !dirs || !out || M <= 0 || K <= 0) return PG_E_ARG;
    const long long gx = (M + PJ_M - 1) / PJ_M, gy = (K + PJ_K - 1) / PJ_K;
    if (gx > 0x7fffffffLL || gy > 65535) return PG_E_UNSUP;
    const size_t smem = (size_t)PJ_M * (PATCH * C) * sizeof(float);
    static std::atomic<uint64_t> smem_set{0};           // devices (by ordinal) on which THIS instantiation's LDS limit has been raised
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return (int)e;
    const uint64_t bit = dev < 64 ? 1ull << dev : 0;
    if (!(smem_set.load(std::memory_order_relaxed) & bit) || !bit) {
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(swd_project_kernel<C>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
            e != hipSuccess)
            return (int)e;
        smem_set.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(swd_project_kernel<C>, dim3((unsigned)gx, (unsigned)gy), dim3(256), smem, (hipStream_t)stream,
                       desc, dirs, out, (long long)M, K);
    return (int)hipGetLastError();
}

// fn<C>(args...) for the run-time C; PG_E_ARG outside 1 .. PG_SWD_MAX_CHANNELS
#define PG_SWD_BY_CHANNELS(C, fn, ...)                                                                                                 \
    ((C) == 1 ? fn<1>(__VA_ARGS__) : (C) == 2 ? fn<2>(__VA_ARGS__) : (C) == 3 ? fn<3>(__VA_ARGS__) : (C) == 4 ? fn<4>(__VA_ARGS__) : PG_E_ARG)
static_assert(PG_SWD_MAX_CHANNELS == 4, "PG_SWD_BY_CHANNELS lists the instantiations");

}  // namespace

extern "C" int pg_swd_gather(const float* level, const int32_t* centres, float* out, int64_t ndesc, int P, int S,
                             int64_t row_offset, int64_t out_rows, pg_stream_t stream)
{
    return gather_c<3>(level, centres, out, ndesc, P, S, row_offset, out_rows, stream);
}

extern "C" int pg_swd_channel_stats(const float* desc, int64_t M, double* partials, float* stats, pg_stream_t stream)
{
    return channel_stats_c<3>(desc, M, partials, stats, stream);
}

extern "C" int pg_swd_normalize(float* desc, int64_t M, const float* stats, pg_stream_t stream)
{
    return normalize_c<3>(desc, M, stats, stream);
}

extern "C" int pg_swd_project(const float* desc, const float* dirs, float* out, int64_t M, int K, pg_stream_t stream)
{
    return project_c<3>(desc, dirs, out, M, K, stream);
}

extern "C" int pg_swd_gather_c(const float* level, const int32_t* centres, float* out, int64_t ndesc, int P, int C, int S,
                               int64_t row_offset, int64_t out_rows, pg_stream_t stream)
{
    return PG_SWD_BY_CHANNELS(C, gather_c, level, centres, out, ndesc, P, S, row_offset, out_rows, stream);
}

extern "C" int pg_swd_channel_stats_c(const float* desc, int64_t M, int C, double* partials, float* stats, pg_stream_t stream)
{
    return PG_SWD_BY_CHANNELS(C, channel_stats_c, desc, M, partials, stats, stream);
}

extern "C" int pg_swd_normalize_c(float* desc, int64_t M, int C, const float* stats, pg_stream_t stream)
{
    return PG_SWD_BY_CHANNELS(C, normalize_c, desc, M, stats, stream);
}

extern "C" int pg_swd_project_c(const float* desc, const float* dirs, float* out, int64_t M, int C, int K, pg_stream_t stream)
{
    return PG_SWD_BY_CHANNELS(C, project_c, desc, dirs, out, M, K, stream);
}

extern "C" int pg_swd_sort_rows(float* buf, float* tmp, int K, int64_t M, pg_stream_t stream)
{
    if (!buf || K <= 0 || K > 65535 || M <= 0 || M > PG_SWD_SORT_MAX_M) return PG_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (M <= RUN) {
        int n2 = 1;
        while (n2 < M) n2 <<= 1;
        hipLaunchKernelGGL(swd_sort_runs_kernel, dim3(1, K), dim3(SORT_THREADS), 0, st, (const float*)buf, buf, (long long)M, n2);
        return (int)hipGetLastError();
    }
    if (!tmp) return PG_E_ARG;
    int passes = 0;
    for (long long L = RUN; L < M; L <<= 1) ++passes;
    float* cur = (passes & 1) ? tmp : buf;              // so that the last pass lands in buf
    hipLaunchKernelGGL(swd_sort_runs_kernel, dim3((unsigned)((M + RUN - 1) / RUN), K), dim3(SORT_THREADS), 0, st,
                       (const float*)buf, cur, (long long)M, RUN);
    for (long long L = RUN; L < M; L <<= 1) {
        float* other = cur == buf ? tmp : buf;
        hipLaunchKernelGGL(swd_merge_pass_kernel, dim3((unsigned)((M + TILE - 1) / TILE), K), dim3(MERGE_THREADS), 0, st,
                           (const float*)cur, other, (long long)M, L);
        cur = other;
    }
    return (int)hipGetLastError();
}

extern "C" int pg_swd_l1(const float* a, const float* b, int64_t n, double* partials, float* out, pg_stream_t stream)
{
    if (!a || !b || !partials || !out || n <= 0) return PG_E_ARG;
    const int blocks = grid_for(n, 256 * 8, RED_BLOCKS);
    hipLaunchKernelGGL(swd_l1_partial_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, b, (long long)n, partials);
    hipLaunchKernelGGL(swd_l1_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, blocks, (long long)n, out);
    return (int)hipGetLastError();
}
