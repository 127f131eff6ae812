// The ends of the random convolutional embedding and the fp64 moments of its features (include/pggan_hip_embed.h):
//   pg_emb_stem_u8_bf16 : uint8 NCHW images -> the 8-channel bf16 NHWC input of the first 3x3 layer
//   pg_emb_pool2_bf16   : 2x2 mean of a bf16 NHWC map, one rounding
//   pg_emb_gap_f32      : mean over the pixels of a bf16 NHWC map in fp32, in row-major order
//   pg_fd_moments_f64   : mean and covariance of a feature matrix in fp64, the covariance on v_mfma_f64_16x16x4_f64
// The layers between the ends are pg_smp_conv3_bf16 (csrc/sampling.hip), which this file does not touch.  No atomics: one writer per
// output element and a fixed order of operations, so two calls give the same bits and the three ends equal tests/fd_ref.py with ==.
//
// The moments.  Rows are cut into slices of SLICE = 256, columns into blocks of TILE = 64; only the T = B (B + 1) / 2 block pairs
// (bi <= bj) on or above the diagonal are computed.  Launch 1 leaves the column sums of every slice, launch 2 the mean, launch 3 one
// TILE x TILE partial of sum_r (x_r - mean)(x_r - mean)^T per (slice, block pair), launch 4 adds the partials in ascending slice order,
// divides and mirrors.
//
// Launch 3.  A workgroup of 4 waves walks its slice in chunks of RC = 32 rows.  Thread (sr, sq) = (tid >> 4, tid & 15) loads the four
// floats of columns 4 sq .. 4 sq + 3 of rows sr and sr + 16 of both column blocks one chunk ahead, and stores (double)x - mean -- or an
// exact zero for a row at or past M or a column at or past F -- into As / Bs [RC][LDP] (a diagonal pair stages one side and reads it
// twice).  LDP = TILE + 16 doubles: consecutive rows start 32 banks apart, so the two rows x 16 columns that half a wave reads in one
// 8-byte access fall on 64 distinct banks.  Wave (wr, wc) owns the 32 x 32 quarter (wr, wc) as 2 x 2 MFMA tiles.  The instruction
// computes D = A B + C with A [16][4] and B [4][16]: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] -- here the centred value
// of data row k0 + (l >> 4) in column (l & 15) of the quarter's row side / column side -- and holds D[(l >> 4) + 4 g][l & 15] in element
// g of its result.  That is NOT the fp32 16x16 map (row 4 (l >> 4) + g).  Four rows per instruction in ascending order: a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_embed.h"

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int STEM_CH = PG_EMB_STEM_CH;
constexpr int SLICE = PG_FD_SLICE, TILE = PG_FD_TILE;
constexpr int RC = 32;                     // rows of one staged chunk
constexpr int LDP = TILE + 16;             // row pitch of the staged operands, in doubles
constexpr int RUN = SLICE / 4;             // rows of one run of the column sums
static_assert(STEM_CH == 8, "one 16-byte store per pixel");
static_assert(TILE == 64 && SLICE % RC == 0 && RC == 32, "the covariance kernel is written for 64 x 64 tiles and 32-row chunks");

inline bool misaligned(const void* p, uintptr_t a = 16) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

inline unsigned grid_for(int64_t threads, int64_t cap = 1 << 20)
{
    const int64_t blocks = (threads + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > cap ? cap : blocks);
}

// Round to nearest even, NaN stays NaN (quiet): the rounding function of csrc/sampling.hip
__device__ __forceinline__ uint32_t rne(float f)
{
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ float lo_f32(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float hi_f32(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// ------------------------------------------------------------------------------------------------------------------------- the ends
__global__ __launch_bounds__(256) void emb_stem_kernel(const uint8_t* __restrict__ x, uint16_t* __restrict__ y, int64_t P, int C, int64_t HW)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += stride) {
        const int64_t m = p / HW;
        const uint8_t* px = x + m * C * HW + (p - m * HW);
        uint32_t o[2] = {0u, 0u};
#pragma unroll
        for (int c = 0; c < PG_EMB_MAX_C; ++c)
            if (c < C) o[c >> 1] |= rne(__fdiv_rn((float)px[c * HW] - 127.5f, 127.5f)) << (16 * (c & 1));
        *reinterpret_cast<uint4*>(y + p * STEM_CH) = make_uint4(o[0], o[1], 0u, 0u);
    }
}

__device__ __forceinline__ uint32_t pool_word(uint32_t a00, uint32_t a01, uint32_t a10, uint32_t a11)
{
    const float lo = ((lo_f32(a00) + lo_f32(a01)) + (lo_f32(a10) + lo_f32(a11))) * 0.25f;
    const float hi = ((hi_f32(a00) + hi_f32(a01)) + (hi_f32(a10) + hi_f32(a11))) * 0.25f;
    return rne(lo) | (rne(hi) << 16);
}

// one thread per 8 channels of an output pixel: four 16-byte loads, one 16-byte store
__global__ __launch_bounds__(256) void emb_pool2_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int64_t total, int Ho, int Wo, int C8)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t Ch = 8 * (int64_t)C8, W = 2 * (int64_t)Wo;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int c8 = (int)(i % C8);
        int64_t q = i / C8;
        const int w = (int)(q % Wo);
        q /= Wo;
        const int h = (int)(q % Ho);
        const int64_t n = q / Ho;
        const uint16_t* p = x + ((n * 2 * Ho + 2 * h) * W + 2 * w) * Ch + 8 * c8;
        const uint4 a00 = *reinterpret_cast<const uint4*>(p), a01 = *reinterpret_cast<const uint4*>(p + Ch);
        const uint4 a10 = *reinterpret_cast<const uint4*>(p + W * Ch), a11 = *reinterpret_cast<const uint4*>(p + W * Ch + Ch);
        *reinterpret_cast<uint4*>(y + i * 8) = make_uint4(pool_word(a00.x, a01.x, a10.x, a11.x), pool_word(a00.y, a01.y, a10.y, a11.y),
                                                          pool_word(a00.z, a01.z, a10.z, a11.z), pool_word(a00.w, a01.w, a10.w, a11.w));
    }
}

// one thread per (image, channel): the pixels in ascending order
__global__ __launch_bounds__(256) void emb_gap_kernel(const uint16_t* __restrict__ x, float* __restrict__ f, int64_t total, int HW, int Ch, float inv)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int64_t n = i / Ch;
        const uint16_t* p = x + n * HW * Ch + (i - n * Ch);
        float s = 0.0f;
        for (int q = 0; q < HW; ++q) s += __uint_as_float((uint32_t)p[(int64_t)q * Ch] << 16);
        f[i] = s * inv;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- the moments
// grid (S, ceil(F / 64)): thread (run, c) adds the rows of run `run` of the slice in column c in ascending order
__global__ __launch_bounds__(256) void fd_colsum_kernel(const float* __restrict__ x, int64_t M, int F, double* __restrict__ colpart)
{
    __shared__ double part[4][64];
    const int run = threadIdx.x >> 6, c = threadIdx.x & 63;
    const int f = blockIdx.y * 64 + c;
    const int64_t r0 = (int64_t)blockIdx.x * SLICE + run * RUN;
    const int64_t r1 = r0 + RUN < M ? r0 + RUN : M;
    double s = 0.0;
    if (f < F)
        for (int64_t r = r0; r < r1; ++r) s += (double)x[r * F + f];
    part[run][c] = s;
    __syncthreads();
    if (run == 0 && f < F) colpart[(int64_t)blockIdx.x * F + f] = ((part[0][c] + part[1][c]) + part[2][c]) + part[3][c];
}

__global__ __launch_bounds__(256) void fd_mean_kernel(const double* __restrict__ colpart, int64_t S, int64_t M, int F, double* __restrict__ mean)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    double s = 0.0;
    for (int64_t k = 0; k < S; ++k) s += colpart[k * F + f];
    mean[f] = s / (double)M;
}

// grid (S, T): the partial of block pair blockIdx.y over slice blockIdx.x
__global__ __launch_bounds__(256) void fd_cov_kernel(const float* __restrict__ x, const double* __restrict__ mean, int64_t M, int F, int B,
                                                     double* __restrict__ covpart)
{
    __shared__ double As[RC * LDP], Bs[RC * LDP];
    int t = blockIdx.y, bi = 0;
    while (t >= B - bi) { t -= B - bi; ++bi; }
    const int bj = bi + t;
    const bool diag = bi == bj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int sr = tid >> 4, sc = 4 * (tid & 15);
    const int ca = bi * TILE + sc, cb = bj * TILE + sc;
    const bool ina = ca < F, inb = !diag && cb < F;            // F % 16 == 0: the four columns of a thread are inside or outside together
    double ma[4] = {0.0, 0.0, 0.0, 0.0}, mb[4] = {0.0, 0.0, 0.0, 0.0};
    if (ina) { ma[0] = mean[ca]; ma[1] = mean[ca + 1]; ma[2] = mean[ca + 2]; ma[3] = mean[ca + 3]; }
    if (inb) { mb[0] = mean[cb]; mb[1] = mean[cb + 1]; mb[2] = mean[cb + 2]; mb[3] = mean[cb + 3]; }
    const int64_t row0 = (int64_t)blockIdx.x * SLICE;
    const int64_t left = M - row0;                             // >= 1: the grid has ceil(M / SLICE) slices
    const int rows = left < SLICE ? (int)left : SLICE;
    const int nchunks = (rows + RC - 1) / RC;                  // chunks past the last row would add exact zeros: skipped
    const double* const Bsrc = diag ? As : Bs;
    float4 ra[2], rb[2];

    auto load = [&](int chunk) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = chunk * RC + sr + 16 * h;
            const bool valid = r < rows;
            ra[h] = rb[h] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ina && valid) ra[h] = *reinterpret_cast<const float4*>(x + (row0 + r) * F + ca);
            if (inb && valid) rb[h] = *reinterpret_cast<const float4*>(x + (row0 + r) * F + cb);
        }
    };
    auto store = [&](int chunk) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = sr + 16 * h;
            const bool valid = chunk * RC + r < rows;
            double* a = As + r * LDP + sc;
            const bool va = ina && valid;
            a[0] = va ? (double)ra[h].x - ma[0] : 0.0; a[1] = va ? (double)ra[h].y - ma[1] : 0.0;
            a[2] = va ? (double)ra[h].z - ma[2] : 0.0; a[3] = va ? (double)ra[h].w - ma[3] : 0.0;
            if (!diag) {
                double* b = Bs + r * LDP + sc;
                const bool vb = inb && valid;
                b[0] = vb ? (double)rb[h].x - mb[0] : 0.0; b[1] = vb ? (double)rb[h].y - mb[1] : 0.0;
                b[2] = vb ? (double)rb[h].z - mb[2] : 0.0; b[3] = vb ? (double)rb[h].w - mb[3] : 0.0;
            }
        }
    };

    v4d acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int fk = lane >> 4, fc = lane & 15;
    load(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        store(chunk);
        __syncthreads();
        if (chunk + 1 < nchunks) load(chunk + 1);
#pragma unroll
        for (int k0 = 0; k0 < RC; k0 += 4) {
            const double* ar = As + (k0 + fk) * LDP + wr * 32 + fc;
            const double* br = Bsrc + (k0 + fk) * LDP + wc * 32 + fc;
            const double a0 = ar[0], a1 = ar[16], b0 = br[0], b1 = br[16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    double* out = covpart + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (TILE * TILE);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                out[(wr * 32 + a * 16 + fk + 4 * g) * TILE + wc * 32 + b * 16 + fc] = acc[a][b][g];
}

// one thread per element of cov; those on or above the diagonal add their partials and write both copies
__global__ __launch_bounds__(256) void fd_finish_kernel(const double* __restrict__ covpart, int64_t S, int64_t M, int F, int B, int T,
                                                        double* __restrict__ cov)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= F * F) return;
    const int i = idx / F, j = idx - i * F;
    if (i > j) return;
    const int bi = i / TILE, bj = j / TILE;
    const int t = bi * B - bi * (bi - 1) / 2 + (bj - bi);
    const double* p = covpart + (int64_t)t * (TILE * TILE) + (i - bi * TILE) * TILE + (j - bj * TILE);
    const int64_t pitch = (int64_t)T * (TILE * TILE);
    double s = 0.0;
    for (int64_t k = 0; k < S; ++k) s += p[k * pitch];
    const double v = s / (double)(M - 1);
    cov[(int64_t)i * F + j] = v;
    cov[(int64_t)j * F + i] = v;
}

}  // namespace

extern "C" int pg_emb_stem_u8_bf16(const uint8_t* x, uint16_t* y, int64_t M, int C, int H, int W, pg_stream_t stream)
{
    if (!x || !y || M <= 0 || H <= 0 || W <= 0 || C < 1 || C > PG_EMB_MAX_C) return PG_E_ARG;
    if (misaligned(x) || misaligned(y)) return PG_E_ALIGN;
    const int64_t HW = (int64_t)H * W;
    if (M >= ((int64_t)1 << 40) / HW) return PG_E_UNSUP;
    const int64_t P = M * HW;
    hipLaunchKernelGGL(emb_stem_kernel, dim3(grid_for(P)), dim3(256), 0, (hipStream_t)stream, x, y, P, C, HW);
    return (int)hipGetLastError();
}

extern "C" int pg_emb_pool2_bf16(const uint16_t* x, uint16_t* y, int64_t N, int H, int W, int Ch, pg_stream_t stream)
{
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || Ch <= 0 || ((H | W) & 1)) return PG_E_ARG;
    if ((Ch & 7) || misaligned(x) || misaligned(y)) return PG_E_ALIGN;
    const int64_t per = (int64_t)(H / 2) * (W / 2) * (Ch / 8);
    if (N >= ((int64_t)1 << 40) / per) return PG_E_UNSUP;
    const int64_t total = N * per;
    hipLaunchKernelGGL(emb_pool2_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, y, total, H / 2, W / 2, Ch / 8);
    return (int)hipGetLastError();
}

extern "C" int pg_emb_gap_f32(const uint16_t* x, float* f, int64_t N, int H, int W, int Ch, pg_stream_t stream)
{
    if (!x || !f || N <= 0 || H <= 0 || W <= 0 || Ch <= 0) return PG_E_ARG;
    if (misaligned(x) || misaligned(f)) return PG_E_ALIGN;
    const int64_t HW = (int64_t)H * W;
    if (HW >= (1 << 24) || N >= ((int64_t)1 << 40) / (HW * Ch)) return PG_E_UNSUP;
    const int64_t total = N * Ch;
    hipLaunchKernelGGL(emb_gap_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, f, total, (int)HW, Ch,
                       1.0f / (float)HW);
    return (int)hipGetLastError();
}

extern "C" int pg_fd_moments_f64(const float* x, int64_t M, int F, double* mean, double* cov, double* scratch, int64_t scratch_doubles,
                                 pg_stream_t stream)
{
    if (!x || !mean || !cov || !scratch || M < 2 || F < PG_FD_MIN_F || F > PG_FD_MAX_F || (F & 15)) return PG_E_ARG;
    if (misaligned(x) || misaligned(mean, 8) || misaligned(cov, 8) || misaligned(scratch, 8)) return PG_E_ALIGN;
    if (M > ((int64_t)1 << 31)) return PG_E_UNSUP;
    const int64_t S = (M + SLICE - 1) / SLICE;
    const int B = (F + TILE - 1) / TILE, T = B * (B + 1) / 2;
    if (scratch_doubles < S * ((int64_t)F + (int64_t)T * TILE * TILE)) return PG_E_ARG;
    double* colpart = scratch;
    double* covpart = scratch + S * F;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fd_colsum_kernel, dim3((unsigned)S, (F + 63) / 64), dim3(256), 0, s, x, M, F, colpart);
    hipLaunchKernelGGL(fd_mean_kernel, dim3((F + 255) / 256), dim3(256), 0, s, colpart, S, M, F, mean);
    hipLaunchKernelGGL(fd_cov_kernel, dim3((unsigned)S, T), dim3(256), 0, s, x, mean, M, F, B, covpart);
    hipLaunchKernelGGL(fd_finish_kernel, dim3((F * F + 255) / 256), dim3(256), 0, s, covpart, S, M, F, B, T, cov);
    return (int)hipGetLastError();
}
