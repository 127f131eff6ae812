// Multi-scale structural similarity between pairs of images (Wang, Simoncelli & Bovik 2003, in the form Karras et al. 2018 use to
// detect loss of variation), evaluated where the generated images already are:
//   pg_msssim_scale  : one scale of every (pair, channel) plane: [quantise ->] 11x11 Gaussian moments -> ssim / cs maps -> per-workgroup
//                      partial sums, plus the 2x2 box mean of both images for the next scale.  Reads two images, writes two quarter-size ones.
//   pg_msssim_finish : the per-workgroup partials of all scales -> per-pair value and per-scale terms, in fp64.
// The reference has no metric: parity is against the published definition, restated for the CPU in tests/msssim_ref.py.
//
// Why VALU and LDS, not MFMA: the filter is separable and each of its two passes is an 11-tap dot product per output, below the K = 16 at
// which a matrix instruction starts to pay, and a banded [T+10] x [T] operand would spend 3/4 of an fp32 MFMA (which runs at the fp32
// VALU rate on gfx950 anyway) on zeros.  What the kernel has to avoid is traffic: five moment planes written and re-read per scale.
// They live in LDS only.
//
// One workgroup of 256 threads owns a TILE x TILE block of one plane: the outputs whose window starts in it and the pixels of it (for
// the pooled image).  The valid sides 6, 22, 54, 118, 246, ... are never a multiple of TILE, but ceil((side - 10) / TILE) * TILE >= side
// for every power-of-two side >= 16, so the tiles that cover the valid outputs also cover every pixel once.
//   1. stage the (TILE+10)^2 halo of a and b in LDS (zero outside the image; quantised on load at scale 0);
//   2. pool: thread t writes the 2x2 mean of its pixel block of a and of b -- ((p00 + p01) + p10) + p11, then x 0.25;
//   3. horizontal pass: work item (row, 8 outputs) reads 18 + 18 samples and leaves the five filtered planes a, b, aa, bb, ab in LDS;
//   4. vertical pass: thread (column, 4 rows) reads 14 x 5 samples, forms both maps at its 4 positions;
//   5. sums of both maps over the valid positions: fp32 over a thread's 4, then fp64 by wave64 shuffles and across the 4 waves in a fixed
//      order; one (ssim, cs) pair of doubles per workgroup.  No atomics anywhere (the library is built with -munsafe-fp-atomics): the
//      same inputs give the same bits, and a pair's value does not depend on its neighbours in the batch.
// LDS: rows of the halo are 43 floats and rows of the filtered planes 33, both odd, so that the 32 lanes of a group of step 3 (8 rows x 4
// segments) and of step 4 (one row) fall in 32 different banks.  42 KB per workgroup: three workgroups per CU.
//
// Precision: the variances are differences of second moments of values up to 255^2.  The pixels are CENTRED before the moments: each
// workgroup subtracts the sample in the middle of its own halo (one value for a, one for b).  Variances and covariance do not change
// under a shift, the means shift back.  On a near-flat image this removes the cancellation; on a textured one it changes nothing.
//
// Exactness: a*b, a*a and b*b are the same __fmul_rn, the five planes go through the same fmaf chains, 2*sab is sab + sab and saa + sbb
// is the same doubling when a == b, so numerator and denominator of both quotients are bit-equal for identical images and the pair's
// value is exactly 1.  Contraction is off for the whole file; every fused operation is an explicit fmaf.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "pggan_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int TILE = PG_MSSSIM_TILE;     // outputs (and owned pixels) per workgroup side
constexpr int WIN = 11;
constexpr int HALO = TILE + WIN - 1;     // 42
constexpr int APITCH = HALO + 1;         // 43
constexpr int HPITCH = TILE + 1;         // 33
constexpr int SEG = 8;                   // outputs of one work item of the horizontal pass
constexpr int VROWS = 4;                 // outputs of one thread of the vertical pass
constexpr int MAX_SCALES = PG_MSSSIM_MAX_SCALES;
static_assert(TILE == 32 && TILE % SEG == 0 && TILE * TILE == 256 * VROWS && (TILE / 2) * (TILE / 2) == 256, "the thread maps below assume a 32x32 tile and 256 threads");
static_assert(WIN - 1 < TILE, "the tiles of the valid outputs must cover every pixel");

struct Taps { float w[WIN]; };
struct Weights { double w[MAX_SCALES]; };

// pg_image_grid_u8's arithmetic: (x - lo) * scale with one rounding each, round half to even, clip.  mode 0: x is already in [0, 255]
// units (a pooled image); 1: map the range only (quantize=False); 2: map, round, clip.
__device__ __forceinline__ float to_level(float x, int mode, float lo, float scale)
{
    if (mode == 0) return x;
    float y = __fmul_rn(__fsub_rn(x, lo), scale);
    if (mode == 2) y = fminf(fmaxf(rintf(y), 0.f), 255.f);
    return y;
}

__global__ __launch_bounds__(256) void msssim_scale_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           float* __restrict__ pool_a, float* __restrict__ pool_b,
                                                           double* __restrict__ partials, int side, int tiles, int mode, float lo,
                                                           float scale, Taps taps)
{
    __shared__ float sa[HALO * APITCH], sb[HALO * APITCH];
    __shared__ float sh[5][HALO * HPITCH];
    __shared__ double red[4][2];

    const int tid = threadIdx.x;
    const long long wg = blockIdx.x;
    const int tx = (int)(wg % tiles);
    const int ty = (int)((wg / tiles) % tiles);
    const size_t plane = (size_t)(wg / ((long long)tiles * tiles));
    const int x0 = tx * TILE, y0 = ty * TILE;
    const float* pa = a + plane * side * side;
    const float* pb = b + plane * side * side;

    // 1. halo
    for (int i = tid; i < HALO * HALO; i += 256) {
        const int r = i / HALO, c = i - r * HALO;
        const int gy = y0 + r, gx = x0 + c;
        float va = 0.f, vb = 0.f;
        if (gy < side && gx < side) {
            const size_t o = (size_t)gy * side + gx;
            va = to_level(pa[o], mode, lo, scale);
            vb = to_level(pb[o], mode, lo, scale);
        }
        sa[r * APITCH + c] = va;
        sb[r * APITCH + c] = vb;
    }
    __syncthreads();

    // 2. pooled images of the owned pixel block (the block lies inside the image in whole 2x2 cells: side and TILE are even)
    if (pool_a) {
        const int px = tid & 15, py = tid >> 4;
        const int gx = x0 + 2 * px, gy = y0 + 2 * py;
        if (gx < side && gy < side) {
            const int hs = side >> 1;
            const size_t o = plane * hs * hs + (size_t)(gy >> 1) * hs + (gx >> 1);
            const float* q = sa + (2 * py) * APITCH + 2 * px;
            pool_a[o] = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(q[0], q[1]), q[APITCH]), q[APITCH + 1]), 0.25f);
            q = sb + (2 * py) * APITCH + 2 * px;
            pool_b[o] = __fmul_rn(__fadd_rn(__fadd_rn(__fadd_rn(q[0], q[1]), q[APITCH]), q[APITCH + 1]), 0.25f);
        }
    }

    // the shift of this workgroup: the middle sample of each halo, inside the image for every tile (HALO / 2 = 21 < 32 pixels of it are)
    const int cr = min(HALO / 2, side - 1 - y0), cc = min(HALO / 2, side - 1 - x0);
    const float ca = sa[cr * APITCH + cc], cb = sb[cr * APITCH + cc];

    // 3. horizontal pass: item = (row, segment of 8 outputs)
    if (tid < HALO * (TILE / SEG)) {
        const int r = tid >> 2, sg = tid & 3;
        const float* ra = sa + r * APITCH + sg * SEG;
        const float* rb = sb + r * APITCH + sg * SEG;
        float acc[SEG][5];
#pragma unroll
        for (int o = 0; o < SEG; ++o)
#pragma unroll
            for (int p = 0; p < 5; ++p) acc[o][p] = 0.f;
#pragma unroll
        for (int j = 0; j < SEG + WIN - 1; ++j) {
            const float va = __fsub_rn(ra[j], ca), vb = __fsub_rn(rb[j], cb);
            const float v[5] = {va, vb, __fmul_rn(va, va), __fmul_rn(vb, vb), __fmul_rn(va, vb)};
#pragma unroll
            for (int o = 0; o < SEG; ++o) {
                const int k = j - o;
                if (k >= 0 && k < WIN) {
#pragma unroll
                    for (int p = 0; p < 5; ++p) acc[o][p] = fmaf(taps.w[k], v[p], acc[o][p]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < 5; ++p)
#pragma unroll
            for (int o = 0; o < SEG; ++o) sh[p][r * HPITCH + sg * SEG + o] = acc[o][p];
    }
    __syncthreads();

    // 4. vertical pass: thread = (column, 4 output rows)
    const int x = tid & (TILE - 1), yb = (tid >> 5) * VROWS;
    float m[VROWS][5];
#pragma unroll
    for (int i = 0; i < VROWS; ++i)
#pragma unroll
        for (int p = 0; p < 5; ++p) m[i][p] = 0.f;
#pragma unroll
    for (int j = 0; j < VROWS + WIN - 1; ++j) {
        float v[5];
#pragma unroll
        for (int p = 0; p < 5; ++p) v[p] = sh[p][(yb + j) * HPITCH + x];
#pragma unroll
        for (int i = 0; i < VROWS; ++i) {
            const int k = j - i;
            if (k >= 0 && k < WIN) {
#pragma unroll
                for (int p = 0; p < 5; ++p) m[i][p] = fmaf(taps.w[k], v[p], m[i][p]);
            }
        }
    }

    const float C1 = (float)(0.01 * 255.0 * 0.01 * 255.0), C2 = (float)(0.03 * 255.0 * 0.03 * 255.0);
    const int valid = side - (WIN - 1);
    float s_ssim = 0.f, s_cs = 0.f;
#pragma unroll
    for (int i = 0; i < VROWS; ++i) {
        // shifted means and the (shift-invariant) second central moments
        const float da = m[i][0], db = m[i][1];
        const float saa = __fsub_rn(m[i][2], __fmul_rn(da, da));
        const float sbb = __fsub_rn(m[i][3], __fmul_rn(db, db));
        const float sab = __fsub_rn(m[i][4], __fmul_rn(da, db));
        const float mua = __fadd_rn(da, ca), mub = __fadd_rn(db, cb);
        const float maa = __fmul_rn(mua, mua), mbb = __fmul_rn(mub, mub), mab = __fmul_rn(mua, mub);
        const float cs = __fdiv_rn(__fadd_rn(__fadd_rn(sab, sab), C2), __fadd_rn(__fadd_rn(saa, sbb), C2));
        const float lum = __fdiv_rn(__fadd_rn(__fadd_rn(mab, mab), C1), __fadd_rn(__fadd_rn(maa, mbb), C1));
        const bool in = (x0 + x < valid) && (y0 + yb + i < valid);
        s_cs = __fadd_rn(s_cs, in ? cs : 0.f);
        s_ssim = __fadd_rn(s_ssim, in ? __fmul_rn(lum, cs) : 0.f);
    }

    // 5. one pair of doubles per workgroup, combined in a fixed order
    double d0 = (double)s_ssim, d1 = (double)s_cs;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        d0 += __shfl_down(d0, off, 64);
        d1 += __shfl_down(d1, off, 64);
    }
    if ((tid & 63) == 0) { red[tid >> 6][0] = d0; red[tid >> 6][1] = d1; }
    __syncthreads();
    if (tid == 0) {
        partials[2 * (size_t)wg] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        partials[2 * (size_t)wg + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
}

__host__ __device__ inline int tiles_of(int side) { return (side - (WIN - 1) + TILE - 1) / TILE; }

// One wave per pair.  partials: per scale (finest first) [n][C][tiles_s^2][2]; a lane sums every 64th entry of its pair's span, the
// lanes combine by shuffles -- a fixed order.  terms[i][s] = mean cs of scale s below the last, mean ssim of the last; value = the
// weighted product of the terms clamped at 0 (a negative mean contrast term of unrelated noise would make a fractional power NaN).
__global__ __launch_bounds__(64) void msssim_finish_kernel(const double* __restrict__ partials, double* __restrict__ values,
                                                           double* __restrict__ terms, long long n, int C, int R, int S, Weights wt)
{
    const long long pair = blockIdx.x;
    const int lane = threadIdx.x;
    size_t base = 0;
    double value = 1.0;
    int side = R;
    for (int s = 0; s < S; ++s, side >>= 1) {
        const int t = tiles_of(side), per_pair = C * t * t;
        const double* p = partials + 2 * (base + (size_t)pair * per_pair);
        double d0 = 0.0, d1 = 0.0;
        for (int e = lane; e < per_pair; e += 64) { d0 += p[2 * e]; d1 += p[2 * e + 1]; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            d0 += __shfl_down(d0, off, 64);
            d1 += __shfl_down(d1, off, 64);
        }
        if (lane == 0) {
            const double valid = (double)(side - (WIN - 1));
            const double count = (double)C * valid * valid;
            const double term = (s == S - 1 ? d0 : d1) / count;
            terms[pair * S + s] = term;
            const double f = term <= 0.0 ? 0.0 : (term == 1.0 ? 1.0 : pow(term, wt.w[s]));
            value *= f;
        }
        base += (size_t)n * per_pair;
    }
    if (lane == 0) values[pair] = value;
}

inline int scales_of(int R)
{
    int lg = 0;
    while ((1 << lg) < R) ++lg;
    return lg - 3 < MAX_SCALES ? lg - 3 : MAX_SCALES;
}

inline bool good_side(int side) { return side >= 16 && side <= 32768 && !(side & (side - 1)); }

}  // namespace

extern "C" int pg_msssim_scale(const float* a, const float* b, float* pool_a, float* pool_b, double* partials, int64_t planes, int side,
                               int mode, float lo, float hi, pg_stream_t stream)
{
    if (!a || !b || !partials || planes <= 0 || !good_side(side) || mode < 0 || mode > 2 || (!pool_a) != (!pool_b)) return PG_E_ARG;
    if (mode != 0 && !(hi > lo)) return PG_E_ARG;
    if (pool_a && side < 32) return PG_E_ARG;                              // a pooled side below 16 has no scale
    const int t = tiles_of(side);
    const long long grid = (long long)planes * t * t;
    if (grid > 0x7fffffffLL) return PG_E_UNSUP;
    static const Taps taps = [] {
        double g[WIN], sum = 0.0;
        for (int i = 0; i < WIN; ++i) { g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += g[i]; }
        Taps r;
        for (int i = 0; i < WIN; ++i) r.w[i] = (float)(g[i] / sum);
        return r;
    }();
    const float scale = mode ? (float)(255.0 / ((double)hi - (double)lo)) : 1.f;
    hipLaunchKernelGGL(msssim_scale_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a, b, pool_a, pool_b, partials, side,
                       t, mode, lo, scale, taps);
    return (int)hipGetLastError();
}

extern "C" int pg_msssim_finish(const double* partials, double* values, double* terms, int64_t n, int C, int R, pg_stream_t stream)
{
    if (!partials || !values || !terms || n <= 0 || n > 0x7fffffffLL || C <= 0 || !good_side(R)) return PG_E_ARG;
    const int S = scales_of(R);
    static const double published[MAX_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    Weights wt;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += published[s];
    for (int s = 0; s < MAX_SCALES; ++s) wt.w[s] = s < S ? published[s] / sum : 0.0;
    hipLaunchKernelGGL(msssim_finish_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, partials, values, terms, (long long)n,
                       C, R, S, wt);
    return (int)hipGetLastError();
}
