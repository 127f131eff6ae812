// Image loss of the latent projection (include/pggan_hip_projection.h): the multi-resolution squared error between two image batches and
// its gradient with respect to the first.  Everything between the fp32 loads and the one fp32 rounding per output is fp64 in a fixed
// order; there are no atomics.
//
// A workgroup of 256 threads takes one level-0 tile of min(r, 64) pixels on a side of one image plane.  A thread holds a 4x4 patch of
// e = img - target in registers (four float4 rows of either tensor), so levels 0, 1 and 2 of the box-mean pyramid are register
// arithmetic; levels 3 .. 6 of the tile (8x8 .. 1x1 cells) are built in LDS, 341 doubles.  Up to r = 256 no cell is larger than a tile
// and the gradient is complete in this one pass.  At 512 and 1024 the cells of levels 7 and 8 span 2x2 and 4x4 tiles: the first pass
// leaves every tile's mean in a compact fp64 pyramid, pyr_finish_kernel (one workgroup per sample, which sums the loss in any case)
// builds those cells from it, and a second tile pass re-reads the images and writes the gradient, once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_projection.h"

namespace {

constexpr int kTileLevels = 7;                        // levels 0 .. 6 can lie inside a 64-pixel tile

struct PyrParams {
    double coef[PG_PYR_MAX_LEVELS];                   // w_l * 2 / (C r_l^2) * 4^-l: gradient of level l per unit of P_l; 0 = level skipped
    double lw[PG_PYR_MAX_LEVELS];                     // w_l / (C r_l^2): loss of level l per unit of its sum of squares
    int r, C, T, tps, lt, nlev;                       // side, channels, tile side, tiles per side, log2(T), levels of the pyramid
};

// offset of level l (2 .. 6) of a tile in the LDS pyramid: sides 16, 8, 4, 2, 1 at the most
__device__ __forceinline__ int lds_off(int l)
{
    return l == 2 ? 0 : l == 3 ? 256 : l == 4 ? 320 : l == 5 ? 336 : 340;
}

__device__ __forceinline__ double mean4(double a, double b, double c, double d)
{
    return 0.25 * ((a + b) + (c + d));
}

__device__ __forceinline__ double wave_sum_down(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;                                         // lane 0 holds the sum
}

// sum of v over the 256 threads in a fixed order, returned to every thread; red: 4 doubles of LDS
__device__ __forceinline__ double block_sum(double v, double* red)
{
    v = wave_sum_down(v);
    __syncthreads();                                  // (a previous use of red has been read)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

template <bool FIRST, bool GRAD>
__global__ __launch_bounds__(256) void pyr_tile_kernel(const float* __restrict__ img, const float* __restrict__ tgt,
                                                       float* __restrict__ grad, double* __restrict__ part, double* __restrict__ top,
                                                       const double* __restrict__ span, const PyrParams p)
{
    __shared__ double lv[341];
    __shared__ double red[4][kTileLevels];
    const int t = threadIdx.x;
    const int tpr = p.T >> 2;                         // threads per tile side
    const unsigned ntiles = (unsigned)(p.tps * p.tps);
    const unsigned plane = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const int tyi = (int)(tile / (unsigned)p.tps), txi = (int)(tile % (unsigned)p.tps);
    const bool active = t < tpr * tpr;
    const int ty = active ? t / tpr : 0, tx = active ? t % tpr : 0;
    const size_t base = (size_t)plane * p.r * p.r + (size_t)(tyi * p.T + 4 * ty) * p.r + (size_t)(txi * p.T + 4 * tx);

    double e[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (active) {
            a = *reinterpret_cast<const float4*>(img + base + (size_t)i * p.r);
            b = *reinterpret_cast<const float4*>(tgt + base + (size_t)i * p.r);
        }
        e[i][0] = (double)a.x - (double)b.x;
        e[i][1] = (double)a.y - (double)b.y;
        e[i][2] = (double)a.z - (double)b.z;
        e[i][3] = (double)a.w - (double)b.w;
    }
    double q[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) q[i][j] = mean4(e[2 * i][2 * j], e[2 * i][2 * j + 1], e[2 * i + 1][2 * j], e[2 * i + 1][2 * j + 1]);
    const double m = mean4(q[0][0], q[0][1], q[1][0], q[1][1]);

    double acc[kTileLevels];
#pragma unroll
    for (int l = 0; l < kTileLevels; ++l) acc[l] = 0.0;
    if (FIRST) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[0] += e[i][j] * e[i][j];
        acc[1] = (q[0][0] * q[0][0] + q[0][1] * q[0][1]) + (q[1][0] * q[1][0] + q[1][1] * q[1][1]);
        acc[2] = m * m;
    }

    // levels 2 .. min(6, log2 T) of the tile in LDS
    if (active) lv[ty * tpr + tx] = m;
    int side = tpr;
#pragma unroll
    for (int l = 3; l < kTileLevels; ++l) {
        if (l <= p.lt) {                              // (uniform)
            __syncthreads();
            const int ps = side;
            side >>= 1;
            if (t < side * side) {
                const int y = t / side, x = t % side;
                const double* s = lv + lds_off(l - 1) + (2 * y) * ps + 2 * x;
                const double v = mean4(s[0], s[1], s[ps], s[ps + 1]);
                lv[lds_off(l) + t] = v;
                if (FIRST) acc[l] = v * v;
            }
        }
    }
    __syncthreads();

    if (FIRST) {
#pragma unroll
        for (int l = 0; l < kTileLevels; ++l) {
            const double s = wave_sum_down(acc[l]);
            if ((t & 63) == 0) red[t >> 6][l] = s;
        }
        __syncthreads();
        const size_t pt = (size_t)plane * ntiles + tile;
        if (t < kTileLevels) part[pt * kTileLevels + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        if (t == 0 && p.lt == 6) top[pt] = lv[lds_off(6)];
    }

    if (GRAD) {
        if (!active) return;
        // the levels this thread's whole patch shares, in ascending order; a level with coefficient 0 is skipped, never multiplied
        double tail = 0.0;
        if (p.coef[2] != 0.0) tail += p.coef[2] * m;
        int sh = 0;
#pragma unroll
        for (int l = 3; l < kTileLevels; ++l) {
            ++sh;
            if (l <= p.lt && p.coef[l] != 0.0) {
                const int sd = tpr >> sh;
                tail += p.coef[l] * lv[lds_off(l) + (ty >> sh) * sd + (tx >> sh)];
            }
        }
        if (p.nlev > kTileLevels) {                   // cells of 2x2 (and 4x4) tiles, from pyr_finish_kernel
            const double* sp = span + (size_t)plane * ntiles;
            const int s7 = p.tps >> 1;
            if (p.coef[7] != 0.0) tail += p.coef[7] * sp[(tyi >> 1) * s7 + (txi >> 1)];
            if (p.nlev > 8 && p.coef[8] != 0.0) tail += p.coef[8] * sp[(ntiles >> 2) + (unsigned)((tyi >> 2) * (s7 >> 1) + (txi >> 2))];
        }
        const double c0 = p.coef[0], c1 = p.coef[1];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double g = 0.0;
                if (c0 != 0.0) g += c0 * e[i][j];
                if (c1 != 0.0) g += c1 * q[i >> 1][j >> 1];
                g += tail;
                o[j] = (float)g;
            }
            *reinterpret_cast<float4*>(grad + base + (size_t)i * p.r) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// One workgroup per sample: the loss from the tiles' sums of squares, and (r >= 512) the cells of levels 7 and 8 from the tiles' means.
__global__ __launch_bounds__(256) void pyr_finish_kernel(const double* __restrict__ part, const double* __restrict__ top,
                                                         double* __restrict__ span, float* __restrict__ loss, const PyrParams p)
{
    __shared__ double red[4];
    __shared__ double c7[64];
    const int t = threadIdx.x;
    const unsigned ntiles = (unsigned)(p.tps * p.tps);
    const unsigned count = (unsigned)p.C * ntiles;    // (plane, tile) pairs of this sample
    const size_t first = (size_t)blockIdx.x * count;
    double total = 0.0;
    const int nin = p.nlev < kTileLevels ? p.nlev : kTileLevels;
    for (int l = 0; l < nin; ++l) {
        if (p.lw[l] == 0.0) continue;                 // (uniform)
        double v = 0.0;
        for (unsigned i = t; i < count; i += 256) v += part[(first + i) * kTileLevels + l];
        total += p.lw[l] * block_sum(v, red);
    }
    if (p.nlev > kTileLevels) {
        const int s7 = p.tps >> 1, n7 = s7 * s7;      // 4x4 or 8x8 cells
        const int s8 = s7 >> 1, n8 = p.nlev > 8 ? s8 * s8 : 0;
        double a7 = 0.0, a8 = 0.0;
        for (int c = 0; c < p.C; ++c) {
            const size_t pl = ((size_t)blockIdx.x * p.C + c) * ntiles;
            __syncthreads();                          // (c7 of the previous channel has been read)
            if (t < n7) {
                const int y = t / s7, x = t % s7;
                const double* s = top + pl + (size_t)(2 * y) * p.tps + 2 * x;
                const double v = mean4(s[0], s[1], s[p.tps], s[p.tps + 1]);
                c7[t] = v;
                span[pl + t] = v;
                a7 += v * v;
            }
            __syncthreads();
            if (t < n8) {
                const int y = t / s8, x = t % s8;
                const double* s = c7 + (2 * y) * s7 + 2 * x;
                const double v = mean4(s[0], s[1], s[s7], s[s7 + 1]);
                span[pl + (ntiles >> 2) + t] = v;
                a8 += v * v;
            }
        }
        const double sum7 = block_sum(a7, red);
        if (p.lw[7] != 0.0) total += p.lw[7] * sum7;
        if (p.nlev > 8) {
            const double sum8 = block_sum(a8, red);
            if (p.lw[8] != 0.0) total += p.lw[8] * sum8;
        }
    }
    if (t == 0) loss[blockIdx.x] = (float)total;
}

inline int ilog2(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

}  // namespace

extern "C" int pg_pyr_loss_grad(const float* img, const float* target, const float* weights, int nlevels, float* grad, float* loss,
                                double* scratch, size_t scratch_bytes, int N, int C, int r, pg_stream_t stream)
{
    if (!img || !target || !loss || !scratch || N < 1 || C < 1 || r < 4 || (r & (r - 1))) return PG_E_ARG;
    if (r > PG_PYR_MAX_SIDE || C > PG_PYR_MAX_C) return PG_E_UNSUP;
    PyrParams p;
    p.r = r;
    p.C = C;
    p.T = r < PG_PYR_TILE ? r : PG_PYR_TILE;
    p.tps = r / p.T;
    p.lt = ilog2(p.T);
    p.nlev = ilog2(r) - 1;                            // levels 0 .. log2(r / 4)
    if (nlevels < 0 || nlevels > p.nlev || (weights != nullptr) != (nlevels > 0)) return PG_E_ARG;
    for (int l = 0; l < PG_PYR_MAX_LEVELS; ++l) {
        double w = 0.0;
        if (l < p.nlev) w = weights ? (l < nlevels ? (double)weights[l] : 0.0) : 1.0;
        if (!(w >= 0.0) || w > 3.0e38) return PG_E_ARG;            // negative, NaN, infinite
        const double rl = (double)(r >> l);
        p.lw[l] = l < p.nlev ? w / ((double)C * rl * rl) : 0.0;
        p.coef[l] = p.lw[l] * 2.0 / (double)(1LL << (2 * l));
    }
    const size_t ntiles = (size_t)p.tps * p.tps;
    const size_t pairs = (size_t)N * C * ntiles;
    if (pairs > 0x7fffffffULL) return PG_E_UNSUP;
    if (scratch_bytes < pairs * PG_PYR_SCRATCH_PER_TILE * sizeof(double)) return PG_E_ARG;
    if (((uintptr_t)img | (uintptr_t)target | (uintptr_t)grad | (uintptr_t)scratch) & 15) return PG_E_ALIGN;
    double* part = scratch;
    double* top = part + pairs * kTileLevels;
    double* span = top + pairs;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)pairs), block(256);
    const bool two_pass = grad && p.nlev > kTileLevels;            // cells larger than a tile: the gradient needs every tile's mean first
    if (grad && !two_pass)
        hipLaunchKernelGGL((pyr_tile_kernel<true, true>), grid, block, 0, s, img, target, grad, part, top, span, p);
    else
        hipLaunchKernelGGL((pyr_tile_kernel<true, false>), grid, block, 0, s, img, target, grad, part, top, span, p);
    hipLaunchKernelGGL(pyr_finish_kernel, dim3((unsigned)N), block, 0, s, part, top, span, loss, p);
    if (two_pass)
        hipLaunchKernelGGL((pyr_tile_kernel<false, true>), grid, block, 0, s, img, target, grad, part, top, span, p);
    return (int)hipGetLastError();
}
