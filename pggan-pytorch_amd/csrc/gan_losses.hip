// Loss block of the selectable GAN objectives (include/pggan_hip_gan.h): per-score terms of the WGAN, non-saturating logistic, hinge and
// least-squares objectives with their score gradients, and the R1 penalty with its tangent seed.  The two loss kernels are one wavefront
// with a fixed-order reduction, like pg_d_loss / pg_g_loss (csrc/elementwise.hip); the seed is a float4 stream like pg_gp_seed.
// Every fp32 operation is spelled with a rounding intrinsic: the sequence below is what tests/gan_losses_ref.py charges, whatever the
// compiler would contract.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_gan.h"

namespace {

inline int grid_for(size_t total, int block, int cap)
{
    size_t g = (total + block - 1) / block;
    if (g > (size_t)cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
    return v;
}

// softplus(x) = max(x, 0) + log1p(exp(-|x|)): exp's argument is <= 0, so nothing overflows
__device__ __forceinline__ float softplus(float x)
{
    return __fadd_rn(fmaxf(x, 0.f), log1pf(expf(-fabsf(x))));
}

// its derivative, 1 / (1 + e^-x) for x >= 0 and e^x / (1 + e^x) for x < 0
__device__ __forceinline__ float sigmoid(float x)
{
    const float e = expf(-fabsf(x));
    return __fdiv_rn(x >= 0.f ? 1.f : e, __fadd_rn(1.f, e));
}

// the term of one score and its derivative: `fake` selects F, otherwise R without the drift term (which is L as well)
__device__ __forceinline__ void score_term(int kind, float s, bool fake, float& term, float& dterm)
{
    switch (kind) {
    case PG_GAN_LOGISTIC: {
        const float x = fake ? s : -s;
        term = softplus(x);
        const float sg = sigmoid(x);
        dterm = fake ? sg : -sg;
        break;
    }
    case PG_GAN_HINGE: {
        if (fake) { term = fmaxf(0.f, __fadd_rn(1.f, s)); dterm = s > -1.f ? 1.f : 0.f; }
        else      { term = fmaxf(0.f, __fsub_rn(1.f, s)); dterm = s < 1.f ? -1.f : 0.f; }
        break;
    }
    case PG_GAN_LSGAN: {
        const float t = fake ? s : __fsub_rn(s, 1.f);
        term = __fmul_rn(t, t);
        dterm = __fmul_rn(2.f, t);
        break;
    }
    default:                                         // PG_GAN_WGAN
        term = fake ? s : -s;
        dterm = fake ? 1.f : -1.f;
    }
}

__global__ __launch_bounds__(64) void gan_d_loss_kernel(const float* __restrict__ s, const float* __restrict__ pen,
                                                        float* __restrict__ d_cost, float* __restrict__ d_real,
                                                        float* __restrict__ d_fake, float* __restrict__ gscore,
                                                        int N, int groups, int kind, float drift)
{
    float acc = 0.f;
    const float invn = __fdiv_rn(1.f, (float)N);
    const float drift2 = __fmul_rn(2.f, drift);
    for (int n = threadIdx.x; n < N; n += 64) {
        const float sr = s[n], sf = s[N + n];
        float r, dr, f, df;
        score_term(kind, sr, false, r, dr);
        score_term(kind, sf, true, f, df);
        r = __fadd_rn(r, __fmul_rn(__fmul_rn(sr, sr), drift));
        dr = __fadd_rn(dr, __fmul_rn(drift2, sr));
        d_real[n] = r; d_fake[n] = f;
        float t = __fadd_rn(f, r);
        if (pen) t = __fadd_rn(t, pen[n]);
        acc = __fadd_rn(acc, t);
        gscore[n] = __fmul_rn(dr, invn);
        gscore[N + n] = __fmul_rn(df, invn);
        if (groups == 3) gscore[2 * N + n] = 0.f;
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) d_cost[0] = __fmul_rn(acc, invn);
}

__global__ __launch_bounds__(64) void gan_g_loss_kernel(const float* __restrict__ s, float* __restrict__ g_cost,
                                                        float* __restrict__ gscore, int N, int kind)
{
    float acc = 0.f;
    const float invn = __fdiv_rn(1.f, (float)N);
    const int side = kind == PG_GAN_HINGE ? PG_GAN_WGAN : kind;      // the hinge objective's generator term is -s
    for (int n = threadIdx.x; n < N; n += 64) {
        float l, dl;
        score_term(side, s[n], false, l, dl);
        acc = __fadd_rn(acc, l);
        gscore[n] = __fmul_rn(dl, invn);
    }
    acc = wave_sum(acc);
    if (threadIdx.x == 0) g_cost[0] = __fmul_rn(acc, invn);
}

// u = (inv_n gamma) g over the N E elements as ONE range (the coefficient does not depend on the row, so rows need no alignment of
// their own): float4 over total / 4, the last total mod 4 elements by the first workgroup; pen[n] by the first workgroup as well.
__global__ __launch_bounds__(256) void r1_seed_kernel(const float* __restrict__ g, const float* __restrict__ ss,
                                                      float* __restrict__ pen, float* __restrict__ u, int N, size_t total,
                                                      float half_gamma, float coef)
{
    const size_t block = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const size_t stride = (size_t)gridDim.x * gridDim.y * blockDim.x;
    const size_t total4 = total >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    float4* u4 = reinterpret_cast<float4*>(u);
    for (size_t i = block * blockDim.x + threadIdx.x; i < total4; i += stride) {
        const float4 v = g4[i];
        u4[i] = make_float4(__fmul_rn(v.x, coef), __fmul_rn(v.y, coef), __fmul_rn(v.z, coef), __fmul_rn(v.w, coef));
    }
    if (block == 0) {
        const size_t tail0 = total4 << 2;
        if (threadIdx.x < total - tail0) u[tail0 + threadIdx.x] = __fmul_rn(g[tail0 + threadIdx.x], coef);
        for (int n = threadIdx.x; n < N; n += blockDim.x) pen[n] = __fmul_rn(half_gamma, ss[n]);
    }
}

}  // namespace

#define LAUNCH(kern, grid, block, smem, stream, ...) \
    hipLaunchKernelGGL(kern, grid, block, smem, (hipStream_t)(stream), __VA_ARGS__); \
    return (int)hipGetLastError()

static bool known_kind(int kind) { return kind >= PG_GAN_WGAN && kind <= PG_GAN_LSGAN; }

extern "C" int pg_gan_d_loss(const float* s, const float* pen, float* d_cost, float* d_real, float* d_fake, float* gscore, int N,
                             int groups, int kind, float drift, pg_stream_t stream)
{
    if (!s || !d_cost || !d_real || !d_fake || !gscore || N <= 0 || (groups != 2 && groups != 3) || !known_kind(kind)) return PG_E_ARG;
    LAUNCH(gan_d_loss_kernel, dim3(1), dim3(64), 0, stream, s, pen, d_cost, d_real, d_fake, gscore, N, groups, kind, drift);
}

extern "C" int pg_gan_g_loss(const float* s, float* g_cost, float* gscore, int N, int kind, pg_stream_t stream)
{
    if (!s || !g_cost || !gscore || N <= 0 || !known_kind(kind)) return PG_E_ARG;
    LAUNCH(gan_g_loss_kernel, dim3(1), dim3(64), 0, stream, s, g_cost, gscore, N, kind);
}

extern "C" int pg_r1_seed(const float* g, const float* ss, float* pen, float* u, int N, int64_t E, float gamma, float inv_n,
                          pg_stream_t stream)
{
    if (!g || !ss || !pen || !u || N <= 0 || E <= 0) return PG_E_ARG;
    if (((uintptr_t)g | (uintptr_t)u) & 15) return PG_E_ALIGN;
    LAUNCH(r1_seed_kernel, dim3(grid_for(((size_t)E + 3) >> 2, 256, 1024), N), dim3(256), 0, stream, g, ss, pen, u, N,
           (size_t)N * (size_t)E, 0.5f * gamma, inv_n * gamma);
}
