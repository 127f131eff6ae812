// The bf16 sampling path (include/pggan_hip_sampling.h): a forward-only generator on the bf16 matrix cores.
//   cast       fp32 -> bf16, round to nearest even (the weight twin of the flat parameter buffer, the output of block 0's c1)
//   conv3      3x3 pad-1 layer, NHWC bf16 in, bf16 or fp32 out: implicit GEMM on v_mfma_f32_16x16x32_bf16 with the equalized-lr
//              constant, bias, LeakyReLU and (where a wave holds every cout of its pixels) PixelNorm in the fp32 epilogue
//   pixelnorm  fp32 -> bf16, for the layers whose PixelNorm the conv could not fuse
//   torgb      bf16 activations -> the fp32 NCHW image, with the fade-in blend of the previous stage's toRGB
// Owns the contract's device side: ONE rounding per stored activation (rne below), fp32 accumulation, no atomics, one writer per
// output element and a fixed summation order.  None of the fp32 conv kernels is involved.
//
// conv3, the implicit GEMM: M = cout (the MFMA's A rows: 16 NT per workgroup), N = output pixels (B columns: 64 PF per workgroup, 16 PF
// per wave, PF = 1, 2, 4, 8 by the size of the map: dispatch_conv3), K = (tap, cin).  With NHWC activations and [tap][Cout][Cin] weights a lane's 8-element fragment is 8 consecutive
// channels of one tap in both operands: one 16-byte LDS read.  K is walked in units of such 8-channel groups, q = tap * (kc / 8) +
// c8 inside a chunk of kc <= 32 input channels; the four 16-lane groups of a wave take q = 4 s + g in k-step s and groups past the
// chunk's 9 kc / 8 contribute zero fragments.  So a 32-channel chunk is 9 k-steps of one tap each, and Cin = 8 (the 1024^2 stage) is
// 3 k-steps of 4 taps with K = 72 padded to 96.  The accumulator has the pixel on the lane (lane & 15) and 4 consecutive couts in
// its registers (row = 4 (lane >> 4) + reg), so the epilogue stores 8 or 16 bytes per lane and a pixel's sum of squares is two lane
// shuffles away.  LDS rows (a halo pixel's or a weight row's chunk) are padded by 16 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_sampling.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BPX = 64;                       // output pixels of a workgroup: TN images x TH x TW
constexpr int KC = 32;                        // input channels of a chunk
constexpr int KCP = KC + 8;                   // LDS row stride in bf16 elements
constexpr int LDS_MAX = 160 * 1024;           // a CU's LDS: the most a launch may ask for
constexpr int MIN_WORKGROUPS = 512;           // two per CU: below that a smaller tile is taken
constexpr int PERSIST_GRID = 2048;            // workgroups of a single-chunk layer: each keeps its weights in LDS over its tiles

static_assert(PG_SMP_PIXELNORM_MAX_COUT == 128, "the widest instantiation of smp_conv3_kernel is 8 x 16 couts");

// Round to nearest even, NaN stays NaN (quiet): the one rounding function of the path
__device__ __forceinline__ uint32_t rne(float f)
{
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ uint2 rne4(float a, float b, float c, float d)
{
    return make_uint2(rne(a) | (rne(b) << 16), rne(c) | (rne(d) << 16));
}

__global__ __launch_bounds__(256) void smp_cast_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, int64_t n)
{
    const int64_t n4 = n >> 2, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<uint2*>(y)[i] = rne4(v.x, v.y, v.z, v.w);
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < (int)(n & 3)) {
        const int64_t j = (n4 << 2) + threadIdx.x;
        y[j] = (uint16_t)rne(x[j]);
    }
}

struct SmpConv {
    const uint16_t* x; const uint16_t* w; const float* bias; void* y;
    int N, Hin, Win, H, W, Cin, Cout;
    int lgTW, lgTH, TN, tilesW, tilesH, ntiles, kcp;
    int ups, pixelnorm, out_f32;
    float scale, slope, eps;
};

// NT cout fragments x PF pixel fragments per wave: a workgroup takes 64 PF output pixels (TN images x TH x TW) x 16 NT couts.  LDS
// (dynamic): the weights of a chunk [tap][16 NT couts][kcp], then the halo tile [TN][TH + 2][TW + 2][kcp], kcp = min(Cin, 32) + 8.
template <int NT, int PF>
__global__ __launch_bounds__(256) void smp_conv3_kernel(SmpConv p)
{
    constexpr int BN = 16 * NT;
    extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
    const int kcp = p.kcp;
    uint16_t* const wl = lds;
    uint16_t* const xl = lds + 9 * BN * kcp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, g = lane >> 4;
    const int TW = 1 << p.lgTW, TH = 1 << p.lgTH, HW = TW + 2, HH = TH + 2;
    const int halo = p.TN * HH * HW;
    const int cob = blockIdx.y * BN;
    const int nchunks = (p.Cin + KC - 1) / KC;
    // this lane's pixels of the tile (the B columns of its wave's PF fragments) and the halo index of their tap (0, 0)
    int pbase[PF];
#pragma unroll
    for (int f = 0; f < PF; ++f) {
        const int m = (wave * PF + f) * 16 + li;
        const int tx = m & (TW - 1), ty = (m >> p.lgTW) & (TH - 1), tn = m >> (p.lgTW + p.lgTH);
        pbase[f] = (tn * HH + ty) * HW + tx;
    }
    bool weights_staged = false;

    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int tw0 = (tile % p.tilesW) << p.lgTW;
        const int th0 = ((tile / p.tilesW) % p.tilesH) << p.lgTH;
        const int n0 = (tile / (p.tilesW * p.tilesH)) * p.TN;
        f32x4 acc[PF][NT];
#pragma unroll
        for (int f = 0; f < PF; ++f)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int ch = 0; ch < nchunks; ++ch) {
            const int c0 = ch * KC;
            const int kc8 = min(KC, p.Cin - c0) >> 3;                 // 8-channel groups of this chunk: 1 .. 4
            __syncthreads();                                           // the last k-loop has read its LDS
            if (nchunks > 1 || !weights_staged) {
                for (int i = tid; i < 9 * BN * kc8; i += 256) {
                    const int c8 = i % kc8, r = i / kc8;               // r = tap * BN + cout of the tile
                    const int co = cob + (r & (BN - 1)), tap = r / BN;
                    uint4 v = make_uint4(0u, 0u, 0u, 0u);
                    if (co < p.Cout) v = *reinterpret_cast<const uint4*>(p.w + ((size_t)tap * p.Cout + co) * p.Cin + c0 + c8 * 8);
                    *reinterpret_cast<uint4*>(wl + r * kcp + c8 * 8) = v;
                }
                weights_staged = true;
            }
            for (int i = tid; i < halo * kc8; i += 256) {
                const int c8 = i % kc8, hp = i / kc8;
                const int hx = hp % HW, q = hp / HW;
                const int hy = q % HH, n = n0 + q / HH;
                const int gy = th0 + hy - 1, gx = tw0 + hx - 1;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (n < p.N && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
                    const int sy = p.ups ? gy >> 1 : gy, sx = p.ups ? gx >> 1 : gx;
                    v = *reinterpret_cast<const uint4*>(p.x + (((size_t)n * p.Hin + sy) * p.Win + sx) * p.Cin + c0 + c8 * 8);
                }
                *reinterpret_cast<uint4*>(xl + hp * kcp + c8 * 8) = v;
            }
            __syncthreads();

            // a chunk's 9 kc products are summed on their own and then added to the total: two levels keep the fp32 rounding error of a
            // K = 4608 layer at that of a blocked CPU sum (one running accumulator measured 2.5x the 3 e32 bound of the tests)
            f32x4 part[PF][NT];
#pragma unroll
            for (int f = 0; f < PF; ++f)
#pragma unroll
                for (int t = 0; t < NT; ++t) part[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int steps = (9 * kc8 + 3) >> 2;
            int tap = 0, c8 = g;
            while (c8 >= kc8) { c8 -= kc8; ++tap; }
            for (int s = 0; s < steps; ++s) {
                const bool valid = tap < 9;
                const int tp = valid ? tap : 8;
                const int kh = (tp * 11) >> 5, kw = tp - 3 * kh;       // tp / 3, tp % 3 for tp < 9
                const int xoff = (kh * HW + kw) * kcp + c8 * 8;
                bf16x8 b[PF], a[NT];
#pragma unroll
                for (int f = 0; f < PF; ++f) {
                    b[f] = *reinterpret_cast<const bf16x8*>(xl + pbase[f] * kcp + xoff);
                    if (!valid) b[f] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                }
                const uint16_t* wrow = wl + (tp * BN + li) * kcp + c8 * 8;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    a[t] = *reinterpret_cast<const bf16x8*>(wrow + t * 16 * kcp);
                    if (!valid) a[t] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
                }
#pragma unroll
                for (int f = 0; f < PF; ++f)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        part[f][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], b[f], part[f][t], 0, 0, 0);
                c8 += 4;
                while (c8 >= kc8) { c8 -= kc8; ++tap; }
            }
#pragma unroll
            for (int f = 0; f < PF; ++f)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[f][t] += part[f][t];
        }

        // epilogue: x c + bias, LeakyReLU, PixelNorm over the couts of the lane's pixel, one rounding
#pragma unroll
        for (int f = 0; f < PF; ++f) {
            const int m = (wave * PF + f) * 16 + li;
            const int tx = m & (TW - 1), ty = (m >> p.lgTW) & (TH - 1), tn = m >> (p.lgTW + p.lgTH);
            const int n = n0 + tn;
            const size_t pix = ((size_t)n * p.H + th0 + ty) * p.W + tw0 + tx;
            float ss = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int co = cob + t * 16 + g * 4;
                const bool in = co < p.Cout;
                float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
                if (in && p.bias) bv = *reinterpret_cast<const float4*>(p.bias + co);
                const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[f][t][r] * p.scale + bb[r];
                    v = v > 0.f ? v : v * p.slope;
                    if (!in) v = 0.f;
                    acc[f][t][r] = v;
                    ss += v * v;
                }
            }
            float inv = 1.f;
            if (p.pixelnorm) {                                        // (every lane of the wave is here: the shuffles are whole)
                ss += __shfl_xor(ss, 16);
                ss += __shfl_xor(ss, 32);
                inv = 1.f / sqrtf(ss / (float)p.Cout + p.eps);
            }
            if (n < p.N) {
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const int co = cob + t * 16 + g * 4;
                    if (co >= p.Cout) continue;
                    const float v0 = acc[f][t][0] * inv, v1 = acc[f][t][1] * inv, v2 = acc[f][t][2] * inv, v3 = acc[f][t][3] * inv;
                    if (p.out_f32)
                        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.y) + pix * p.Cout + co) = make_float4(v0, v1, v2, v3);
                    else
                        *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(p.y) + pix * p.Cout + co) = rne4(v0, v1, v2, v3);
                }
            }
        }
    }
}

// One wave per pixel: the sum of squares over lanes in a fixed order, then x / sqrt(mean + eps), one rounding
__global__ __launch_bounds__(256) void smp_pixelnorm_kernel(const float* __restrict__ x, uint16_t* __restrict__ y, int64_t P, int C, float eps)
{
    const int lane = threadIdx.x & 63;
    const int64_t px = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (px >= P) return;                                              // (a whole wave leaves)
    const float4* row = reinterpret_cast<const float4*>(x + px * C);
    float ss = 0.f;
    for (int i = lane; i < (C >> 2); i += 64) {
        const float4 v = row[i];
        ss += v.x * v.x; ss += v.y * v.y; ss += v.z * v.z; ss += v.w * v.w;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) ss += __shfl_xor(ss, off);
    const float inv = 1.f / sqrtf(ss / (float)C + eps);
    uint2* out = reinterpret_cast<uint2*>(y + px * C);
    for (int i = lane; i < (C >> 2); i += 64) {
        const float4 v = row[i];
        out[i] = rne4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
    }
}

__device__ __forceinline__ float bf16_bits_to_f32(uint32_t b) { return __uint_as_float(b << 16); }

// sum_ci w[c][ci] x[ci] for the C image channels of one pixel: 8 partial sums per channel (one per position of the 8-channel
// piece), combined pairwise -- a fixed order whose rounding error grows with Cin / 8, not Cin
template <int C>
__device__ __forceinline__ void torgb_dot(const uint16_t* __restrict__ x, const float* __restrict__ w, int Cin, float (&out)[C])
{
    float a[C][8];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) a[c][j] = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += 8) {
        const uint4 v = *reinterpret_cast<const uint4*>(x + c0);
        const float f[8] = {bf16_bits_to_f32(v.x & 0xffffu), bf16_bits_to_f32(v.x >> 16), bf16_bits_to_f32(v.y & 0xffffu), bf16_bits_to_f32(v.y >> 16),
                            bf16_bits_to_f32(v.z & 0xffffu), bf16_bits_to_f32(v.z >> 16), bf16_bits_to_f32(v.w & 0xffffu), bf16_bits_to_f32(v.w >> 16)};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float4 w0 = *reinterpret_cast<const float4*>(w + (size_t)c * Cin + c0);
            const float4 w1 = *reinterpret_cast<const float4*>(w + (size_t)c * Cin + c0 + 4);
            a[c][0] = fmaf(f[0], w0.x, a[c][0]); a[c][1] = fmaf(f[1], w0.y, a[c][1]);
            a[c][2] = fmaf(f[2], w0.z, a[c][2]); a[c][3] = fmaf(f[3], w0.w, a[c][3]);
            a[c][4] = fmaf(f[4], w1.x, a[c][4]); a[c][5] = fmaf(f[5], w1.y, a[c][5]);
            a[c][6] = fmaf(f[6], w1.z, a[c][6]); a[c][7] = fmaf(f[7], w1.w, a[c][7]);
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
        out[c] = ((a[c][0] + a[c][1]) + (a[c][2] + a[c][3])) + ((a[c][4] + a[c][5]) + (a[c][6] + a[c][7]));
}

struct SmpRgb {
    const uint16_t* x; const float* w; const float* bias; float scale, out_mul;
    const uint16_t* px; const float* pw; const float* pbias; float pscale, prev_mul; int PCin;
    float* img; int N, H, W, Cin;
};

// One thread per pixel: the image rows are written coalesced, channel plane by channel plane
template <int C>
__global__ __launch_bounds__(256) void smp_torgb_kernel(SmpRgb p)
{
    const int64_t hw = (int64_t)p.H * p.W;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.N * hw) return;
    const int64_t n = idx / hw, r = idx - n * hw;
    float s[C];
    torgb_dot<C>(p.x + idx * p.Cin, p.w, p.Cin, s);
    float ps[C];
    if (p.px) {
        const int h = (int)(r / p.W), w = (int)(r - (int64_t)h * p.W);
        const int64_t pidx = (n * (p.H >> 1) + (h >> 1)) * (p.W >> 1) + (w >> 1);
        torgb_dot<C>(p.px + pidx * p.PCin, p.pw, p.PCin, ps);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float v = p.out_mul * (p.scale * s[c] + (p.bias ? p.bias[c] : 0.f));
        if (p.px) v = p.prev_mul * (p.pscale * ps[c] + (p.pbias ? p.pbias[c] : 0.f)) + v;
        p.img[(n * C + c) * hw + r] = v;
    }
}

inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline int lg2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline bool misaligned(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) != 0; }

// Tile geometry of 64 PF pixels: PF = 1 takes any map (8x8, or whole 4-wide maps of several images); the larger tiles whole maps of
// at least their size.  Returns false where the geometry does not fit the map.
bool tile_geometry(SmpConv& p, int PF)
{
    int TW, TH;
    if (PF == 1) { TW = p.W < 8 ? p.W : 8; TH = p.H < 8 ? p.H : 8; }
    else { TW = PF == 8 ? 32 : 16; TH = PF == 2 ? 8 : 16; if (p.W < TW || p.H < TH) return false; }
    p.lgTW = lg2(TW); p.lgTH = lg2(TH); p.TN = BPX * PF / (TW * TH);
    p.tilesW = p.W / TW; p.tilesH = p.H / TH;
    const long long ntiles = (long long)p.tilesW * p.tilesH * ((p.N + p.TN - 1) / p.TN);
    if (ntiles >= (1ll << 31)) return false;
    p.ntiles = (int)ntiles;
    return true;
}

template <int NT, int PF>
int launch_conv3(const SmpConv& p, hipStream_t s)
{
    const int ncob = (p.Cout + 16 * NT - 1) / (16 * NT);
    const int gx = p.Cin <= KC && p.ntiles > PERSIST_GRID ? PERSIST_GRID : p.ntiles;
    const int halo = p.TN * ((1 << p.lgTH) + 2) * ((1 << p.lgTW) + 2);
    const size_t lds = (size_t)(9 * 16 * NT + halo) * p.kcp * sizeof(uint16_t);
    if (lds > 64 * 1024) {                                   // above the default limit of a launch (wide layers: the call is small beside them)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(smp_conv3_kernel<NT, PF>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((smp_conv3_kernel<NT, PF>), dim3(gx, ncob), dim3(256), lds, s, p);
    return (int)hipGetLastError();
}

// The pixel tile: the largest that still leaves every CU two workgroups (weights and halo are re-read least, and a workgroup of a
// narrow layer has the most bytes in flight); NT * PF <= 16 accumulator fragments per wave.
template <int NT>
int dispatch_conv3(SmpConv& p, hipStream_t s)
{
    const int ncob = (p.Cout + 16 * NT - 1) / (16 * NT);
    constexpr int PFMAX = 16 / NT;
    if (PFMAX >= 8 && tile_geometry(p, 8) && (long long)p.ntiles * ncob >= MIN_WORKGROUPS) return launch_conv3<NT, (PFMAX >= 8 ? 8 : 1)>(p, s);
    if (PFMAX >= 4 && tile_geometry(p, 4) && (long long)p.ntiles * ncob >= MIN_WORKGROUPS) return launch_conv3<NT, (PFMAX >= 4 ? 4 : 1)>(p, s);
    if (PFMAX >= 2 && tile_geometry(p, 2) && (long long)p.ntiles * ncob >= MIN_WORKGROUPS) return launch_conv3<NT, (PFMAX >= 2 ? 2 : 1)>(p, s);
    if (!tile_geometry(p, 1)) return PG_E_UNSUP;
    return launch_conv3<NT, 1>(p, s);
}

}  // namespace

extern "C" int pg_smp_cast_bf16(const float* x, uint16_t* y, int64_t n, pg_stream_t stream)
{
    if (!x || !y || n <= 0) return PG_E_ARG;
    if (misaligned(x) || misaligned(y)) return PG_E_ALIGN;
    const int64_t blocks = ((n >> 2) + 255) / 256;
    const int grid = (int)(blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks);
    hipLaunchKernelGGL(smp_cast_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, y, n);
    return (int)hipGetLastError();
}

extern "C" int pg_smp_conv3_bf16(const uint16_t* x, const uint16_t* w, const float* bias, void* y, int N, int Hin, int Win, int Cin, int Cout,
                                 int flags, float scale, float slope, float eps, pg_stream_t stream)
{
    if (!x || !w || !y || N <= 0 || Hin <= 0 || Win <= 0 || Cin <= 0 || Cout <= 0) return PG_E_ARG;
    if (flags & ~(PG_SMP_UPSAMPLE | PG_SMP_PIXELNORM | PG_SMP_OUT_F32)) return PG_E_ARG;
    if ((Cin & 7) || (Cout & 7)) return PG_E_ALIGN;
    if (misaligned(x) || misaligned(w) || misaligned(y) || misaligned(bias)) return PG_E_ALIGN;
    SmpConv p;
    p.x = x; p.w = w; p.bias = bias; p.y = y;
    p.N = N; p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.Cout = Cout;
    p.ups = (flags & PG_SMP_UPSAMPLE) ? 1 : 0; p.pixelnorm = (flags & PG_SMP_PIXELNORM) ? 1 : 0; p.out_f32 = (flags & PG_SMP_OUT_F32) ? 1 : 0;
    p.scale = scale; p.slope = slope; p.eps = eps;
    if (Hin >= (1 << 20) || Win >= (1 << 20)) return PG_E_UNSUP;
    p.H = p.ups ? 2 * Hin : Hin; p.W = p.ups ? 2 * Win : Win;
    if (!pow2(p.H) || !pow2(p.W) || p.H < 4 || p.W < 4) return PG_E_UNSUP;
    if ((long long)N * Hin * Win * Cin >= (1ll << 31) || (long long)N * p.H * p.W * Cout >= (1ll << 31) ||
        (long long)9 * Cout * Cin >= (1ll << 31)) return PG_E_UNSUP;
    if (p.pixelnorm && Cout > PG_SMP_PIXELNORM_MAX_COUT) return PG_E_UNSUP;
    p.kcp = (Cin < KC ? Cin : KC) + 8;
    if (!tile_geometry(p, 1)) return PG_E_UNSUP;
    const long long ntiles = p.ntiles;
    hipStream_t s = (hipStream_t)stream;
    if (p.pixelnorm)                                      // every cout of a pixel in one wave
        return Cout <= 16 ? dispatch_conv3<1>(p, s) : Cout <= 32 ? dispatch_conv3<2>(p, s) : Cout <= 64 ? dispatch_conv3<4>(p, s) : dispatch_conv3<8>(p, s);
    // otherwise the widest cout tile (weights read least often) that still gives every CU a workgroup
    if (Cout > 32 && ntiles * ((Cout + 63) / 64) >= 256) return dispatch_conv3<4>(p, s);
    if (Cout > 16 && (Cout <= 32 || ntiles * ((Cout + 31) / 32) >= 256)) return dispatch_conv3<2>(p, s);
    return dispatch_conv3<1>(p, s);
}

extern "C" int pg_smp_pixelnorm_bf16(const float* x, uint16_t* y, int64_t P, int C, float eps, pg_stream_t stream)
{
    if (!x || !y || P <= 0 || C <= 0) return PG_E_ARG;
    if ((C & 3) || misaligned(x) || misaligned(y)) return PG_E_ALIGN;
    const int64_t blocks = (P + 3) / 4;
    if (blocks >= (1ll << 31)) return PG_E_UNSUP;
    hipLaunchKernelGGL(smp_pixelnorm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, y, P, C, eps);
    return (int)hipGetLastError();
}

extern "C" int pg_smp_torgb_bf16(const uint16_t* x, const float* w, const float* bias, float scale, float out_mul,
                                 const uint16_t* px, const float* pw, const float* pbias, float pscale, float prev_mul, int PCin,
                                 float* img, int N, int C, int H, int W, int Cin, pg_stream_t stream)
{
    if (!x || !w || !img || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Cin <= 0) return PG_E_ARG;
    if (px && (!pw || PCin <= 0 || ((H | W) & 1))) return PG_E_ARG;
    if (C > PG_SMP_TORGB_MAX_C) return PG_E_UNSUP;
    if ((Cin & 7) || (px && (PCin & 7))) return PG_E_ALIGN;
    if (misaligned(x) || misaligned(w) || misaligned(px) || misaligned(pw) || misaligned(img)) return PG_E_ALIGN;
    const long long npix = (long long)N * H * W;
    if (npix * Cin >= (1ll << 31) || npix * C >= (1ll << 31)) return PG_E_UNSUP;
    SmpRgb p;
    p.x = x; p.w = w; p.bias = bias; p.scale = scale; p.out_mul = out_mul;
    p.px = px; p.pw = pw; p.pbias = pbias; p.pscale = pscale; p.prev_mul = prev_mul; p.PCin = PCin;
    p.img = img; p.N = N; p.H = H; p.W = W; p.Cin = Cin;
    const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
    case 1: hipLaunchKernelGGL(smp_torgb_kernel<1>, grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL(smp_torgb_kernel<2>, grid, block, 0, s, p); break;
    case 3: hipLaunchKernelGGL(smp_torgb_kernel<3>, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(smp_torgb_kernel<4>, grid, block, 0, s, p); break;
    }
    return (int)hipGetLastError();
}
