// Block-MFMA forward kernel of the 8/16-cout 3x3 layers of the equalized-lr convolution (gfx950 / CDNA4).
//
// Owns: conv_thin_kernel with launch_thin, and pgk::dispatch_thin, which hands strip-sized maps to the row-streaming kernels of
// conv_strip.hip first.  Which requests come here: thin_shape / conv2d_impl and pg_conv2d_unpooled_nhwc (conv_api.hip).
#include "convp.h"

namespace {

using namespace pgk;

// 3x3 layers with 8 or 16 output channels and <= 32 input channels (the 512^2 / 1024^2 stages and their
// backward-data convs).  A 16x16x4 tile wastes half of its rows on 8 couts and, more importantly, these layers have
// no K loop to pipeline; v_mfma_f32_4x4x1_16B_f32 with block = (cout quad, pixel quad) covers COUT couts x
// 64*4/COUT consecutive pixels of a row per instruction for one (tap, cin), every lane useful.
// Workgroup: TH rows x 32 pixels of one image, whole-K halo tile in LDS (row stride CIN+4 floats: conflict-free
// b128), one barrier, wave w owns TH/4 rows; weights are re-read from LDS per (tap, cin quad) as one b128.
// Optional fused 2x2 average pool of the activated output (see pg_conv2d_pool_nhwc).
template <int COUT, int CIN, int TH>
__global__ __launch_bounds__(256) void conv_thin_kernel(ConvP p)
{
    constexpr int S = CIN + 4, WT = 34, HT = TH + 2, C4 = CIN / 4;
    constexpr int QO = COUT / 4, QP = 16 / QO, PXG = 4 * QP;            // pixels per MFMA group: 32 (8 couts) / 16
    constexpr int GPR = 32 / PXG, G = (TH / 4) * GPR;                   // groups per row, groups per wave
    extern __shared__ __align__(16) float lds[];
    float* xt = lds;                             // [HT][WT][S]
    float* wl = lds + HT * WT * S;               // [9][COUT][CIN]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = lane >> 2, j = lane & 3, qo = blk % QO, qp = blk / QO;
    int b = (int)pg_xcd_remap(blockIdx.x, gridDim.x);         // contiguous tile ranges per XCD: halos come from its L2
    const int tw_i = b % (p.Wout >> 5); b /= (p.Wout >> 5);
    const int th_i = b % (p.Hout / TH); const int n = b / (p.Hout / TH);
    const int oh0 = th_i * TH, ow0 = tw_i << 5;
    const int xH = p.ups ? (p.Hin >> 1) : p.Hin, xW = p.ups ? (p.Win >> 1) : p.Win;

    // one image through a raw buffer (bufload.h): out-of-image halo pixels are zero-filled by the hardware, no branch per load
    const __amdgpu_buffer_rsrc_t rx = pg_make_rsrc(p.x + (size_t)n * xH * xW * CIN, (unsigned)((size_t)xH * xW * CIN * 4));
    constexpr int NLD = (HT * WT * C4 + 255) / 256;
    const unsigned char* gbase = p.gbytes ? p.gbytes + (size_t)n * p.Hin * p.Win * C4 : nullptr;     // this image's sign bytes
    float4 xv[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + 256 * i;
        const int c4 = e % C4; const int q = e / C4;
        const int tw = q % WT, th = q / WT;
        int ih = oh0 + th - 1, iw = ow0 + tw - 1;
        const bool ok = e < HT * WT * C4 && (unsigned)ih < (unsigned)p.Hin && (unsigned)iw < (unsigned)p.Win;
        unsigned char gb = 0;
        if (p.gbytes && ok) gb = gbase[(ih * p.Win + iw) * C4 + c4];
        if (p.ups) { ih >>= 1; iw >>= 1; }
        xv[i] = pg_buf_load4(rx, ok ? 4u * (unsigned)((ih * xW + iw) * CIN + 4 * c4) : PG_OOB, 0);
        if (p.gbytes) {                              // pool adjoint in the gather: x 1/4 (x mul) x LeakyReLU' of the finer activation
            const float4 f = pg_sign_factors(gb, p.gslope);
            xv[i].x *= f.x * p.gmul; xv[i].y *= f.y * p.gmul; xv[i].z *= f.z * p.gmul; xv[i].w *= f.w * p.gmul;
        }
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int e = tid + 256 * i;
        if (e < HT * WT * C4) *reinterpret_cast<float4*>(xt + (e / C4) * S + 4 * (e % C4)) = xv[i];
    }
    for (int e = tid; e < 9 * COUT * C4; e += 256)
        *reinterpret_cast<float4*>(wl + 4 * e) = *reinterpret_cast<const float4*>(p.w + 4 * e);
    __syncthreads();

    f32x4 acc[G], acc2[G];
    int xoff[G];                                 // LDS offset of this lane's pixel in group g (tap 0,0)
#pragma unroll
    for (int g = 0; g < G; ++g) {
        acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc2[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int gg = wave * G + g;
        xoff[g] = ((gg / GPR) * WT + (gg % GPR) * PXG + 4 * qp + j) * S;
    }
    const float* wrow = wl + (4 * qo + j) * CIN; // A operand: couts 4*qo + (lane&3)
#pragma unroll
    for (int tp = 0; tp < 9; ++tp) {
        const int toff = ((tp / 3) * WT + (tp % 3)) * S;
#pragma unroll
        for (int c4 = 0; c4 < C4; ++c4) {
            const float4 a = *reinterpret_cast<const float4*>(wrow + tp * COUT * CIN + 4 * c4);
            float4 bq[G];
#pragma unroll
            for (int g = 0; g < G; ++g) bq[g] = *reinterpret_cast<const float4*>(xt + xoff[g] + toff + 4 * c4);
            // two accumulation chains per group (even / odd channel of the quad) and the groups interleaved: consecutive MFMAs
            // never share an accumulator (a dependent v_mfma_f32_4x4x1 cannot issue back to back)
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(a.x, bq[g].x, acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < G; ++g) acc2[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(a.y, bq[g].y, acc2[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < G; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(a.z, bq[g].z, acc[g], 0, 0, 0);
#pragma unroll
            for (int g = 0; g < G; ++g) acc2[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(a.w, bq[g].w, acc2[g], 0, 0, 0);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] += acc2[g];
    // D register r of this lane = out[pixel][cout 4*qo + r]
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) bv = *reinterpret_cast<const float4*>(p.bias + 4 * qo);
    float4 ov[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int gg = wave * G + g;
        const int oy = oh0 + gg / GPR, ox = ow0 + (gg % GPR) * PXG + 4 * qp + j;
        const size_t off = (((size_t)n * p.Hout + oy) * p.Wout + ox) * COUT + 4 * qo;
        float4 o = make_float4(acc[g][0] * p.scale, acc[g][1] * p.scale, acc[g][2] * p.scale, acc[g][3] * p.scale);
        if (p.mask) {
            float4 f;
            if (p.mask_bytes) f = pg_sign_factors(reinterpret_cast<const unsigned char*>(p.mask)[off >> 2], p.mask_slope);
            else {
                const float4 mk = *reinterpret_cast<const float4*>(p.mask + off);
                f = make_float4(mk.x > 0.f ? 1.f : p.mask_slope, mk.y > 0.f ? 1.f : p.mask_slope,
                                mk.z > 0.f ? 1.f : p.mask_slope, mk.w > 0.f ? 1.f : p.mask_slope);
            }
            o.x *= f.x; o.y *= f.y; o.z *= f.z; o.w *= f.w;
        } else {
            o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
            o.x = o.x > 0.f ? o.x : o.x * p.slope; o.y = o.y > 0.f ? o.y : o.y * p.slope;
            o.z = o.z > 0.f ? o.z : o.z * p.slope; o.w = o.w > 0.f ? o.w : o.w * p.slope;
            if (p.ysigns) p.ysigns[off >> 2] = pg_sign_byte(o);
        }
        if (p.pnb_y) {                               // adjoint of the previous layer's (LeakyReLU -> PixelNorm), see ConvP
            const float4 yv = *reinterpret_cast<const float4*>(p.pnb_y + off);
            const float4 gv = make_float4(acc[g][0] * p.scale, acc[g][1] * p.scale, acc[g][2] * p.scale, acc[g][3] * p.scale);
            float dt = (gv.x * yv.x + gv.y * yv.y) + (gv.z * yv.z + gv.w * yv.w);
            dt += __shfl_xor(dt, 4, 64);
            if (QO >= 4) dt += __shfl_xor(dt, 8, 64);
            const float rr = p.pnb_r[((size_t)n * p.Hout + oy) * p.Wout + ox], mean = dt / (float)COUT;
            o.x = rr * (gv.x - yv.x * mean) * (yv.x > 0.f ? 1.f : p.mask_slope);
            o.y = rr * (gv.y - yv.y * mean) * (yv.y > 0.f ? 1.f : p.mask_slope);
            o.z = rr * (gv.z - yv.z * mean) * (yv.z > 0.f ? 1.f : p.mask_slope);
            o.w = rr * (gv.w - yv.w * mean) * (yv.w > 0.f ? 1.f : p.mask_slope);
        }
        if (p.pn_r) {                                // PixelNorm over the COUT channels of the pixel: QO lanes (4 apart) share it
            float ssq = (o.x * o.x + o.y * o.y) + (o.z * o.z + o.w * o.w);
            ssq += __shfl_xor(ssq, 4, 64);
            if (QO >= 4) ssq += __shfl_xor(ssq, 8, 64);
            const float rr = rsqrtf(ssq / (float)COUT + p.pn_eps);
            o.x *= rr; o.y *= rr; o.z *= rr; o.w *= rr;
            if (qo == 0) p.pn_r[((size_t)n * p.Hout + oy) * p.Wout + ox] = rr;
        }
        if (p.y_bytes) reinterpret_cast<unsigned char*>(p.y)[off >> 2] = pg_sign_byte(o);
        else if (!(p.ypool && p.pool_only)) *reinterpret_cast<float4*>(p.y + off) = o;
        ov[g] = o;
    }
    if (p.ypool) {                               // 2x2 mean: column partner = lane^1, row partner = group g + GPR (same wave)
        static_assert(TH % 8 == 0, "a wave must own complete row pairs");
#pragma unroll
        for (int g = 0; g < G; ++g) {
            ov[g].x += __shfl_xor(ov[g].x, 1, 64); ov[g].y += __shfl_xor(ov[g].y, 1, 64);
            ov[g].z += __shfl_xor(ov[g].z, 1, 64); ov[g].w += __shfl_xor(ov[g].w, 1, 64);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (((g / GPR) & 1) != 0) continue;                  // compile-time: even rows lead
            const int gg = wave * G + g;
            const int oy = oh0 + gg / GPR, ox = ow0 + (gg % GPR) * PXG + 4 * qp + j;
            float4 v = make_float4(((ov[g].x + ov[g + GPR].x)) * 0.25f, ((ov[g].y + ov[g + GPR].y)) * 0.25f,
                                   ((ov[g].z + ov[g + GPR].z)) * 0.25f, ((ov[g].w + ov[g + GPR].w)) * 0.25f);
            if (j & 1) continue;
            const size_t poff = (((size_t)n * (p.Hout >> 1) + (oy >> 1)) * (p.Wout >> 1) + (ox >> 1)) * COUT + 4 * qo;
            if (p.pool_other) {
                const float4 q = *reinterpret_cast<const float4*>(p.pool_other + poff);
                v.x = fmaf(v.x, p.pool_a, p.pool_b * q.x); v.y = fmaf(v.y, p.pool_a, p.pool_b * q.y);
                v.z = fmaf(v.z, p.pool_a, p.pool_b * q.z); v.w = fmaf(v.w, p.pool_a, p.pool_b * q.w);
            } else if (p.pool_a != 1.f) { v.x *= p.pool_a; v.y *= p.pool_a; v.z *= p.pool_a; v.w *= p.pool_a; }
            *reinterpret_cast<float4*>(p.ypool + poff) = v;
        }
    }
}

template <int COUT, int CIN, int TH>
int launch_thin(ConvP& p, hipStream_t s)
{
    const size_t smem = ((size_t)(TH + 2) * 34 * (CIN + 4) + 9 * COUT * CIN) * sizeof(float);
    if ((long long)p.Hin * p.Win * CIN * 4 >= (1ll << 31)) return PG_E_UNSUP;                  // 32-bit buffer offsets per image
    auto kern = conv_thin_kernel<COUT, CIN, TH>;
    if (int rc = set_smem(kern, smem)) return rc;
    dim3 grid((unsigned)(p.N * (p.Hout / TH) * (p.Wout >> 5)));
    snprintf(g_last_kernel, sizeof(g_last_kernel), "conv_thin_kernel<%d, %d, %d>", COUT, CIN, TH);
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, p);
    return (int)hipGetLastError();
}

}  // namespace

int pgk::dispatch_thin(ConvP& p, hipStream_t s)
{
    if (g_tune[PG_TUNE_PATH] != PG_PATH_TILE_NOT_STRIP) {        // row-streaming kernel (conv_strip.hip) where the shape allows
        const int rc = launch_conv_strip(p, s);
        if (rc != PG_E_UNSUP) return rc;
    }
#define THIN(CO_, CI_) if (p.Cout == CO_ && p.Cin == CI_) return launch_thin<CO_, CI_, 8>(p, s);
    THIN(8, 8) THIN(8, 16) THIN(16, 8)
#undef THIN
    return PG_E_UNSUP;
}
