// Equalized-lr convolution as an implicit GEMM on v_mfma_f32_16x16x4_f32 (gfx950 / CDNA4): the tile forward kernels.
//
// Owns: conv_igemm_kernel (generic tile kernel: forward / backward-data / GP-tangent, every fused epilogue) with
// conv_epilogue_kernel (deferred epilogue of its split-K launches) and launch_conv; conv_ksplit_kernel (four-wave K-split for
// small maps) with launch_ksplit; the tile-shape cost model and dispatch_conv behind pgk::dispatch_conv_tile.  (The other
// units of the direct conv: see convp.h.)
//
// Layout: activations NHWC, weights [KH][KW][Cout][Cin] => both MFMA operands are K-contiguous,
// so one ds_read_b128 per lane feeds four 16x16x4 k-steps (lane (i = l&15, kk = l>>4) owns
// channels 4kk..4kk+3 of a 16-channel chunk; k-step s contracts channels {s, 4+s, 8+s, 12+s}).
// MFMA roles: A = weights (row i = cout), B = activations (col j = pixel); the C/D fragment then
// holds 4 consecutive couts of one pixel per lane -> 16-byte NHWC stores.
// Exact fp32 FMA chain (no reduced-precision path): parity with the fp32 CPU oracle to ~1e-6.
//
// Pipeline: per-thread load descriptors are computed once; the NEXT K-chunk is fetched global->VGPR while the MFMAs of the
// current one run out of LDS (one LDS buffer, two workgroups per CU), and inside a chunk the fragments of the next tap / k-step
// are read from LDS while the current MFMAs issue.  LDS row strides are chosen conflict-free for the
// lane groups of ds_read_b128 / ds_read_b32 on gfx950 (24 floats for 16-channel rows).
#include "convp.h"

namespace {

using namespace pgk;

// One workgroup (4 waves) computes BCO couts x BPX output pixels; the pixel tile is
// TN images x TH x TW (powers of two) so that the (KS-1)-halo of the input is staged once in LDS
// and every tap is a shifted read of the same tile.
template <int KS, int VEC, int WAVES_CO, int WM, int WN>
__global__ __launch_bounds__(256) void conv_igemm_kernel(ConvP p)
{
    constexpr int WAVES_PX = 4 / WAVES_CO;
    constexpr int BCO = 16 * WM * WAVES_CO, BPX = 16 * WN * WAVES_PX;
    constexpr int KC = 4 * VEC, KCP = RowStride<VEC>::value;
    constexpr int TAPS = KS * KS;
    constexpr int WEL = TAPS * BCO * VEC;                       // float4 elements of one weight chunk
    constexpr int WPT = (WEL + 255) / 256;
    constexpr int XMAX = halo_max(KS, BPX);
    constexpr int XPT = (XMAX * VEC + 255) / 256;
    extern __shared__ __align__(16) float lds[];

    const int TW = 1 << p.lgTW, TH = 1 << p.lgTH;
    const int HT = TH + KS - 1, WT = TW + KS - 1;
    float* wt = lds;                          // [TAPS][BCO][KCP]
    float* xt = lds + TAPS * BCO * KCP;       // [TN][HT][WT][KCP]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_co = wave % WAVES_CO, wave_px = wave / WAVES_CO;
    const int li = lane & 15, kk = lane >> 4;

    int t = (int)pg_xcd_remap(blockIdx.x, gridDim.x);       // contiguous tile ranges per XCD (bufload.h)
    const int tw_i = t % p.tilesW; t /= p.tilesW;
    const int th_i = t % p.tilesH; t /= p.tilesH;
    const int n0 = t * p.TN;
    const int oh0 = th_i << p.lgTH, ow0 = tw_i << p.lgTW;
    const int co0 = blockIdx.y * BCO;

    int pixbase[WN], wbase[WM];
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int j = (wave_px * WN + n) * 16 + li;
        const int tw = j & (TW - 1), th = (j >> p.lgTW) & (TH - 1), tn = j >> (p.lgTW + p.lgTH);
        pixbase[n] = ((tn * HT + th) * WT + tw) * KCP + VEC * kk;
    }
#pragma unroll
    for (int m = 0; m < WM; ++m) wbase[m] = ((wave_co * WM + m) * 16 + li) * KCP + VEC * kk;

    // ---- per-thread load descriptors (element offsets without the channel-chunk offset; -1 = zero fill)
    const int xH = p.ups ? (p.Hin >> 1) : p.Hin, xW = p.ups ? (p.Win >> 1) : p.Win;
    const int npix = p.TN * HT * WT;
    // global loads go through raw buffers (bufload.h): byte offsets, PG_OOB = zero fill, x relative to image n0
    const size_t img = (size_t)xH * xW * p.Cin;
    const __amdgpu_buffer_rsrc_t rx = pg_make_rsrc(p.x + (size_t)n0 * img, (unsigned)(min(p.TN, p.N - n0) * img * 4));
    const __amdgpu_buffer_rsrc_t rw = pg_make_rsrc(p.w, (unsigned)((size_t)TAPS * p.Cout * p.Cin * 4));
    unsigned wsrc[WPT], xsrc[XPT];
    int wdst[WPT], xdst[XPT];
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
        const int idx = tid + 256 * i;
        const int r = idx / VEC, v = idx - r * VEC;
        const int tap = r / BCO, col = r - tap * BCO, co = co0 + col;
        wdst[i] = idx < WEL ? r * KCP + 4 * v : -1;
        wsrc[i] = (idx < WEL && co < p.Cout) ? 4u * (unsigned)((tap * p.Cout + co) * p.Cin + 4 * v) : PG_OOB;
    }
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
        const int idx = tid + 256 * i;
        const int q = idx / VEC, v = idx - q * VEC;
        const int r2 = (int)__umulhi((unsigned)q, p.mWT), tw = q - r2 * WT;       // q / WT, q % WT (q < 2^16)
        const int tn = (int)__umulhi((unsigned)r2, p.mHT), th = r2 - tn * HT;
        const int n = n0 + tn;
        int ih = oh0 + th - p.pad, iw = ow0 + tw - p.pad;
        const bool in_tile = q < npix;
        const bool ok = in_tile && n < p.N && (unsigned)ih < (unsigned)p.Hin && (unsigned)iw < (unsigned)p.Win;
        if (p.ups) { ih >>= 1; iw >>= 1; }
        xdst[i] = in_tile ? q * KCP + 4 * v : -1;
        xsrc[i] = ok ? 4u * (unsigned)(((tn * xH + ih) * xW + iw) * p.Cin + 4 * v) : PG_OOB;
    }
    int tapoff[TAPS];
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp) tapoff[tp] = ((tp / KS) * WT + (tp % KS)) * KCP;

    f32x4 acc[WM][WN];
#pragma unroll
    for (int m = 0; m < WM; ++m)
#pragma unroll
        for (int n = 0; n < WN; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc_odd = f32x4{0.f, 0.f, 0.f, 0.f};                  // second accumulation chain of the single-tile variants

    const int nchunks = p.Cin / KC;
    const int cper = (nchunks + p.ksplit - 1) / p.ksplit;
    const int kc_begin = blockIdx.z * cper;
    const int kc_end = min(nchunks, kc_begin + cper);

    float4 wreg[WPT], xreg[XPT];
    auto fetch = [&](int kc) {
        const int k0 = kc * KC;
#pragma unroll
        for (int i = 0; i < WPT; ++i) wreg[i] = pg_buf_load4(rw, wsrc[i], 4u * (unsigned)k0);
#pragma unroll
        for (int i = 0; i < XPT; ++i) xreg[i] = pg_buf_load4(rx, xsrc[i], 4u * (unsigned)k0);
    };

    if (kc_begin < kc_end) fetch(kc_begin);
    for (int kc = kc_begin; kc < kc_end; ++kc) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) if (wdst[i] >= 0) *reinterpret_cast<float4*>(wt + wdst[i]) = wreg[i];
#pragma unroll
        for (int i = 0; i < XPT; ++i) if (xdst[i] >= 0) *reinterpret_cast<float4*>(xt + xdst[i]) = xreg[i];
        __syncthreads();
        if (kc + 1 < kc_end) fetch(kc + 1);              // in flight while the MFMAs below run

        float a[2][WM][VEC], b[2][WN][VEC];
#pragma unroll
        for (int m = 0; m < WM; ++m) lds_load<VEC>(wt + wbase[m], a[0][m]);
#pragma unroll
        for (int n = 0; n < WN; ++n) lds_load<VEC>(xt + pixbase[n] + tapoff[0], b[0][n]);
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) {
            const int cur = tp & 1, nxt = cur ^ 1;
            if (tp + 1 < TAPS) {
#pragma unroll
                for (int m = 0; m < WM; ++m) lds_load<VEC>(wt + (tp + 1) * BCO * KCP + wbase[m], a[nxt][m]);
#pragma unroll
                for (int n = 0; n < WN; ++n) lds_load<VEC>(xt + pixbase[n] + tapoff[tp + 1], b[nxt][n]);
            }
            // pin the order "issue next tap's LDS reads, THEN this tap's MFMAs": hipcc otherwise sinks the reads
            // next to their first use and every tap starts with an exposed LDS round trip
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < VEC; ++s) {
                if constexpr (WM * WN == 1) {
                    // one output tile per wave: alternate two accumulators so that two MFMAs on the same accumulator are
                    // never adjacent (32-cycle issue, 40-cycle dependent latency, ~43 extra with anything in between)
                    if (s & 1) acc_odd = MFMA16(a[cur][0][s], b[cur][0][s], acc_odd);
                    else acc[0][0] = MFMA16(a[cur][0][s], b[cur][0][s], acc[0][0]);
                } else {
#pragma unroll
                    for (int m = 0; m < WM; ++m)
#pragma unroll
                        for (int n = 0; n < WN; ++n) acc[m][n] = MFMA16(a[cur][m][s], b[cur][n][s], acc[m][n]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }
    if constexpr (WM * WN == 1 && VEC > 1) acc[0][0] += acc_odd;

    // epilogue: lane holds couts cb..cb+3 of pixel j
    if (p.pn_r != nullptr) {                     // conv -> bias -> LeakyReLU -> PixelNorm; the workgroup holds every cout of its pixels
        float4 o[WM][WN];
        float ss[WN];
#pragma unroll
        for (int n = 0; n < WN; ++n) ss[n] = 0.f;
#pragma unroll
        for (int m = 0; m < WM; ++m) {
            const int cb = co0 + (wave_co * WM + m) * 16 + 4 * kk;
            float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (p.bias && cb < p.Cout) bv = *reinterpret_cast<const float4*>(p.bias + cb);
#pragma unroll
            for (int n = 0; n < WN; ++n) {
                float4 v = make_float4(acc[m][n][0] * p.scale + bv.x, acc[m][n][1] * p.scale + bv.y,
                                       acc[m][n][2] * p.scale + bv.z, acc[m][n][3] * p.scale + bv.w);
                v.x = v.x > 0.f ? v.x : v.x * p.slope; v.y = v.y > 0.f ? v.y : v.y * p.slope;
                v.z = v.z > 0.f ? v.z : v.z * p.slope; v.w = v.w > 0.f ? v.w : v.w * p.slope;
                if (cb >= p.Cout) v = make_float4(0.f, 0.f, 0.f, 0.f);
                o[m][n] = v;
                ss[n] += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
            }
        }
#pragma unroll
        for (int n = 0; n < WN; ++n) {
            ss[n] += __shfl_xor(ss[n], 16, 64);
            ss[n] += __shfl_xor(ss[n], 32, 64);
            const float rr = rsqrtf(ss[n] / (float)p.Cout + p.pn_eps);
            const int j = (wave_px * WN + n) * 16 + li;
            const int tw = j & (TW - 1), th = (j >> p.lgTW) & (TH - 1), tn = j >> (p.lgTW + p.lgTH);
            const int ni = n0 + tn;
            if (ni >= p.N) continue;
            const size_t pix = ((size_t)ni * p.Hout + oh0 + th) * p.Wout + ow0 + tw;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                const int cb = co0 + (wave_co * WM + m) * 16 + 4 * kk;
                if (cb >= p.Cout) continue;
                *reinterpret_cast<float4*>(p.y + pix * p.Cout + cb) =
                    make_float4(o[m][n].x * rr, o[m][n].y * rr, o[m][n].z * rr, o[m][n].w * rr);
            }
            if (kk == 0) p.pn_r[pix] = rr;
        }
        return;
    }
    if (p.pnb_y != nullptr) {                    // backward-data conv + adjoint of the previous layer's LeakyReLU -> PixelNorm
        float4 gq[WM][WN], yq[WM][WN];
        float dot[WN];
#pragma unroll
        for (int n = 0; n < WN; ++n) dot[n] = 0.f;
#pragma unroll
        for (int n = 0; n < WN; ++n) {
            const int j = (wave_px * WN + n) * 16 + li;
            const int tw = j & (TW - 1), th = (j >> p.lgTW) & (TH - 1), tn = j >> (p.lgTW + p.lgTH);
            const int ni = n0 + tn;
            const size_t pix = ((size_t)(ni < p.N ? ni : 0) * p.Hout + oh0 + th) * p.Wout + ow0 + tw;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                const int cb = co0 + (wave_co * WM + m) * 16 + 4 * kk;
                float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), yv = gv;
                if (cb < p.Cout && ni < p.N) {
                    gv = make_float4(acc[m][n][0] * p.scale, acc[m][n][1] * p.scale, acc[m][n][2] * p.scale, acc[m][n][3] * p.scale);
                    yv = *reinterpret_cast<const float4*>(p.pnb_y + pix * p.Cout + cb);
                }
                gq[m][n] = gv; yq[m][n] = yv;
                dot[n] += (gv.x * yv.x + gv.y * yv.y) + (gv.z * yv.z + gv.w * yv.w);
            }
        }
#pragma unroll
        for (int n = 0; n < WN; ++n) {
            dot[n] += __shfl_xor(dot[n], 16, 64);
            dot[n] += __shfl_xor(dot[n], 32, 64);
            const int j = (wave_px * WN + n) * 16 + li;
            const int tw = j & (TW - 1), th = (j >> p.lgTW) & (TH - 1), tn = j >> (p.lgTW + p.lgTH);
            const int ni = n0 + tn;
            if (ni >= p.N) continue;
            const size_t pix = ((size_t)ni * p.Hout + oh0 + th) * p.Wout + ow0 + tw;
            const float rr = p.pnb_r[pix], mean = dot[n] / (float)p.Cout;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                const int cb = co0 + (wave_co * WM + m) * 16 + 4 * kk;
                if (cb >= p.Cout) continue;
                const float4 gv = gq[m][n], yv = yq[m][n];
                float4 o;
                o.x = rr * (gv.x - yv.x * mean) * (yv.x > 0.f ? 1.f : p.mask_slope);
                o.y = rr * (gv.y - yv.y * mean) * (yv.y > 0.f ? 1.f : p.mask_slope);
                o.z = rr * (gv.z - yv.z * mean) * (yv.z > 0.f ? 1.f : p.mask_slope);
                o.w = rr * (gv.w - yv.w * mean) * (yv.w > 0.f ? 1.f : p.mask_slope);
                *reinterpret_cast<float4*>(p.y + pix * p.Cout + cb) = o;
            }
        }
        return;
    }
    const bool pooling = p.ypool != nullptr && p.ksplit == 1;
#pragma unroll
    for (int m = 0; m < WM; ++m) {
        const int cb = co0 + (wave_co * WM + m) * 16 + 4 * kk;
        const bool cvalid = cb < p.Cout;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p.bias && cvalid) bv = *reinterpret_cast<const float4*>(p.bias + cb);
        float4 ov[WN];
#pragma unroll
        for (int n = 0; n < WN; ++n) {
            ov[n] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int j = (wave_px * WN + n) * 16 + li;
            const int tw = j & (TW - 1), th = (j >> p.lgTW) & (TH - 1), tn = j >> (p.lgTW + p.lgTH);
            const int ni = n0 + tn;
            if (!cvalid || ni >= p.N) continue;
            const size_t off = (((size_t)ni * p.Hout + oh0 + th) * p.Wout + ow0 + tw) * p.Cout + cb;
            float4 o;
            o.x = acc[m][n][0] * p.scale; o.y = acc[m][n][1] * p.scale;
            o.z = acc[m][n][2] * p.scale; o.w = acc[m][n][3] * p.scale;
            if (p.ksplit > 1) {
                atomicAdd(p.y + off + 0, o.x); atomicAdd(p.y + off + 1, o.y);
                atomicAdd(p.y + off + 2, o.z); atomicAdd(p.y + off + 3, o.w);
                continue;
            }
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
            }
            if (p.yup) {                                         // unpool: four masked copies, y itself is not needed
                const float k = p.up_mul * 0.25f;
                const size_t W2 = (size_t)2 * p.Wout;
                const size_t ubase = (((size_t)ni * 2 * p.Hout + 2 * (oh0 + th)) * W2 + 2 * (ow0 + tw)) * p.Cout + cb;
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const size_t uo = ubase + ((size_t)(d >> 1) * W2 + (d & 1)) * p.Cout;
                    float4 v = make_float4(o.x * k, o.y * k, o.z * k, o.w * k);
                    if (p.upmask) {
                        float4 f;
                        if (p.mask_bytes) f = pg_sign_factors(reinterpret_cast<const unsigned char*>(p.upmask)[uo >> 2], p.mask_slope);
                        else {
                            const float4 mk = *reinterpret_cast<const float4*>(p.upmask + uo);
                            f = make_float4(mk.x > 0.f ? 1.f : p.mask_slope, mk.y > 0.f ? 1.f : p.mask_slope,
                                            mk.z > 0.f ? 1.f : p.mask_slope, mk.w > 0.f ? 1.f : p.mask_slope);
                        }
                        v.x *= f.x; v.y *= f.y; v.z *= f.z; v.w *= f.w;
                    }
                    *reinterpret_cast<float4*>(p.yup + uo) = v;
                }
                continue;
            }
            if (p.y_bytes) reinterpret_cast<unsigned char*>(p.y)[off >> 2] = pg_sign_byte(o);     // only the sign is kept (pooled output below)
            else if (!(pooling && p.pool_only)) *reinterpret_cast<float4*>(p.y + off) = o;
            if (p.ysigns) p.ysigns[off >> 2] = pg_sign_byte(o);
            ov[n] = o;
        }
        if (pooling) {
            // 2x2 mean inside the wave: the horizontal neighbour is lane^1; the vertical neighbour is lane^TW for
            // tiles <= 8 wide, the next 16-pixel group (TW 16) or the one after (TW 32) otherwise -- launch_conv
            // restricts TW so that this group belongs to the same wave.  Same summation order as pg_avgpool2_fwd.
#pragma unroll
            for (int n = 0; n < WN; ++n) {
                ov[n].x += __shfl_xor(ov[n].x, 1, 64); ov[n].y += __shfl_xor(ov[n].y, 1, 64);
                ov[n].z += __shfl_xor(ov[n].z, 1, 64); ov[n].w += __shfl_xor(ov[n].w, 1, 64);
            }
            bool rowlead[WN];
            if (p.lgTW <= 3) {
#pragma unroll
                for (int n = 0; n < WN; ++n) {
                    ov[n].x += __shfl_xor(ov[n].x, TW, 64); ov[n].y += __shfl_xor(ov[n].y, TW, 64);
                    ov[n].z += __shfl_xor(ov[n].z, TW, 64); ov[n].w += __shfl_xor(ov[n].w, TW, 64);
                    rowlead[n] = (li & TW) == 0;
                }
            } else if (p.lgTW == 4) {
#pragma unroll
                for (int n = 0; n < WN; ++n) rowlead[n] = (n & 1) == 0;
                if constexpr (WN >= 2) {
#pragma unroll
                    for (int n = 0; n < WN; n += 2) {
                        ov[n].x += ov[n + 1].x; ov[n].y += ov[n + 1].y; ov[n].z += ov[n + 1].z; ov[n].w += ov[n + 1].w;
                    }
                }
            } else {
#pragma unroll
                for (int n = 0; n < WN; ++n) rowlead[n] = (n & 2) == 0;
                if constexpr (WN >= 4) {
#pragma unroll
                    for (int n = 0; n < WN; n += 4) {
                        ov[n].x += ov[n + 2].x; ov[n].y += ov[n + 2].y; ov[n].z += ov[n + 2].z; ov[n].w += ov[n + 2].w;
                        ov[n + 1].x += ov[n + 3].x; ov[n + 1].y += ov[n + 3].y; ov[n + 1].z += ov[n + 3].z; ov[n + 1].w += ov[n + 3].w;
                    }
                }
            }
#pragma unroll
            for (int n = 0; n < WN; ++n) {
                const int j = (wave_px * WN + n) * 16 + li;
                const int tw = j & (TW - 1), th = (j >> p.lgTW) & (TH - 1), tn = j >> (p.lgTW + p.lgTH);
                const int ni = n0 + tn;
                if (!cvalid || ni >= p.N || !rowlead[n] || (li & 1)) continue;
                const size_t poff = (((size_t)ni * (p.Hout >> 1) + ((oh0 + th) >> 1)) * (p.Wout >> 1) + ((ow0 + tw) >> 1)) * p.Cout + cb;
                float4 v = make_float4(ov[n].x * 0.25f, ov[n].y * 0.25f, ov[n].z * 0.25f, ov[n].w * 0.25f);
                if (p.pool_other) {
                    const float4 q = *reinterpret_cast<const float4*>(p.pool_other + poff);
                    v.x = fmaf(v.x, p.pool_a, p.pool_b * q.x); v.y = fmaf(v.y, p.pool_a, p.pool_b * q.y);   // same form as
                    v.z = fmaf(v.z, p.pool_a, p.pool_b * q.z); v.w = fmaf(v.w, p.pool_a, p.pool_b * q.w);   // avgpool2_fwd_kernel
                } else if (p.pool_a != 1.f) { v.x *= p.pool_a; v.y *= p.pool_a; v.z *= p.pool_a; v.w *= p.pool_a; }
                *reinterpret_cast<float4*>(p.ypool + poff) = v;
            }
        }
    }
}

// Deferred epilogue of a split-K launch: y = mask ? y*lrelu'(mask) : lrelu(y + bias)   (in place)
__global__ __launch_bounds__(256) void conv_epilogue_kernel(float* __restrict__ y, const float* __restrict__ bias,
                                                            const float* __restrict__ mask, size_t npix, int Cout,
                                                            float slope, float mask_slope)
{
    const int c4n = Cout >> 2;
    const size_t total = npix * c4n;
    float4* y4 = reinterpret_cast<float4*>(y);
    const float4* m4 = reinterpret_cast<const float4*>(mask);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        float4 o = y4[i];
        if (mask) {
            const float4 mk = m4[i];
            o.x *= mk.x > 0.f ? 1.f : mask_slope; o.y *= mk.y > 0.f ? 1.f : mask_slope;
            o.z *= mk.z > 0.f ? 1.f : mask_slope; o.w *= mk.w > 0.f ? 1.f : mask_slope;
        } else {
            if (bias) {
                const float4 bv = *reinterpret_cast<const float4*>(bias + 4 * (i % c4n));
                o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
            }
            o.x = o.x > 0.f ? o.x : o.x * slope; o.y = o.y > 0.f ? o.y : o.y * slope;
            o.z = o.z > 0.f ? o.z : o.z * slope; o.w = o.w > 0.f ? o.w : o.w * slope;
        }
        y4[i] = o;
    }
}

template <int KS, int VEC, int WAVES_CO, int WM, int WN>
int launch_conv(ConvP& p, hipStream_t s)
{
    constexpr int WAVES_PX = 4 / WAVES_CO;
    constexpr int BCO = 16 * WM * WAVES_CO, BPX = 16 * WN * WAVES_PX, KCP = RowStride<VEC>::value;
    // fused pooling needs the vertical 2x2 partner inside the wave: <= 8-wide tiles always work (lane ^ TW),
    // 16-wide ones need two, 32-wide ones four 16-pixel groups per wave
    const int max_tw = p.ypool ? (WN >= 4 ? 32 : (WN >= 2 ? 16 : 8)) : 32;
    TileGeom g;
    if (!set_geom(p, g, BPX, KS, halo_max(KS, BPX), max_tw)) return PG_E_UNSUP;       // halo larger than the register-prefetch budget
    if ((long long)g.TN * (p.ups ? p.Hin >> 1 : p.Hin) * (p.ups ? p.Win >> 1 : p.Win) * p.Cin * 4 >= (1ll << 31)) return PG_E_UNSUP;   // 32-bit buffer offsets
    const size_t smem = (size_t)(KS * KS * BCO + g.halo) * KCP * sizeof(float);
    auto kern = conv_igemm_kernel<KS, VEC, WAVES_CO, WM, WN>;
    if (int rc = set_smem(kern, smem)) return rc;
    const int ncob = (p.Cout + BCO - 1) / BCO;
    const int nchunks = p.Cin / (4 * VEC);
    const int ksplit = g_tune[PG_TUNE_SPLITK] > 0 ? whole_slices(nchunks, g_tune[PG_TUNE_SPLITK]) : splitk_rule(g.ntiles * ncob, nchunks);
    if (ksplit > 1 && (p.yup || p.pn_r || p.pnb_y || p.mask_bytes || p.y_bytes || p.ysigns)) return PG_E_UNSUP;   // these epilogues need complete sums
    if ((p.pn_r || p.pnb_y) && (WAVES_CO != 1 || ncob != 1)) return PG_E_UNSUP;  // ... and every cout of a pixel inside one wave
    p.ksplit = ksplit;
    const size_t npix = (size_t)p.N * p.Hout * p.Wout;
    if (ksplit > 1) {
        hipError_t e = hipMemsetAsync(p.y, 0, npix * p.Cout * sizeof(float), s);
        if (e != hipSuccess) return (int)e;
    }
    dim3 grid(g.ntiles, ncob, ksplit);
    snprintf(g_last_kernel, sizeof(g_last_kernel), "conv_igemm_kernel<%d, %d, %d, %d, %d>", KS, VEC, WAVES_CO, WM, WN);
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, p);
    if (ksplit > 1) {
        const size_t total = npix * (p.Cout >> 2);
        int eg = (int)((total + 255) / 256); if (eg > 2048) eg = 2048;
        const bool identity = !p.mask && !p.bias && p.slope == 1.0f;
        if (!identity)
            hipLaunchKernelGGL(conv_epilogue_kernel, dim3(eg), dim3(256), 0, s, p.y, p.bias, p.mask, npix, p.Cout,
                               p.slope, p.mask_slope);
    }
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------
// Small-M layers (4x4 .. 16x16 at minibatch 3: a few hundred output pixels against K = 9*512).  The generic kernel
// has to slice K across workgroups there (memset + fp32 atomics + a deferred epilogue launch).  Here the FOUR WAVES of a
// workgroup split K instead: all waves own the same 16-cout x (16*WN)-pixel tile, wave w takes channels
// [64c + 16w, 64c + 16w + 16) of every 64-channel super-chunk (its own slice of the LDS rows), the four partial
// accumulators are summed through LDS and wave 0 runs the fused epilogue -- one launch, no atomics.
template <int WN>
__global__ __launch_bounds__(256) void conv_ksplit_kernel(ConvP p)
{
    // LDS row = 4 wave slices + 4 floats: with a row stride of 96 floats the 16 lanes (li) of a ds_read_b128 group sat on TWO
    // 4-bank groups (96 li mod 64 = 0 / 32: eight-way conflicts, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.65); 100 li mod 64
    // walks through all sixteen 4-bank groups
    constexpr int KS = 3, TAPS = 9, BCO = 16, BPX = 16 * WN, KCP = 24, RS = 4 * KCP + 4;
    constexpr int WEL = TAPS * BCO * 16;                        // float4 per weight super-chunk
    constexpr int WPT = (WEL + 255) / 256;
    constexpr int XMAX = BPX <= 16 ? 36 : (BPX * 9) / 4;
    constexpr int XPT = (XMAX * 16 + 255) / 256;
    extern __shared__ __align__(16) float lds[];
    const int TW = 1 << p.lgTW, TH = 1 << p.lgTH;
    const int HT = TH + KS - 1, WT = TW + KS - 1;
    float* wt = lds;                          // [TAPS][BCO][4][KCP]
    float* xt = lds + TAPS * BCO * RS;        // [TN*HT*WT][4][KCP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kk = lane >> 4;
    int t = blockIdx.x;
    const int tw_i = t % p.tilesW; t /= p.tilesW;
    const int th_i = t % p.tilesH; t /= p.tilesH;
    const int n0 = t * p.TN;
    const int oh0 = th_i << p.lgTH, ow0 = tw_i << p.lgTW;
    const int co0 = blockIdx.y * BCO;

    int pixbase[WN];
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        const int j = n * 16 + li;
        const int tw = j & (TW - 1), th = (j >> p.lgTW) & (TH - 1), tn = j >> (p.lgTW + p.lgTH);
        pixbase[n] = ((tn * HT + th) * WT + tw) * RS + wave * KCP + 4 * kk;
    }
    const int wbase = li * RS + wave * KCP + 4 * kk;

    const int npix = p.TN * HT * WT;
    int wsrc[WPT], wdst[WPT], xsrc[XPT], xdst[XPT], wch[WPT], xch[XPT];
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
        const int idx = tid + 256 * i;
        const int r = idx >> 4, v = idx & 15;                   // row (tap, cout), float4 index inside the 64 channels
        const int tap = r / BCO, col = r - tap * BCO, co = co0 + col;
        wdst[i] = idx < WEL ? r * RS + (v >> 2) * KCP + 4 * (v & 3) : -1;
        wsrc[i] = (idx < WEL && co < p.Cout) ? (tap * p.Cout + co) * p.Cin : -1;        // element offsets; -1 = zero fill
        wch[i] = 4 * v;
    }
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
        const int idx = tid + 256 * i;
        const int q = idx >> 4, v = idx & 15;
        const int r2 = (int)__umulhi((unsigned)q, p.mWT), tw = q - r2 * WT;
        const int tn = (int)__umulhi((unsigned)r2, p.mHT), th = r2 - tn * HT;
        const int n = n0 + tn;
        const int ih = oh0 + th - p.pad, iw = ow0 + tw - p.pad;
        const bool in_tile = q < npix;
        const bool ok = in_tile && n < p.N && (unsigned)ih < (unsigned)p.Hin && (unsigned)iw < (unsigned)p.Win;
        xdst[i] = in_tile ? q * RS + (v >> 2) * KCP + 4 * (v & 3) : -1;
        xsrc[i] = ok ? ((n * p.Hin + ih) * p.Win + iw) * p.Cin : -1;
        xch[i] = 4 * v;
    }
    int tapoff[TAPS];
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp) tapoff[tp] = ((tp / KS) * WT + (tp % KS)) * RS;

    f32x4 acc[WN];
#pragma unroll
    for (int n = 0; n < WN; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 acc_odd = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nsuper = (p.Cin + 63) >> 6;
    const __amdgpu_buffer_rsrc_t rx = pg_make_rsrc(p.x, (unsigned)((size_t)p.N * p.Hin * p.Win * p.Cin * 4));    // small-M layers: a few MB
    const __amdgpu_buffer_rsrc_t rw = pg_make_rsrc(p.w, (unsigned)((size_t)TAPS * p.Cout * p.Cin * 4));
    float4 wreg[WPT], xreg[XPT];
    auto fetch = [&](int sc) {
        const int k0 = sc << 6;
        // raw buffer loads (bufload.h): a select on the offset instead of a branch around every load
#pragma unroll
        for (int i = 0; i < WPT; ++i)
            wreg[i] = pg_buf_load4(rw, (wsrc[i] >= 0 && k0 + wch[i] < p.Cin) ? 4u * (unsigned)(wsrc[i] + k0 + wch[i]) : PG_OOB, 0);
#pragma unroll
        for (int i = 0; i < XPT; ++i)
            xreg[i] = pg_buf_load4(rx, (xsrc[i] >= 0 && k0 + xch[i] < p.Cin) ? 4u * (unsigned)(xsrc[i] + k0 + xch[i]) : PG_OOB, 0);
    };
    fetch(0);
    for (int sc = 0; sc < nsuper; ++sc) {
#pragma unroll
        for (int i = 0; i < WPT; ++i) if (wdst[i] >= 0) *reinterpret_cast<float4*>(wt + wdst[i]) = wreg[i];
#pragma unroll
        for (int i = 0; i < XPT; ++i) if (xdst[i] >= 0) *reinterpret_cast<float4*>(xt + xdst[i]) = xreg[i];
        __syncthreads();
        if (sc + 1 < nsuper) fetch(sc + 1);
        float a[2][4], b[2][WN][4];
        lds_load<4>(wt + wbase, a[0]);
#pragma unroll
        for (int n = 0; n < WN; ++n) lds_load<4>(xt + pixbase[n] + tapoff[0], b[0][n]);
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) {
            const int cur = tp & 1, nxt = cur ^ 1;
            if (tp + 1 < TAPS) {
                lds_load<4>(wt + (tp + 1) * BCO * RS + wbase, a[nxt]);
#pragma unroll
                for (int n = 0; n < WN; ++n) lds_load<4>(xt + pixbase[n] + tapoff[tp + 1], b[nxt][n]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                if constexpr (WN == 1) {                      // two accumulation chains: no adjacent dependent MFMAs
                    if (s4 & 1) acc_odd = MFMA16(a[cur][s4], b[cur][0][s4], acc_odd);
                    else acc[0] = MFMA16(a[cur][s4], b[cur][0][s4], acc[0]);
                } else {
#pragma unroll
                    for (int n = 0; n < WN; ++n) acc[n] = MFMA16(a[cur][s4], b[cur][n][s4], acc[n]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }
    if constexpr (WN == 1) acc[0] += acc_odd;
    // ---- sum the four K slices through LDS; wave 0 finishes
    float* red = lds;                                           // [3][WN][64][4]
    if (wave > 0) {
#pragma unroll
        for (int n = 0; n < WN; ++n)
            *reinterpret_cast<float4*>(red + (((wave - 1) * WN + n) * 64 + lane) * 4) = make_float4(acc[n][0], acc[n][1], acc[n][2], acc[n][3]);
    }
    __syncthreads();
    if (wave != 0) return;
    const int cb = co0 + 4 * kk;
    if (cb >= p.Cout) return;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p.bias) bv = *reinterpret_cast<const float4*>(p.bias + cb);
#pragma unroll
    for (int n = 0; n < WN; ++n) {
        float4 sacc = make_float4(acc[n][0], acc[n][1], acc[n][2], acc[n][3]);
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const float4 v = *reinterpret_cast<const float4*>(red + ((w * WN + n) * 64 + lane) * 4);
            sacc.x += v.x; sacc.y += v.y; sacc.z += v.z; sacc.w += v.w;
        }
        const int j = n * 16 + li;
        const int tw = j & (TW - 1), th = (j >> p.lgTW) & (TH - 1), tn = j >> (p.lgTW + p.lgTH);
        const int ni = n0 + tn;
        if (ni >= p.N) continue;
        const size_t off = (((size_t)ni * p.Hout + oh0 + th) * p.Wout + ow0 + tw) * p.Cout + cb;
        float4 o = make_float4(sacc.x * p.scale, sacc.y * p.scale, sacc.z * p.scale, sacc.w * p.scale);
        if (p.mask) {
            const float4 mk = *reinterpret_cast<const float4*>(p.mask + off);
            o.x *= mk.x > 0.f ? 1.f : p.mask_slope; o.y *= mk.y > 0.f ? 1.f : p.mask_slope;
            o.z *= mk.z > 0.f ? 1.f : p.mask_slope; o.w *= mk.w > 0.f ? 1.f : p.mask_slope;
        } else {
            o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
            o.x = o.x > 0.f ? o.x : o.x * p.slope; o.y = o.y > 0.f ? o.y : o.y * p.slope;
            o.z = o.z > 0.f ? o.z : o.z * p.slope; o.w = o.w > 0.f ? o.w : o.w * p.slope;
        }
        *reinterpret_cast<float4*>(p.y + off) = o;
    }
}

template <int WN>
int launch_ksplit(ConvP& p, hipStream_t s)
{
    constexpr int BPX = 16 * WN;
    // the kernel spells its prefetch budget "BPX <= 16 ? 36 : 9 BPX / 4" (a 16-pixel tile is 4 x 4 with a 6 x 6 halo): the same number
    static_assert(halo_max(3, BPX) == (BPX <= 16 ? 36 : (BPX * 9) / 4), "conv_ksplit_kernel's XMAX");
    TileGeom g;
    if (!set_geom(p, g, BPX, 3, halo_max(3, BPX))) return PG_E_UNSUP;
    if ((long long)p.N * p.Hin * p.Win * p.Cin * 4 >= (1ll << 31) || (long long)9 * p.Cout * p.Cin * 4 >= (1ll << 31)) return PG_E_UNSUP;   // 32-bit buffer offsets
    size_t smem = (size_t)(9 * 16 + g.halo) * 100 * sizeof(float);      // RS of the kernel
    const size_t red = (size_t)3 * WN * 256 * sizeof(float);
    if (red > smem) smem = red;
    auto kern = conv_ksplit_kernel<WN>;
    if (int rc = set_smem(kern, smem)) return rc;
    p.ksplit = 1;
    dim3 grid(g.ntiles, (p.Cout + 15) / 16);
    snprintf(g_last_kernel, sizeof(g_last_kernel), "conv_ksplit_kernel<%d>", WN);
    hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, p);
    return (int)hipGetLastError();
}

// Tile-shape selection.  A workgroup (4 waves, one per SIMD) runs for  L = chunks x (MFMA cycles per chunk + per-chunk
// overhead) + fixed cycles  when it has the CU to itself; r workgroups are resident per CU (LDS / VGPR limited) and
// share the matrix pipes, so a batch of r workgroups takes max(L, r x MFMA cycles) and the launch takes
// (batches over 256 CUs) x that.  Small tiles have a longer MFMA-free fraction per workgroup but far more residents,
// which is what wins on the 256/512-channel layers at minibatch 3; the constants were fitted to a sweep of every
// candidate over every layer shape of the schedule (tools/sweeps/sweep_conv_all.py, tools/sweeps/fit_cost_model.py: 0.7 % regret).
// Shapes with < 192 workgroups are K-split in launch_conv (memset + atomics + deferred epilogue: fixed penalty).
struct TileCand { int bpx, bco; };

template <int KS, int VEC>
int dispatch_conv(ConvP& p, hipStream_t s)
{
    if constexpr (KS == 4) {
        return launch_conv<KS, VEC, 4, 1, 1>(p, s);               // 16-tap halo: keep the pixel tile small
    } else {
        if constexpr (VEC == 4) {
            const long long Mpx = (long long)p.N * p.Hout * p.Wout;
            // (conv_ksplit_kernel's epilogue knows fp32 masks only: sign-byte masks / outputs keep the generic tile kernel)
            if (!p.ups && !p.ypool && !p.yup && !p.pn_r && !p.pnb_y && !p.mask_bytes && !p.y_bytes && !p.ysigns && p.Cin >= 128 && g_tune[PG_TUNE_CONV_TILE] < 0 &&
                g_tune[PG_TUNE_PATH] != PG_PATH_NO_SMALLMAP_SPLIT && Mpx <= (g_tune[PG_TUNE_PATH] == PG_PATH_SMALLMAP_SPLIT_2304 ? 2304 : 576)) {
                const int rc = Mpx <= 256 ? launch_ksplit<1>(p, s) : launch_ksplit<2>(p, s);
                if (rc != PG_E_UNSUP) return rc;
            }
        }
        static const TileCand cands[] = {{256, 16}, {128, 64}, {128, 32}, {128, 16}, {64, 64}, {64, 32}, {64, 16}, {16, 64}};
        // registers per lane of each instantiation (hipcc 7.2, KS = 3): residency = min(LDS, 512 / vgpr)
        static const int vgpr4[] = {160, 200, 128, 100, 164, 100, 68, 92};
        static const int vgpr2[] = {120, 144, 92, 76, 120, 76, 52, 60};
        static const int vgpr1[] = {88, 112, 72, 52, 88, 56, 32, 48};
        const int* vg = VEC == 4 ? vgpr4 : (VEC == 2 ? vgpr2 : vgpr1);
        constexpr int KCP = RowStride<VEC>::value;
        const int nchunks = p.Cin / (4 * VEC);
        double best = 1e30; int bi = 1;
        for (int i = 0; i < 8; ++i) {
            const TileCand c = cands[i];
            if (c.bpx == 256 && p.Cout > 16) continue;            // 256-pixel tiles only exist for <= 16 couts
            if (c.bco > 16 && p.Cout <= 16) continue;
            if (c.bco > 32 && p.Cout <= 32) continue;
            if ((p.pn_r || p.pnb_y) && (c.bco < p.Cout || i == 1 || i == 4 || i == 5 || i == 7)) continue;   // fused PixelNorm: one wave row of couts
            const TileGeom g = make_geom(p.N, p.Hout, p.Wout, c.bpx, KS);
            const long long lds = (long long)(KS * KS * c.bco + g.halo) * KCP * 4;
            long long r = 160 * 1024 / lds;
            if (r > 512 / vg[i]) r = 512 / vg[i];
            if (r > 8) r = 8;
            if (r < 1) r = 1;
            const long long blocks = (long long)g.ntiles * ((p.Cout + c.bco - 1) / c.bco);
            const long long ks = splitk_rule(blocks, nchunks);    // what launch_conv will do
            const long long cper = (nchunks + ks - 1) / ks;
            const long long wgs = blocks * ks;
            const double mfma_chunk = (double)(c.bpx / 16) * (c.bco / 16) / 4.0 * VEC * KS * KS * 32.0;
            const double mfma_wg = mfma_chunk * (double)cper;
            const double L = (double)cper * (mfma_chunk + 300.0) + 1500.0 + (ks > 1 ? 5.0 * c.bpx * c.bco + 2000.0 : 0.0);
            const long long full = wgs / (256 * r), rem = wgs % (256 * r);
            double cost = (double)full * (L > r * mfma_wg ? L : r * mfma_wg);
            if (rem) {
                const double rr = (double)((rem + 255) / 256);
                cost += L > rr * mfma_wg ? L : rr * mfma_wg;
            }
            if (ks > 1) cost += 8000.0;
            if (cost < best) { best = cost; bi = i; }
        }
        if (g_tune[PG_TUNE_CONV_TILE] >= 0) bi = g_tune[PG_TUNE_CONV_TILE];
        switch (bi) {
            case 0: return launch_conv<KS, VEC, 1, 1, 4>(p, s);
            case 1: return launch_conv<KS, VEC, 2, 2, 4>(p, s);
            case 2: return launch_conv<KS, VEC, 1, 2, 2>(p, s);
            case 3: return launch_conv<KS, VEC, 1, 1, 2>(p, s);
            case 4: return launch_conv<KS, VEC, 4, 1, 4>(p, s);
            case 5: return launch_conv<KS, VEC, 2, 1, 2>(p, s);
            case 6: return launch_conv<KS, VEC, 1, 1, 1>(p, s);
            default: return launch_conv<KS, VEC, 4, 1, 1>(p, s);
        }
    }
}

template <int KS>
int dispatch_conv_vec(ConvP& p, hipStream_t s)
{
    if ((p.Cin & 15) == 0) return dispatch_conv<KS, 4>(p, s);
    if ((p.Cin & 7) == 0) return dispatch_conv<KS, 2>(p, s);
    return dispatch_conv<KS, 1>(p, s);
}

}  // namespace

int pgk::dispatch_conv_tile(ConvP& p, hipStream_t s)
{
    switch (p.KS) {
        case 1: return dispatch_conv_vec<1>(p, s);
        case 3: return dispatch_conv_vec<3>(p, s);
        case 4: return dispatch_conv_vec<4>(p, s);
        default: return PG_E_UNSUP;
    }
}
