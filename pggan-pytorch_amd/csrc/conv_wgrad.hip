// Weight (+ bias) gradient of the equalized-lr convolution on the tile geometry of conv_igemm.hip (gfx950 / CDNA4).
//
// Owns: conv_wgrad_kernel (16x16x4 MFMA over pixels) with launch_wgrad; conv_wgrad_thin_kernel (4x4x1 block MFMA of the
// 8/16-channel layers) with launch_wgrad_thin, which hands the strip-sized maps to conv_strip.hip first; dispatch_wgrad; the
// entry points pg_conv2d_wgrad_nhwc and pg_conv2d_wgrad_unpooled_nhwc; the PG_WINO_TRACE phase stamps of the thin kernel
// (pg_debug_wgrad_trace, tools/exp/wgrad_trace.py).  The 4x4 boundary layers go to conv_k4.hip.
#include "convp.h"

namespace {

using namespace pgk;

#ifdef PG_WINO_TRACE
#define PG_WSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); if (p.trace && lane == 0 && blockIdx.x < 1024 && (tile - t_begin) < 8) \
    p.trace[((size_t)(blockIdx.x * 4 + wave) * 8 + (tile - t_begin)) * 8 + (i)] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
thread_local unsigned long long* g_wgrad_trace = nullptr;
#else
#define PG_WSTAMP(i) do { } while (0)
#endif

// dW[tap][co][ci] = sum over pixels: A = gz (row i = cout), B = shifted x (col j = cin), the MFMA
// k index runs over PIXELS (4 per instruction).  One workgroup owns a (BCO x BCI) block of every
// tap and a slice of the pixel tiles; its WAVES_K waves split the pixels of a tile and are reduced
// through LDS before ONE commit per workgroup (plain += when it is the only writer, else atomics).
template <int KS, int WM, int WN, int WAVES_CO, int WAVES_CI, int BPX>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgP p)
{
    constexpr int WAVES_K = 4 / (WAVES_CO * WAVES_CI);
    constexpr int BCO = 16 * WM * WAVES_CO, BCI = 16 * WN * WAVES_CI;
    constexpr int SZ = PixStride<BCO>::value, SX = PixStride<BCI>::value;
    constexpr int TAPS = KS * KS;
    constexpr int ZV = BCO / 4, XV = BCI / 4;
    constexpr int ZPT = (BPX * ZV + 255) / 256;
    constexpr int XMAX = KS == 1 ? BPX : (KS == 3 ? (BPX * 9) / 4 : 16 * BPX);
    constexpr int XPT = (XMAX * XV + 255) / 256;
    extern __shared__ __align__(16) float lds[];

    const int TW = 1 << p.lgTW, TH = 1 << p.lgTH;
    const int HT = TH + KS - 1, WT = TW + KS - 1;
    float* gzt = lds;                        // [BPX][SZ]
    float* xt = lds + BPX * SZ;              // [TN*HT*WT][SX]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_co = wave % WAVES_CO, wave_ci = (wave / WAVES_CO) % WAVES_CI, wave_k = wave / (WAVES_CO * WAVES_CI);
    const int li = lane & 15, kk = lane >> 4;
    const int co0 = blockIdx.y * BCO, ci0 = blockIdx.z * BCI;
    const bool do_bias = (p.db != nullptr) && blockIdx.z == 0 && wave_ci == 0;

    f32x4 acc[TAPS][WM][WN];
    f32x4 accb[WM];
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
        for (int m = 0; m < WM; ++m)
#pragma unroll
            for (int n = 0; n < WN; ++n) acc[tp][m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < WM; ++m) accb[m] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int xH = p.ups ? (p.Hin >> 1) : p.Hin, xW = p.ups ? (p.Win >> 1) : p.Win;
    const int npix = p.TN * HT * WT;

    // ---- per-thread load descriptors: tile-relative coordinates (no div/mod in the tile loop)
    int zq[ZPT], zc[ZPT];                    // pixel-in-tile, cout offset
    int xq[XPT], xc[XPT], xdst[XPT];         // packed (tn,th,tw) of the halo pixel, cin offset, LDS offset
#pragma unroll
    for (int i = 0; i < ZPT; ++i) {
        const int idx = tid + 256 * i;
        const int q = idx / ZV, v = idx - q * ZV;
        zq[i] = idx < BPX * ZV ? q : -1;
        zc[i] = co0 + 4 * v;
    }
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
        const int idx = tid + 256 * i;
        const int q = idx / XV, v = idx - q * XV;
        const int r2 = (int)__umulhi((unsigned)q, p.mWT), tw = q - r2 * WT;
        const int tn = (int)__umulhi((unsigned)r2, p.mHT), th = r2 - tn * HT;
        xq[i] = q < npix ? ((tn << 20) | (th << 10) | tw) : -1;
        xc[i] = ci0 + 4 * v;
        xdst[i] = q * SX + 4 * v;
    }
    int tapoff[TAPS];
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp) tapoff[tp] = ((tp / KS) * WT + (tp % KS)) * SX;

    float4 zreg[ZPT], xreg[XPT];
    auto fetch = [&](int tile) {
        int t = tile;
        const int tw_i = t % p.tilesW; t /= p.tilesW;
        const int th_i = t % p.tilesH; t /= p.tilesH;
        const int n0 = t * p.TN;
        const int oh0 = th_i << p.lgTH, ow0 = tw_i << p.lgTW;
#pragma unroll
        for (int i = 0; i < ZPT; ++i) {
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (zq[i] >= 0) {
                const int q = zq[i];
                const int tw = q & (TW - 1), th = (q >> p.lgTW) & (TH - 1), tn = q >> (p.lgTW + p.lgTH);
                const int n = n0 + tn;
                if (n < p.N && zc[i] < p.Cout)
                    val = *reinterpret_cast<const float4*>(p.gz + (((size_t)n * p.Hout + oh0 + th) * p.Wout + ow0 + tw) * p.Cout + zc[i]);
            }
            zreg[i] = val;
        }
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
            if (xq[i] >= 0) {
                const int tw = xq[i] & 1023, th = (xq[i] >> 10) & 1023, tn = xq[i] >> 20;
                const int n = n0 + tn;
                int ih = oh0 + th - p.pad, iw = ow0 + tw - p.pad;
                if (n < p.N && xc[i] < p.Cin && (unsigned)ih < (unsigned)p.Hin && (unsigned)iw < (unsigned)p.Win) {
                    if (p.ups) { ih >>= 1; iw >>= 1; }
                    val = *reinterpret_cast<const float4*>(p.x + (((size_t)n * xH + ih) * xW + iw) * p.Cin + xc[i]);
                }
            }
            xreg[i] = val;
        }
    };

    const int t_begin = (int)pg_xcd_remap(blockIdx.x, gridDim.x) * p.tiles_per_block;   // neighbouring tile ranges on one XCD
    const int t_end = min(t_begin + p.tiles_per_block, p.ntiles);
    constexpr int NSTEPS = BPX / 4;

    if (t_begin < t_end) fetch(t_begin);
    for (int tile = t_begin; tile < t_end; ++tile) {
#pragma unroll
        for (int i = 0; i < ZPT; ++i)
            if (zq[i] >= 0) *reinterpret_cast<float4*>(gzt + zq[i] * SZ + (zc[i] - co0)) = zreg[i];
#pragma unroll
        for (int i = 0; i < XPT; ++i)
            if (xq[i] >= 0) *reinterpret_cast<float4*>(xt + xdst[i]) = xreg[i];
        __syncthreads();
        if (tile + 1 < t_end) fetch(tile + 1);            // in flight while the MFMAs below run

        // k-steps of this wave: step = wave_k, wave_k + WAVES_K, ...  (4 pixels each, same tile row)
        auto frag_addr = [&](int step, int& aoff, int& boff) {
            const int q = 4 * step + kk;
            const int tw = q & (TW - 1), th = (q >> p.lgTW) & (TH - 1), tn = q >> (p.lgTW + p.lgTH);
            aoff = q * SZ + wave_co * WM * 16 + li;
            boff = ((tn * HT + th) * WT + tw) * SX + wave_ci * WN * 16 + li;
        };
        float a[2][WM], b[2][TAPS][WN];
        auto load_frags = [&](int step, float (&af)[WM], float (&bf)[TAPS][WN]) {
            int ao, bo; frag_addr(step, ao, bo);
#pragma unroll
            for (int m = 0; m < WM; ++m) af[m] = gzt[ao + m * 16];
#pragma unroll
            for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
                for (int n = 0; n < WN; ++n) bf[tp][n] = xt[bo + tapoff[tp] + n * 16];
        };
        auto mfmas = [&](const float (&af)[WM], const float (&bf)[TAPS][WN]) {
            if (do_bias) {
#pragma unroll
                for (int m = 0; m < WM; ++m) accb[m] = MFMA16(af[m], 1.0f, accb[m]);
            }
#pragma unroll
            for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
                for (int m = 0; m < WM; ++m)
#pragma unroll
                    for (int n = 0; n < WN; ++n) acc[tp][m][n] = MFMA16(af[m], bf[tp][n], acc[tp][m][n]);
        };
        constexpr int T = NSTEPS / WAVES_K;              // even for every instantiated shape
        static_assert(T % 2 == 0, "k-steps per wave must be even");
        load_frags(wave_k, a[0], b[0]);
        for (int s = 0; s < T; s += 2) {                 // ping-pong: next step's LDS reads under this step's MFMAs
            load_frags(wave_k + (s + 1) * WAVES_K, a[1], b[1]);
            __builtin_amdgcn_sched_barrier(0);           // keep the reads ahead of the MFMAs (see conv_igemm_kernel)
            mfmas(a[0], b[0]);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 2 < T) load_frags(wave_k + (s + 2) * WAVES_K, a[0], b[0]);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(a[1], b[1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
    }

    // ---- reduce the WAVES_K partial sums through LDS (tile buffers are free now), then commit once
    if (WAVES_K > 1) {
        // layout: red[(wave_co,wave_ci)][tile index t = (tp*WM+m)*WN+n (+bias tiles)][lane*4+r]
        constexpr int NT = TAPS * WM * WN + WM;
        float* red = lds + (wave_co + WAVES_CO * wave_ci) * NT * 256;
        for (int w = 0; w < WAVES_K; ++w) {
            if (wave_k == w) {
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
                    for (int m = 0; m < WM; ++m)
#pragma unroll
                        for (int n = 0; n < WN; ++n) {
                            float4* r4 = reinterpret_cast<float4*>(red + (((tp * WM + m) * WN + n) * 64 + lane) * 4);
                            float4 v = make_float4(acc[tp][m][n][0], acc[tp][m][n][1], acc[tp][m][n][2], acc[tp][m][n][3]);
                            if (w > 0) { const float4 o = *r4; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                            if (w == WAVES_K - 1) acc[tp][m][n] = f32x4{v.x, v.y, v.z, v.w}; else *r4 = v;
                        }
#pragma unroll
                for (int m = 0; m < WM; ++m) {
                    float4* r4 = reinterpret_cast<float4*>(red + ((TAPS * WM * WN + m) * 64 + lane) * 4);
                    float4 v = make_float4(accb[m][0], accb[m][1], accb[m][2], accb[m][3]);
                    if (w > 0) { const float4 o = *r4; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
                    if (w == WAVES_K - 1) accb[m] = f32x4{v.x, v.y, v.z, v.w}; else *r4 = v;
                }
            }
            __syncthreads();
        }
        if (wave_k != WAVES_K - 1) return;
    }

    // commit: C/D fragment row = 4*kk + reg -> cout, col = li -> cin
#pragma unroll
    for (int m = 0; m < WM; ++m) {
#pragma unroll
        for (int n = 0; n < WN; ++n) {
            const int ci = ci0 + (wave_ci * WN + n) * 16 + li;
            if (ci >= p.Cin) continue;
#pragma unroll
            for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = co0 + (wave_co * WM + m) * 16 + 4 * kk + r;
                    if (co < p.Cout) {
                        float* dst = p.dw + ((size_t)(tp * p.Cout + co) * p.Cin + ci);
                        const float v = acc[tp][m][n][r] * p.scale;
                        if (p.atomic) atomicAdd(dst, v); else *dst += v;
                    }
                }
        }
        if (do_bias && li == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + (wave_co * WM + m) * 16 + 4 * kk + r;
                if (co < p.Cout) { if (p.atomic) atomicAdd(p.db + co, accb[m][r]); else p.db[co] += accb[m][r]; }
            }
        }
    }
}

template <int KS, int WM, int WN, int WAVES_CO, int WAVES_CI, int BPX>
int launch_wgrad(WgP& p, hipStream_t s)
{
    constexpr int WAVES_K = 4 / (WAVES_CO * WAVES_CI);
    constexpr int BCO = 16 * WM * WAVES_CO, BCI = 16 * WN * WAVES_CI;
    constexpr int SZ = PixStride<BCO>::value, SX = PixStride<BCI>::value;
    static_assert(BPX < 512, "the kernel's XMAX is halo_max without its 32-wide form of >= 512-pixel tiles");
    TileGeom g;
    if (!set_geom(p, g, BPX, KS, halo_max(KS, BPX))) return PG_E_UNSUP;
    size_t smem = ((size_t)BPX * SZ + (size_t)g.halo * SX) * sizeof(float);
    const size_t red = WAVES_K > 1 ? (size_t)WAVES_CO * WAVES_CI * (KS * KS * WM * WN + WM) * 256 * sizeof(float) : 0;
    if (red > smem) smem = red;
    const int gy = (p.Cout + BCO - 1) / BCO, gz_ = (p.Cin + BCI - 1) / BCI;
    int chunks = (512 + gy * gz_ - 1) / (gy * gz_);        // ~512 workgroups: fills 256 CUs twice over while
    if (g_tune[PG_TUNE_SPLITK] > 0) chunks = g_tune[PG_TUNE_SPLITK];                 // (tuning sweep)
    if (chunks > g.ntiles) chunks = g.ntiles;              // keeping the commit traffic (chunks x |dW|) small
    if (chunks < 1) chunks = 1;
    p.tiles_per_block = (g.ntiles + chunks - 1) / chunks;
    chunks = (g.ntiles + p.tiles_per_block - 1) / p.tiles_per_block;
    p.atomic = 1;        // fire-and-forget L2 atomics even for a sole writer: a load-add-store commit serialises on the load latency (+5 us per launch)
    auto kern = conv_wgrad_kernel<KS, WM, WN, WAVES_CO, WAVES_CI, BPX>;
    if (int rc = set_smem(kern, smem)) return rc;
    snprintf(g_last_kernel, sizeof(g_last_kernel), "conv_wgrad_kernel<%d, %d, %d, %d, %d, %d>", KS, WM, WN, WAVES_CO, WAVES_CI, BPX);
    hipLaunchKernelGGL(kern, dim3(chunks, gy, gz_), dim3(256), smem, s, p);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------
// Weight gradient of the 8-channel layers (8->8, 8->16, 16->8 at 1024^2): a 16x16x4 MFMA tile would be 75 % / 50 %
// zero padding.  v_mfma_f32_4x4x1_16B_f32 computes SIXTEEN independent 4x4 outer products per instruction at the
// same FLOP rate: the CO x CI outer product of one pixel is NB = (CO/4)*(CI/4) blocks, so one instruction takes
// 16/NB pixels (4 for 8x8, 2 for 8x16) with every lane doing useful work.  Lane l: block b = l>>2, A row / B col
// = l&3; D register r of lane 4b+j is element [r][j] of block b.  Blocks of the same (co-quad, ci-quad) but
// different pixel slot are separate accumulators, summed by xor-shuffles before the workgroup reduction.
// FIX: the tile is 16 x 4 pixels of one image (every layer this kernel serves from 16 x 16 maps up): the k-step -> LDS address map is
// then a per-lane base plus compile-time constants, i.e. immediate offsets of the ds_reads instead of ~12 VALU instructions per k-step
// (rocprofv3 SQ_INSTS_VALU per wave, 8->16 @1024^2 n9: 9.2 k non-MFMA VALU next to 10.4 k MFMAs before).
template <int CO, int CI, int BPX, bool FIX>
__global__ __launch_bounds__(256) void conv_wgrad_thin_kernel(WgP p)
{
    constexpr int KS = 3, TAPS = 9;
    constexpr int QO = CO / 4, QI = CI / 4, NB = QO * QI;
    constexpr int PPM = NB <= 16 ? 16 / NB : 1;                  // pixels per MFMA
    constexpr int GQ = NB <= 16 ? 1 : NB / 16;                   // MFMAs (groups of 16 blocks) per pixel and tap
    static_assert(NB <= 16 || (16 % QI) == 0, "the B operand must be shared by the block groups");
    constexpr int SZ = PixStride<CO>::value, SX = PixStride<CI>::value;
    constexpr int ZV = CO / 4, XV = CI / 4;
    constexpr int ZPT = (BPX * ZV + 255) / 256;
    constexpr int XMAX = (BPX * 9) / 4;
    constexpr int XPT = (XMAX * XV + 255) / 256;
    extern __shared__ __align__(16) float lds[];

    static_assert(!FIX || BPX == 64, "the fixed geometry is 16 x 4 pixels");
    const int TW = FIX ? 16 : 1 << p.lgTW, TH = FIX ? 4 : 1 << p.lgTH;
    const int HT = TH + KS - 1, WT = TW + KS - 1;
    float* gzt = lds;                        // [BPX][SZ]
    float* xt = lds + BPX * SZ;              // [TN*HT*WT][SX]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = lane >> 2, i4 = lane & 3;
    const int hi = blk % QI, slot = NB <= 16 ? blk / NB : 0;     // group q of this lane: cout quad (16q + blk) / QI
    int ho[GQ];
#pragma unroll
    for (int q = 0; q < GQ; ++q) ho[q] = ((16 * q + blk) / QI) % QO;
    const bool do_bias = p.db != nullptr;

    f32x4 acc[GQ][TAPS];
    float bsum[GQ];
#pragma unroll
    for (int q = 0; q < GQ; ++q) {
        bsum[q] = 0.f;
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp) acc[q][tp] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const int npix = p.TN * HT * WT;
    const int xH = p.ups ? (p.Hin >> 1) : p.Hin, xW = p.ups ? (p.Win >> 1) : p.Win;
    // Per-thread load descriptors, computed ONCE: byte offsets relative to the tile origin (the per-tile part of every address
    // is a wave-uniform scalar) and, for the halo pixels of x, which tile edge they sit on.  The phase trace of round 2
    // (tools/exp/wgrad_trace.py) showed the per-tile address arithmetic of the previous version (integer divisions of the tile
    // index, per-load multiplies and range checks) costing 1400 of the 3700 cycles a tile took.
    int zq[ZPT], zc[ZPT];
    int xdst[XPT];
    unsigned zrel[ZPT], brel[ZPT];
    int xrel[XPT], xedge[XPT];                                   // xedge: bit 0 top, 1 bottom, 2 left, 3 right halo; -1 = unused slot
    const int zH = p.gbytes ? (p.Hout >> 1) : p.Hout, zW = p.gbytes ? (p.Wout >> 1) : p.Wout;
#pragma unroll
    for (int i = 0; i < ZPT; ++i) {
        const int idx = tid + 256 * i;
        const int q = idx / ZV, v = idx - q * ZV;
        zq[i] = idx < BPX * ZV ? q : -1;
        zc[i] = 4 * v;
        const int tw = q & (TW - 1), th = (q >> p.lgTW) & (TH - 1), tn = q >> (p.lgTW + p.lgTH);
        const int zh = p.gbytes ? (th >> 1) : th, zw = p.gbytes ? (tw >> 1) : tw;
        zrel[i] = zq[i] >= 0 ? 4u * (unsigned)(((tn * zH + zh) * zW + zw) * CO + 4 * v) : PG_OOB;
        brel[i] = (unsigned)(((tn * p.Hout + th) * p.Wout + tw) * (CO / 4) + v);
    }
#pragma unroll
    for (int i = 0; i < XPT; ++i) {
        const int idx = tid + 256 * i;
        const int q = idx / XV, v = idx - q * XV;
        const int r2 = (int)__umulhi((unsigned)q, p.mWT), tw = q - r2 * WT;
        const int tn = (int)__umulhi((unsigned)r2, p.mHT), th = r2 - tn * HT;
        xdst[i] = q * SX + 4 * v;
        int ih = th - p.pad, iw = tw - p.pad;
        if (p.ups) { ih >>= 1; iw >>= 1; }                       // nearest-x2 upsample fused into the gather (tile origins are even)
        xrel[i] = 4 * (((tn * xH + ih) * xW + iw) * CI + 4 * v);
        xedge[i] = q < npix ? ((th < p.pad ? 1 : 0) | (th >= TH + p.pad ? 2 : 0) | (tw < p.pad ? 4 : 0) | (tw >= TW + p.pad ? 8 : 0)) : -1;
    }
    int tapoff[TAPS];
#pragma unroll
    for (int tp = 0; tp < TAPS; ++tp) tapoff[tp] = ((tp / KS) * WT + (tp % KS)) * SX;
    int abase[GQ], bbase;                                        // FIX: LDS offsets of this lane's fragments at k-step 0
    {
        const int q0 = PPM * wave + slot;
#pragma unroll
        for (int g = 0; g < GQ; ++g) abase[g] = q0 * SZ + 4 * ho[g] + i4;
        bbase = q0 * SX + 4 * hi + i4;
    }

    float4 zreg[ZPT], xreg[XPT];
    unsigned char zb[ZPT];                   // sign bytes of the prefetched gz values (pool adjoint in the gather)
#pragma unroll
    for (int i = 0; i < ZPT; ++i) zb[i] = 0;
    const size_t zimg = (size_t)zH * zW * CO, ximg = (size_t)xH * xW * CI;
    int f_tw = 0, f_th = 0, f_n = 0;         // tile coordinates of the NEXT fetch (tiles are fetched in order: no divisions per tile)
    auto fetch_seek = [&](int tile) {
        int t = tile;
        f_tw = t % p.tilesW; t /= p.tilesW;
        f_th = t % p.tilesH; f_n = t / p.tilesH;
    };
    auto fetch = [&]() {
        const int n0 = f_n * p.TN;
        const int oh0 = f_th << p.lgTH, ow0 = f_tw << p.lgTW;
        // raw buffers over the TN images of this tile (bufload.h): PG_OOB / beyond-the-records = zero fill, no branch per load
        const int nimg = min(p.TN, p.N - n0);
        const __amdgpu_buffer_rsrc_t rz = pg_make_rsrc(p.gz + (size_t)n0 * zimg, (unsigned)((size_t)nimg * zimg * 4));
        const __amdgpu_buffer_rsrc_t rx = pg_make_rsrc(p.x + (size_t)n0 * ximg, (unsigned)((size_t)nimg * ximg * 4));
        const unsigned zorg = 4u * (unsigned)((((p.gbytes ? oh0 >> 1 : oh0) * zW) + (p.gbytes ? ow0 >> 1 : ow0)) * CO);
        const int xorg = 4 * ((((p.ups ? oh0 >> 1 : oh0) * xW) + (p.ups ? ow0 >> 1 : ow0)) * CI);
        // tile edges that coincide with the image border: their halo pixels are outside the image
        const int border = (oh0 == 0 ? 1 : 0) | (oh0 + TH >= p.Hout ? 2 : 0) | (ow0 == 0 ? 4 : 0) | (ow0 + TW >= p.Wout ? 8 : 0);
#pragma unroll
        for (int i = 0; i < ZPT; ++i) {
            zreg[i] = pg_buf_load4(rz, zrel[i], zorg);
            if (p.gbytes) {
                // the byte is applied when the prefetched value is stored to LDS (next iteration): a multiply here would
                // wait for the load and serialise the register prefetch
                const bool ok = zq[i] >= 0 && (zq[i] >> (p.lgTW + p.lgTH)) < nimg;
                zb[i] = ok ? p.gbytes[((size_t)n0 * p.Hout + oh0) * p.Wout * (CO / 4) + (size_t)ow0 * (CO / 4) + brel[i]] : (unsigned char)0;
            }
        }
#pragma unroll
        for (int i = 0; i < XPT; ++i) {
            const bool ok = xedge[i] >= 0 && (xedge[i] & border) == 0;
            xreg[i] = pg_buf_load4(rx, ok ? (unsigned)(xrel[i] + xorg) : PG_OOB, 0);
        }
        if (++f_tw == p.tilesW) { f_tw = 0; if (++f_th == p.tilesH) { f_th = 0; ++f_n; } }
    };

    const int t_begin = (int)pg_xcd_remap(blockIdx.x, gridDim.x) * p.tiles_per_block;   // neighbouring tile ranges on one XCD
    const int t_end = min(t_begin + p.tiles_per_block, p.ntiles);
    constexpr int NSTEPS = BPX / PPM, T = NSTEPS / 4;            // k-steps per tile / per wave

    fetch_seek(t_begin);
    if (t_begin < t_end) fetch();
    for (int tile = t_begin; tile < t_end; ++tile) {
        PG_WSTAMP(0);
#pragma unroll
        for (int i = 0; i < ZPT; ++i)
            if (zq[i] >= 0) {
                float4 v = zreg[i];
                if (p.gbytes) {
                    const float4 f = pg_sign_factors(zb[i], p.gslope);
                    v.x *= f.x * p.gmul; v.y *= f.y * p.gmul; v.z *= f.z * p.gmul; v.w *= f.w * p.gmul;
                }
                *reinterpret_cast<float4*>(gzt + zq[i] * SZ + zc[i]) = v;
            }
#pragma unroll
        for (int i = 0; i < XPT; ++i)
            if (xedge[i] >= 0) *reinterpret_cast<float4*>(xt + xdst[i]) = xreg[i];
        PG_WSTAMP(1);
        __syncthreads();
        PG_WSTAMP(2);
        if (tile + 1 < t_end) fetch();
        PG_WSTAMP(3);

        auto load_frags = [&](int kstep, float (&af)[GQ], float (&bf)[TAPS]) {      // k-step of this wave: step = wave + 4 kstep
            if constexpr (FIX) {
                // pixel q = q0 + 4 PPM kstep with q0 = PPM wave + slot < 4 PPM <= 16: q0 stays inside tile row 0, kstep walks along the
                // row (16 / (4 PPM) steps) and then down: every offset below is a per-lane base + a compile-time constant
                constexpr int PER_ROW = 16 / (4 * PPM);
                const int th = kstep / PER_ROW, dw_ = (kstep % PER_ROW) * 4 * PPM;
#pragma unroll
                for (int g = 0; g < GQ; ++g) af[g] = gzt[abase[g] + (th * 16 + dw_) * SZ];
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp) bf[tp] = xt[bbase + ((th + tp / KS) * 18 + dw_ + tp % KS) * SX];
            } else {
                const int q = PPM * (wave + 4 * kstep) + slot;
                const int tw = q & (TW - 1), th = (q >> p.lgTW) & (TH - 1), tn = q >> (p.lgTW + p.lgTH);
#pragma unroll
                for (int g = 0; g < GQ; ++g) af[g] = gzt[q * SZ + 4 * ho[g] + i4];
                const int bo = ((tn * HT + th) * WT + tw) * SX + 4 * hi + i4;
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp) bf[tp] = xt[bo + tapoff[tp]];
            }
        };
        auto mfmas = [&](const float (&af)[GQ], const float (&bf)[TAPS]) {
#pragma unroll
            for (int g = 0; g < GQ; ++g) {
                bsum[g] += af[g];
#pragma unroll
                for (int tp = 0; tp < TAPS; ++tp) acc[g][tp] = __builtin_amdgcn_mfma_f32_4x4x1f32(af[g], bf[tp], acc[g][tp], 0, 0, 0);
            }
        };
        float a[2][GQ], b[2][TAPS];
        static_assert(T % 2 == 0, "k-steps per wave must be even");
        load_frags(0, a[0], b[0]);
#pragma unroll
        for (int s2 = 0; s2 < T; s2 += 2) {
            load_frags(s2 + 1, a[1], b[1]);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(a[0], b[0]);
            __builtin_amdgcn_sched_barrier(0);
            if (s2 + 2 < T) load_frags(s2 + 2, a[0], b[0]);
            __builtin_amdgcn_sched_barrier(0);
            mfmas(a[1], b[1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        PG_WSTAMP(4);
        __syncthreads();
        PG_WSTAMP(5);
    }

    // ---- sum the pixel slots (lanes 4*NB apart), then the 4 waves through LDS, then ONE commit per workgroup
#pragma unroll
    for (int g = 0; g < GQ; ++g) {
#pragma unroll
        for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[g][tp][r];
                if (PPM >= 2) v += __shfl_xor(v, 32, 64);
                if (PPM >= 4) v += __shfl_xor(v, 16, 64);
                acc[g][tp][r] = v;
            }
        if (PPM >= 2) bsum[g] += __shfl_xor(bsum[g], 32, 64);
        if (PPM >= 4) bsum[g] += __shfl_xor(bsum[g], 16, 64);
    }
    constexpr int NL = NB <= 16 ? 4 * NB : 64;                   // lanes holding distinct results
    constexpr int NE = GQ * (TAPS * 4 + 1);                      // values per lane: [group][tap*4 + r | bias]
    float* red = lds;                                            // [wave][NE][NL]
    if (lane < NL) {
#pragma unroll
        for (int g = 0; g < GQ; ++g) {
#pragma unroll
            for (int tp = 0; tp < TAPS; ++tp)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[(wave * NE + g * (TAPS * 4 + 1) + tp * 4 + r) * NL + lane] = acc[g][tp][r];
            red[(wave * NE + g * (TAPS * 4 + 1) + TAPS * 4) * NL + lane] = bsum[g];
        }
    }
    __syncthreads();
    // one thread per element sums the four waves and commits
    for (int e = tid; e < NE * NL; e += 256) {
        const int l = e % NL, ve = e / NL;
        const int g = ve / (TAPS * 4 + 1), slot_e = ve % (TAPS * 4 + 1);   // slot_e = tp*4 + r, or TAPS*4 for the bias
        const float v = (red[e] + red[e + NE * NL]) + (red[e + 2 * NE * NL] + red[e + 3 * NE * NL]);
        const int b_ = l >> 2, j = l & 3;
        const int hi_ = b_ % QI, ho_ = ((16 * g + b_) / QI) % QO;
        if (slot_e < TAPS * 4) {
            const int tp = slot_e >> 2, r = slot_e & 3;
            float* dst = p.dw + ((size_t)(tp * CO + 4 * ho_ + r) * CI + 4 * hi_ + j);
            if (p.atomic) atomicAdd(dst, v * p.scale); else *dst += v * p.scale;
        } else if (do_bias && hi_ == 0) {                        // lane (ho, hi = 0, i) carries sum_p gz[p][4*ho + i]
            float* dst = p.db + 4 * ho_ + j;
            if (p.atomic) atomicAdd(dst, v); else *dst += v;
        }
    }
}

template <int CO, int CI, int BPX, bool FIX>
int launch_wgrad_thin_kernel(const WgP& p, int chunks, size_t smem, hipStream_t s)
{
    auto kern = conv_wgrad_thin_kernel<CO, CI, BPX, FIX>;
    if (int rc = set_smem(kern, smem)) return rc;
    hipLaunchKernelGGL(kern, dim3(chunks), dim3(256), smem, s, p);
    return (int)hipGetLastError();
}

template <int BPX, bool FIX>
int launch_wgrad_thin_shape(const WgP& p, int chunks, size_t smem, hipStream_t s)
{
    if (p.Cout == 8 && p.Cin == 8) return launch_wgrad_thin_kernel<8, 8, BPX, FIX>(p, chunks, smem, s);
    if (p.Cout == 16 && p.Cin == 8) return launch_wgrad_thin_kernel<16, 8, BPX, FIX>(p, chunks, smem, s);
    if (p.Cout == 8 && p.Cin == 16) return launch_wgrad_thin_kernel<8, 16, BPX, FIX>(p, chunks, smem, s);
    if (p.Cout == 32 && p.Cin == 16) return launch_wgrad_thin_kernel<32, 16, BPX, FIX>(p, chunks, smem, s);
    if (p.Cout == 16 && p.Cin == 32) return launch_wgrad_thin_kernel<16, 32, BPX, FIX>(p, chunks, smem, s);
    return PG_E_UNSUP;
}

template <int BPX>
int launch_wgrad_thin(WgP& p, hipStream_t s)
{
    if (g_tune[PG_TUNE_WGRAD] != PG_WGRAD_TILE_NOT_STRIP) {      // row-streaming kernel (conv_strip.hip) where the shape allows
        const int rc = launch_wgrad_strip(p, s);
        if (rc != PG_E_UNSUP) return rc;
    }
    TileGeom g;
    if (!set_geom(p, g, BPX, 3, halo_max(3, BPX))) return PG_E_UNSUP;
    if ((long long)g.TN * p.Hout * p.Wout * (p.Cout > p.Cin ? p.Cout : p.Cin) * 4 >= (1ll << 31)) return PG_E_UNSUP;     // 32-bit buffer offsets
    const int sz = p.Cout == 16 ? 16 : p.Cout + 16, sx = p.Cin == 16 ? 16 : p.Cin + 16;      // PixStride<C>
    size_t smem = ((size_t)BPX * sz + (size_t)g.halo * sx) * sizeof(float);
    const int nb = (p.Cout / 4) * (p.Cin / 4);
    const size_t red = (size_t)4 * (nb <= 16 ? 1 : nb / 16) * 37 * (nb <= 16 ? 4 * nb : 64) * sizeof(float);   // [wave][NE][NL]
    if (red > smem) smem = red;
    int chunks = 1024; if (chunks > g.ntiles) chunks = g.ntiles;
    p.tiles_per_block = (g.ntiles + chunks - 1) / chunks;
    chunks = (g.ntiles + p.tiles_per_block - 1) / p.tiles_per_block;
    p.atomic = chunks > 1 ? 1 : 0;
    snprintf(g_last_kernel, sizeof(g_last_kernel), "conv_wgrad_thin_kernel<%d, %d, %d>", p.Cout, p.Cin, BPX);
#ifdef PG_WINO_TRACE
    p.trace = g_wgrad_trace;
#endif
    const bool fix = BPX == 64 && g.lgTW == 4 && g.lgTH == 2 && g.TN == 1;
    return fix ? launch_wgrad_thin_shape<BPX, BPX == 64>(p, chunks, smem, s) : launch_wgrad_thin_shape<BPX, false>(p, chunks, smem, s);
}

template <int KS>
int dispatch_wgrad(WgP& p, hipStream_t s)
{
    if constexpr (KS == 4) {
        return launch_wgrad<KS, 1, 1, 2, 2, 16>(p, s);                                        // 32x32 block, 16-px tiles
    } else {
        const long long M = (long long)p.N * p.Hout * p.Wout;
        if (M <= 32) return launch_wgrad<KS, 1, 1, 2, 2, 16>(p, s);
        if constexpr (KS == 3) {
            // measured (tools/sweeps/sweep_wgrad_thin.py): block-MFMA wins on 32 -> 16 always, on 16 -> 32 below ~1.5 M pixels
            if ((p.Cout == 16 && p.Cin == 32) || (p.Cout == 32 && p.Cin == 16 && M < 1500000))
                return launch_wgrad_thin<64>(p, s);
        }
        if (p.Cout <= 16 && p.Cin <= 16) {
            if constexpr (KS == 3) {
                // 8-channel sides: the 16x16x4 tile would be 50-75 % padding -> 4x4x1 block MFMA kernel
                if ((p.Cout == 8 || p.Cin == 8) && (p.Cout == 8 || p.Cout == 16) && (p.Cin == 8 || p.Cin == 16))
                    return launch_wgrad_thin<64>(p, s);
            }
            return launch_wgrad<KS, 1, 1, 1, 1, 128>(p, s);     // 16x16 block
        }
        if constexpr (KS == 3) {
            switch (g_tune[PG_TUNE_WGRAD]) {                                                   // tuning sweep only
                case PG_WGRAD_32x16_128PX: return launch_wgrad<KS, 2, 1, 1, 1, 128>(p, s);
                case PG_WGRAD_64x16_64PX: return launch_wgrad<KS, 2, 1, 2, 1, 64>(p, s);
                default: break;
            }
        }
        if constexpr (KS == 3) {
            // measured (tools/sweeps/sweep_wgrad.py): with >= ~4e8 MACs per tap the 64-cout block (two K-waves) wins on
            // >= 64 input channels and 128-pixel tiles win on the narrow layers; small launches keep 32x16 / 64 px
            const double macs = (double)M * p.Cout * p.Cin;
            if (g_tune[PG_TUNE_WGRAD] < 0 && macs >= 4e8) {
                if (p.Cin >= 64) return launch_wgrad<KS, 2, 1, 2, 1, 64>(p, s);
                return launch_wgrad<KS, 2, 1, 1, 1, 128>(p, s);
            }
        }
        return launch_wgrad<KS, 2, 1, 1, 1, 64>(p, s);     // 32(cout) x 16(cin) block, 4 waves split the pixels
    }
}

}  // namespace

extern "C" int pg_conv2d_wgrad_nhwc(const float* x, const float* gz, float* dw, float* db,
                                    int N, int Hin, int Win, int Cin, int Cout, int KS, int pad, int ups,
                                    float scale, pg_stream_t stream)
{
    if (!x || !gz || !dw || N <= 0 || Hin <= 0 || Win <= 0 || Cin <= 0 || Cout <= 0) return PG_E_ARG;
    if ((Cin & 3) || (Cout & 3)) return PG_E_ALIGN;
    WgP p;
    p.x = x; p.gz = gz; p.dw = dw; p.db = db;
    p.N = N; p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.Cout = Cout; p.pad = pad; p.ups = ups;
    p.Hout = Hin + 2 * pad - KS + 1; p.Wout = Win + 2 * pad - KS + 1;
    if (p.Hout <= 0 || p.Wout <= 0 || !is_pow2(p.Hout) || !is_pow2(p.Wout)) return PG_E_UNSUP;
    if (ups && ((Hin | Win) & 1)) return PG_E_ARG;
    p.scale = scale;
    hipStream_t s = (hipStream_t)stream;
    if (k4_layer(p, KS)) return launch_k4_wgrad(p, s);
    switch (KS) {
        case 1: return dispatch_wgrad<1>(p, s);
        case 3: return dispatch_wgrad<3>(p, s);
        case 4: return dispatch_wgrad<4>(p, s);
        default: return PG_E_UNSUP;
    }
}

// Weight gradient of a DBlock's c2 layer with the pool adjoint evaluated in the gz gather (see pg_conv2d_unpooled_nhwc, conv_api.hip)
extern "C" int pg_conv2d_wgrad_unpooled_nhwc(const float* x, const float* g, const unsigned char* gbytes, float gmul, float gslope,
                                             float* dw, float* db, int N, int Hin, int Win, int Cin, int Cout,
                                             float scale, pg_stream_t stream)
{
    if (!x || !g || !gbytes || !dw || N <= 0 || Hin <= 0 || Win <= 0) return PG_E_ARG;
    if ((Hin | Win) & 1) return PG_E_ARG;
    if (!((Cout == 16 && Cin == 8) || (Cout == 8 && Cin == 8) || (Cout == 8 && Cin == 16)) || !is_pow2(Hin) || !is_pow2(Win) || Hin < 8 || Win < 8)
        return PG_E_UNSUP;
    WgP p;
    p.x = x; p.gz = g; p.dw = dw; p.db = db;
    p.N = N; p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.Cout = Cout; p.pad = 1; p.ups = 0;
    p.Hout = Hin; p.Wout = Win;
    p.scale = scale;
    p.gbytes = gbytes; p.gmul = gmul; p.gslope = gslope;
    return launch_wgrad_thin<64>(p, (hipStream_t)stream);
}

#ifdef PG_WINO_TRACE
extern "C" int pg_debug_wgrad_trace(void* buf) { g_wgrad_trace = (unsigned long long*)buf; return 0; }
#endif
