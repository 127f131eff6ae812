// What the direct-conv translation units share.  Plain data and inline helpers, host + device:
//   * the launch parameter blocks ConvP / WgP (also read by the Winograd units) and the per-stream Workspace;
//   * the MFMA / LDS idioms of the tile kernels (f32x4, MFMA16, lds_load, RowStride, PixStride, halo_max);
//   * the host plumbing every tile launcher repeats: tile geometry (make_geom / set_geom), the split-K rule, set_smem;
//   * the launch record and tuning switches (g_last_kernel, g_tune: defined in conv_api.hip) and the launchers that cross units.
// Units: conv_igemm.hip (tile forward kernels), conv_wgrad.hip (weight gradients), conv_k4.hip (4x4 boundary layers),
// conv_thin.hip (8/16-cout block-MFMA forward), conv_strip.hip (row-streaming kernels), conv_api.hip (requests and entry points).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include <type_traits>
#include "pggan_hip.h"
#include "pggan_hip_debug.h"
#include "bufload.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

namespace pgk {

inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }      // ceil(log2 v)
inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// Kernel arguments: field order and types are what the compiled kernels read.  The initialisers are "every optional feature off",
// so that an entry point sets what it uses and a new field needs no edit elsewhere.
struct ConvP {
    const float* x = nullptr; const float* w = nullptr; const float* bias = nullptr; const float* mask = nullptr; float* y = nullptr;
    int N = 0, Hin = 0, Win = 0, Cin = 0, Cout = 0, Hout = 0, Wout = 0, KS = 0, pad = 0, ups = 0;
    float scale = 1.f, slope = 1.f, mask_slope = 1.f;
    int lgTW = 0, lgTH = 0, TN = 0, tilesW = 0, tilesH = 0;      // tile geometry: filled by the launcher
    unsigned mWT = 0, mHT = 0;  // floor(2^32/WT)+1, floor(2^32/HT)+1: exact n/d for n < 2^16 via __umulhi
    int ksplit = 1;             // >1: blockIdx.z owns a slice of the Cin chunks, partial sums are
                                // committed with fp32 atomics into a pre-zeroed y (epilogue deferred)
    // fused 2x2 average pool of the activated output (pg_conv2d_pool_nhwc): ypool = pool_a * avgpool2(y) + pool_b * pool_other
    float* ypool = nullptr; const float* pool_other = nullptr; float pool_a = 1.f, pool_b = 0.f; int pool_only = 0;
    // fused adjoint of that pool (pg_conv2d_unpool_nhwc): yup[n][2h+dy][2w+dx][c] = 0.25*up_mul * y[n][h][w][c] * lrelu'(upmask[...])
    float* yup = nullptr; const float* upmask = nullptr; float up_mul = 1.f;
    // fused PixelNorm of the activated output (pg_conv2d_pixelnorm_nhwc): y *= rsqrt(mean_c y^2 + pn_eps), pn_r[pixel] = that factor
    float* pn_r = nullptr; float pn_eps = 0.f;
    // fused adjoint of (LeakyReLU -> PixelNorm) applied to the conv result g (pg_conv2d_pnbwd_nhwc):
    //   y = r[pix] * (g - pnb_y * mean_c(g * pnb_y)) * lrelu'(pnb_y)
    const float* pnb_y = nullptr; const float* pnb_r = nullptr;
    // sign-byte activations (PG_FLAG_MASK_BYTES / PG_FLAG_Y_BYTES): one byte per float4, bit j = (channel 4q+j > 0)
    int mask_bytes = 0, y_bytes = 0;
    unsigned char* ysigns = nullptr;   // PG_FLAG_SIGNS_OUT: the sign bytes of y are written here IN ADDITION to y (forward mode)
    // pool adjoint fused into the input gather (pg_conv2d_unpooled_nhwc): xin[n][h][w][c] = gmul * x[n][h/2][w/2][c] * lrelu'(gbytes[n][h][w][c])
    const unsigned char* gbytes = nullptr; float gmul = 1.f, gslope = 1.f;
};
static_assert(sizeof(ConvP) == 248 && std::is_trivially_copyable_v<ConvP>, "ConvP is a kernel argument: its layout is part of the compiled kernels");

// LeakyReLU' factors of four channels from a sign byte / the sign byte of four activated outputs
__device__ __forceinline__ float4 pg_sign_factors(unsigned char b, float slope)
{
    return make_float4((b & 1) ? 1.f : slope, (b & 2) ? 1.f : slope, (b & 4) ? 1.f : slope, (b & 8) ? 1.f : slope);
}
__device__ __forceinline__ unsigned char pg_sign_byte(float4 o)
{
    return (unsigned char)((o.x > 0.f ? 1 : 0) | (o.y > 0.f ? 2 : 0) | (o.z > 0.f ? 4 : 0) | (o.w > 0.f ? 8 : 0));
}

struct WgP {
    const float* x = nullptr; const float* gz = nullptr; float* dw = nullptr; float* db = nullptr;
    int N = 0, Hin = 0, Win = 0, Cin = 0, Cout = 0, Hout = 0, Wout = 0, pad = 0, ups = 0;
    float scale = 1.f;
    int lgTW = 0, lgTH = 0, TN = 0, tilesW = 0, tilesH = 0, ntiles = 0, tiles_per_block = 0;    // filled by the launcher
    unsigned mWT = 0, mHT = 0;  // magic reciprocals of the halo tile width / height (see ConvP)
    int atomic = 0;             // 0: this workgroup is the only writer of its dW block -> plain +=
    // pool adjoint fused into the gz gather (pg_conv2d_wgrad_unpooled_nhwc): gz[n][h][w][c] = gmul * g[n][h/2][w/2][c] * lrelu'(gbytes[n][h][w][c])
    const unsigned char* gbytes = nullptr; float gmul = 1.f, gslope = 1.f;
#ifdef PG_WINO_TRACE
    unsigned long long* trace = nullptr;   // [workgroup][wave][tile < 8][8] s_memtime stamps (tools/exp/wgrad_trace.py)
#endif
};
#ifndef PG_WINO_TRACE
static_assert(sizeof(WgP) == 128, "WgP is a kernel argument: its layout is part of the compiled kernels");
#endif
static_assert(std::is_trivially_copyable_v<WgP>, "WgP is a kernel argument");

// Scratch registered for a stream by pg_set_workspace (conv_wino.hip): [WS_TICKETS zero-initialised, self-resetting tickets][partial sums].
// Launches on one stream are ordered, so every kernel that slices a reduction across workgroups may use the whole of it.
struct Workspace { int device; hipStream_t stream; char* ptr; size_t bytes; };
constexpr size_t WS_TICKETS = 4096, WS_HEAD = WS_TICKETS * sizeof(unsigned);
bool find_workspace(hipStream_t s, Workspace& out);

template <int VEC> __device__ __forceinline__ void lds_load(const float* p, float (&o)[VEC]);
template <> __device__ __forceinline__ void lds_load<4>(const float* p, float (&o)[4]) {
    float4 v = *reinterpret_cast<const float4*>(p); o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
template <> __device__ __forceinline__ void lds_load<2>(const float* p, float (&o)[2]) {
    float2 v = *reinterpret_cast<const float2*>(p); o[0] = v.x; o[1] = v.y;
}
template <> __device__ __forceinline__ void lds_load<1>(const float* p, float (&o)[1]) { o[0] = *p; }

// LDS row stride (floats) of a KC-channel row: conflict-free for the gfx950 lane groups
//   VEC=4 (ds_read_b128, 4x16 lanes, 64 banks): 24   VEC=2 (ds_read_b64): 12   VEC=1: 8
template <int VEC> struct RowStride { static constexpr int value = VEC == 4 ? 24 : (VEC == 2 ? 12 : 8); };

// row stride == 16 (mod 32): the two 32-lane groups of ds_read_b32 hit disjoint banks
template <int B> struct PixStride { static constexpr int value = (B % 32 == 16) ? B : B + 16; };

// Upper bound of the halo pixels of one tile (sizes the register prefetch): KS=3 with TH,TW >= 4 needs at most
// 2.25*BPX; tiles of >= 512 pixels are always 32 wide (make_geom), so (BPX/32+2)*34 is exact there.
constexpr int halo_max(int KS, int BPX)
{
    return KS == 1 ? BPX : (KS == 4 ? 16 * BPX : (BPX >= 512 ? (BPX / 32 + 2) * 34 : (BPX * 9) / 4));
}

// the two 4x4 boundary layers with their own kernels (conv_k4.hip): 1x1 -> 4x4 (pad 3) and 4x4 -> 1x1 (pad 0), whole 16-channel blocks
template <typename P>
inline bool k4_layer(const P& p, int KS)
{
    return KS == 4 && !p.ups && (p.Cin & 15) == 0 && (p.Cout & 15) == 0 &&
           ((p.pad == 3 && p.Hin == 1 && p.Win == 1) || (p.pad == 0 && p.Hin == 4 && p.Win == 4));
}

// Pixel tile of the tile kernels: TN images x TH x TW output pixels (powers of two, BPX in all) and its (KS-1)-halo HT x WT
struct TileGeom { int lgTW, lgTH, TN, tilesW, tilesH, ntiles, HT, WT, halo; };

inline TileGeom make_geom(int N, int Hout, int Wout, int BPX, int KS, int max_tw = 32)
{
    TileGeom g;
    int TW = Wout < max_tw ? Wout : max_tw; if (TW > BPX) TW = BPX;
    while (TW > 4 && BPX / TW < 4 && Hout >= 4) TW >>= 1;      // keep tiles at least 4 rows tall (halo <= 2.25x)
    int TH = BPX / TW; if (TH > Hout) TH = Hout;
    g.lgTW = ilog2(TW); g.lgTH = ilog2(TH);
    g.TN = BPX / (TW * TH);
    g.tilesW = Wout / TW; g.tilesH = Hout / TH;
    g.ntiles = ((N + g.TN - 1) / g.TN) * g.tilesH * g.tilesW;
    g.HT = TH + KS - 1; g.WT = TW + KS - 1;
    g.halo = g.TN * g.HT * g.WT;
    return g;
}

// The geometry step of every tile launcher: the tile of make_geom into the parameter block (ConvP / WgP) with the magic reciprocals
// of its halo extents.  false: the halo exceeds ``halo_budget``, the register prefetch the kernel was compiled with.
template <typename P>
inline bool set_geom(P& p, TileGeom& g, int BPX, int KS, int halo_budget, int max_tw = 32)
{
    g = make_geom(p.N, p.Hout, p.Wout, BPX, KS, max_tw);
    p.lgTW = g.lgTW; p.lgTH = g.lgTH; p.TN = g.TN; p.tilesW = g.tilesW; p.tilesH = g.tilesH;
    if constexpr (std::is_same_v<P, WgP>) p.ntiles = g.ntiles;
    auto magic = [](int d) { return (unsigned)((1ull << 32) / (unsigned)d) + 1u; };      // see ConvP::mWT
    p.mWT = magic(g.WT); p.mHT = magic(g.HT);
    return g.halo <= halo_budget;
}

// K slices of ``nchunks`` chunks, at most ``ks`` of them, every slice the same whole number of chunks
inline int whole_slices(int nchunks, int ks)
{
    if (ks > nchunks) ks = nchunks;
    const int cper = (nchunks + ks - 1) / ks;
    return (nchunks + cper - 1) / cper;
}

// The split-K rule of the generic tile kernel: fewer than 192 workgroups are too few for 256 CUs, so with at least 4 chunks K is
// sliced towards ~512 workgroups (memset + atomics + deferred epilogue)
inline int splitk_rule(long long blocks, int nchunks)
{
    if (blocks >= 192 || nchunks < 4) return 1;
    return whole_slices(nchunks, (int)((512 + blocks - 1) / blocks));
}

// Dynamic LDS above 48 KB needs the function attribute; it is a per-device property of the loaded code object, so it is set on
// every launch that needs it (an idempotent host-side call: no per-process flag that a second GPU or a second thread could miss).
// ``refuse_above``: sizes the launcher turns down as "not this shape" instead of letting the launch fail.
constexpr size_t SMEM_ANY = ~(size_t)0;
template <typename K>
inline int set_smem(K kern, size_t smem, size_t refuse_above = 160 * 1024)
{
    if (smem > refuse_above) return PG_E_UNSUP;
    if (smem > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

// Launch record and tuning switches of the direct-conv family (per thread; defined in conv_api.hip).  __thread: constant-initialised,
// so a use in another unit is a plain TLS access without the wrapper call a ``thread_local`` declaration implies.
extern __thread char g_last_kernel[96];     // symbol of the last conv kernel launched by this thread (pg_debug_last_conv_kernel)
extern __thread int g_tune[4];              // pg_debug_set_tuning overrides, indexed by pg_tune_key (keys and values: pggan_hip_debug.h)

// Launchers that cross units.  PG_E_UNSUP = "not this shape": the caller keeps or tries another kernel.
int dispatch_conv_tile(ConvP& p, hipStream_t s);      // conv_igemm.hip: generic tile / four-wave K-split kernels, p.KS in {1, 3, 4}
int dispatch_thin(ConvP& p, hipStream_t s);           // conv_thin.hip: row-streaming kernel where the shape allows, else conv_thin_kernel
int launch_k4_conv(ConvP& p, hipStream_t s);          // conv_k4.hip: k4_layer shapes
int launch_k4_wgrad(WgP& p, hipStream_t s);
// Row-streaming kernels (conv_strip.hip)
int launch_conv_strip(ConvP& p, hipStream_t s);
int launch_wgrad_strip(WgP& p, hipStream_t s);
int launch_conv_strip_pn_torgb(const float* x, const float* w, const float* bias, float* y, float* r,
                               const float* t_w, const float* t_b, float t_scale, float* img,
                               int N, int C, int H, int W, int Cin, int Cout, float scale, float slope, float eps, hipStream_t s);
int launch_conv_strip_masked_rgb_bwd(const float* gz, const float* wt, const unsigned char* mask_bytes, float mask_slope, float* y,
                                     const float* rgb_w, float rgb_scale, float* gimg, const float* img, float* rgb_dw, float* rgb_db,
                                     int N, int C, int H, int W, int Cin, int Cout, float scale, hipStream_t s);
int launch_conv_strip_fromrgb(const float* img, const float* rgb_w, const float* rgb_b, float rgb_scale, float rgb_slope,
                              unsigned char* x_signs, const float* w, const float* bias, float* y, unsigned char* y_signs,
                              int N, int C, int H, int W, int Cmid, int Cout, float scale, float slope, hipStream_t s);

}  // namespace pgk
