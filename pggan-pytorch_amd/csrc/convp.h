// Launch parameter blocks of the conv / weight-gradient kernels, shared by conv_igemm.hip (tile kernels) and conv_strip.hip
// (row-streaming kernels of the 8/16-channel 1024^2 layers).  Host + device, plain data.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

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

// Row-streaming kernels (conv_strip.hip).  PG_E_UNSUP = "not this shape": the caller keeps its tile kernel.  ``name`` receives the
// kernel symbol for pg_debug_last_conv_kernel.
int launch_conv_strip(ConvP& p, hipStream_t s, char* name, size_t name_len);
int launch_wgrad_strip(WgP& p, hipStream_t s, char* name, size_t name_len);
int launch_conv_strip_pn_torgb(const float* x, const float* w, const float* bias, float* y, float* r,
                               const float* t_w, const float* t_b, float t_scale, float* img,
                               int N, int C, int H, int W, int Cin, int Cout, float scale, float slope, float eps,
                               hipStream_t s, char* name, size_t name_len);
int launch_conv_strip_masked_rgb_bwd(const float* gz, const float* wt, const unsigned char* mask_bytes, float mask_slope, float* y,
                                     const float* rgb_w, float rgb_scale, float* gimg,
                                     const float* img, float* rgb_dw, float* rgb_db,
                                     int N, int C, int H, int W, int Cin, int Cout, float scale,
                                     hipStream_t s, char* name, size_t name_len);
int launch_conv_strip_fromrgb(const float* img, const float* rgb_w, const float* rgb_b, float rgb_scale, float rgb_slope,
                              unsigned char* x_signs, const float* w, const float* bias, float* y, unsigned char* y_signs,
                              int N, int C, int H, int W, int Cmid, int Cout, float scale, float slope,
                              hipStream_t s, char* name, size_t name_len);

}  // namespace pgk
