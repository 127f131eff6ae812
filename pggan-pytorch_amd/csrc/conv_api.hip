// The direct convolution's requests and C entry points (forward, backward-data and gradient-penalty tangent forms).
//
// Owns: conv_request / conv2d_impl (which kernel family serves a request, what it fuses, what falls back to a second pass) and
// the forward entry points of include/pggan_hip.h on top of them, the three RGB-fused strip forwards included; the weight
// packing of the backward-data convs (pack_dgrad_kernel, pack_dgrad_batched_kernel and their entry points); the launch record
// and tuning switches (pg_debug_last_conv_kernel, pg_debug_set_tuning).  The kernels are in conv_igemm.hip, conv_thin.hip,
// conv_k4.hip and conv_strip.hip; the weight-gradient entry points in conv_wgrad.hip.
#include "convp.h"

__thread char pgk::g_last_kernel[96] = "";
__thread int pgk::g_tune[4] = {-1, -1, -1, -1};

namespace {

using namespace pgk;

// One 32 x 32 (cout x cin) tile of one tap, transposed through LDS:  wt[KS-1-kh][KS-1-kw][ci][co] = w[kh][kw][co][ci]
__device__ __forceinline__ void pack_dgrad_tile(const float* __restrict__ w, float* __restrict__ wt, int KS, int Cout, int Cin,
                                                int tap, int ci_b, int co_b)
{
    __shared__ float tile[32][33];
    const int kh = tap / KS, kw = tap % KS;
    const int otap = (KS - 1 - kh) * KS + (KS - 1 - kw);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int co = co_b + r, ci = ci_b + tx;
        tile[r][tx] = (co < Cout && ci < Cin) ? w[((size_t)tap * Cout + co) * Cin + ci] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int ci = ci_b + r, co = co_b + tx;
        if (ci < Cin && co < Cout) wt[((size_t)otap * Cin + ci) * Cout + co] = tile[tx][r];
    }
}

__global__ void pack_dgrad_kernel(const float* __restrict__ w, float* __restrict__ wt, int KS, int Cout, int Cin)
{
    pack_dgrad_tile(w, wt, KS, Cout, Cin, blockIdx.z, blockIdx.x * 32, blockIdx.y * 32);
}

// All layers of a network in ONE launch (the weights live in one flat buffer, the packed copies in its mirror).
constexpr int PACK_MAX_LAYERS = 32;
struct PackDesc {
    int n;
    int first_block[PACK_MAX_LAYERS + 1];          // prefix sum of the per-layer block counts
    long long off[PACK_MAX_LAYERS];                // element offset of the layer in both flat buffers
    int ks[PACK_MAX_LAYERS], cout[PACK_MAX_LAYERS], cin[PACK_MAX_LAYERS];
};

__global__ void pack_dgrad_batched_kernel(const float* __restrict__ wbase, float* __restrict__ wtbase, PackDesc d)
{
    int l = 0;
    while (l + 1 < d.n && (int)blockIdx.x >= d.first_block[l + 1]) ++l;
    const int Cout = d.cout[l], Cin = d.cin[l];
    int b = blockIdx.x - d.first_block[l];
    const int nbx = (Cin + 31) / 32, nby = (Cout + 31) / 32;
    const int bx = b % nbx; b /= nbx;
    const int by = b % nby; const int tap = b / nby;
    pack_dgrad_tile(wbase + d.off[l], wtbase + d.off[l], d.ks[l], Cout, Cin, tap, bx * 32, by * 32);
}

}  // namespace

// Whatever the launch of a request could not fuse into its epilogue runs as a second pass over y (``pooled``: the launch pooled)
static int second_pass(const ConvP& want, bool pooled, pg_stream_t stream)
{
    const int64_t P = (int64_t)want.N * want.Hout * want.Wout;
    if (want.ypool && !pooled)
        return pg_avgpool2_fwd(want.y, want.pool_other, want.ypool, want.N, want.Hout >> 1, want.Wout >> 1, want.Cout, want.pool_a, want.pool_b, stream);
    if (want.yup) return pg_avgpool2_bwd(want.y, want.upmask, want.yup, want.N, want.Hout, want.Wout, want.Cout, want.up_mul, want.mask_slope, stream);
    if (want.pn_r) return pg_pixelnorm_fwd(want.y, want.y, want.pn_r, P, want.Cout, want.pn_eps, stream);
    if (want.pnb_y) return pg_pixelnorm_lrelu_bwd(want.y, want.pnb_y, want.pnb_r, want.y, P, want.Cout, want.mask_slope, stream);
    return 0;
}

// 3x3 pad-1 layers on maps of whole 32 x 8 pixel tiles, for the block-MFMA kernels of the 8/16-cout layers (dispatch_thin);
// ``channels``: the caller's condition on the channel counts
static bool thin_shape(const ConvP& p, bool channels)
{
    return channels && p.KS == 3 && p.pad == 1 && (p.Wout & 31) == 0 && (p.Hout & 7) == 0 && g_tune[PG_TUNE_PATH] != PG_PATH_NO_THIN;
}

// The fields every conv entry point takes; the optional outputs are set by the entry point that has them
static ConvP conv_request(const float* x, const float* w, const float* bias, const float* mask, float* y,
                          int N, int Hin, int Win, int Cin, int Cout, int KS, int pad, float scale, float slope, float mask_slope)
{
    ConvP p;
    p.x = x; p.w = w; p.bias = bias; p.mask = mask; p.y = y;
    p.N = N; p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.Cout = Cout; p.KS = KS; p.pad = pad;
    p.scale = scale; p.slope = slope; p.mask_slope = mask_slope;
    return p;
}

// ``p``: the request of an entry point (every optional output it wants is set); ``flags``: PG_FLAG_*
static int conv2d_impl(ConvP& p, int flags, pg_stream_t stream)
{
    if (!p.x || !p.w || !p.y || p.N <= 0 || p.Hin <= 0 || p.Win <= 0 || p.Cin <= 0 || p.Cout <= 0) return PG_E_ARG;
    if ((p.Cin & 3) || (p.Cout & 3)) return PG_E_ALIGN;
    const int KS = p.KS, Cin = p.Cin, Cout = p.Cout;
    p.ups = flags & PG_FLAG_UPSAMPLE;
    p.mask_bytes = (flags & PG_FLAG_MASK_BYTES) ? 1 : 0; p.y_bytes = (flags & PG_FLAG_Y_BYTES) ? 1 : 0;
    if (flags & PG_FLAG_SIGNS_OUT) {                        // forward mode: the (otherwise unused) mask argument is the byte output
        if (!p.mask || p.mask_bytes) return PG_E_ARG;
        p.ysigns = reinterpret_cast<unsigned char*>(const_cast<float*>(p.mask));
        p.mask = nullptr;
    }
    p.Hout = p.Hin + 2 * p.pad - KS + 1; p.Wout = p.Win + 2 * p.pad - KS + 1;
    if (p.Hout <= 0 || p.Wout <= 0 || !is_pow2(p.Hout) || !is_pow2(p.Wout)) return PG_E_UNSUP;
    if (p.ups && ((p.Hin | p.Win) & 1)) return PG_E_ARG;
    if (p.ypool && ((p.Hout | p.Wout) & 1)) return PG_E_ARG;
    // 32-bit element offsets inside the kernels
    if ((long long)p.N * p.Hin * p.Win * Cin >= (1ll << 31) || (long long)p.N * p.Hout * p.Wout * Cout >= (1ll << 31) ||
        (long long)KS * KS * Cout * Cin >= (1ll << 31)) return PG_E_UNSUP;
    // ``want`` keeps the request; in p an optional output is set only while the launch at hand fuses it.  The pool is fused by every
    // 3x3 launch that does not split K, the others by the launches below that name them.  With one of those others set (or sign
    // bytes) dispatch_conv_tile is the generic tile kernel in one pass or PG_E_UNSUP: neither split-K form has these epilogues.
    const ConvP want = p;
    if (KS != 3) p.ypool = nullptr;
    p.yup = nullptr; p.pn_r = nullptr; p.pnb_y = nullptr;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (p.mask_bytes || p.y_bytes || p.ysigns) {
        // sign-byte activations exist in the epilogues of the generic tile kernel (no split-K, no second pass) and of the
        // 8-cout block-MFMA kernel only: PG_E_UNSUP tells the caller to redo the layer with fp32 masks
        if (KS != 3 || (p.y_bytes && !p.ypool) || want.pn_r || want.pnb_y) return PG_E_UNSUP;
        p.yup = want.yup;
        const bool thin_plain = !p.y_bytes && !p.yup && !p.ypool && ((Cout == 8 && (Cin == 8 || Cin == 16)) || (Cout == 16 && Cin == 8 && p.mask));
        // 8->16 + pool (forward: sign bytes out; tangent: masked): +8..14 % over the generic tile kernel (tools/sweeps/bench_thin16pool.py)
        const bool thin_pool = g_tune[PG_TUNE_PATH] != PG_PATH_NO_THIN_POOL16 && !p.yup && p.ypool && Cout == 16 && Cin == 8;
        return thin_shape(p, thin_plain || thin_pool) ? dispatch_thin(p, s) : dispatch_conv_tile(p, s);
    }
    const bool thin_pn = thin_shape(p, Cout == 8 && (Cin == 8 || Cin == 16));
    if (want.pnb_y && want.pnb_r && KS == 3 && Cout <= 32) {             // fused PixelNorm adjoint: thin kernel (8 couts) or one-row generic tiles
        p.pnb_y = want.pnb_y;
        rc = thin_pn ? dispatch_thin(p, s) : dispatch_conv_tile(p, s);
        if (rc != PG_E_UNSUP) return rc;
        p.pnb_y = nullptr;
    }
    if (want.pn_r && KS == 3 && Cout <= 32 && !p.mask && g_tune[PG_TUNE_PATH] != PG_PATH_UNFUSED_PIXELNORM) {   // fused PixelNorm, likewise
        p.pn_r = want.pn_r;
        rc = thin_pn ? dispatch_thin(p, s) : dispatch_conv_tile(p, s);
        if (rc != PG_E_UNSUP) return rc;
        p.pn_r = nullptr;
    }
    if (want.yup && KS == 3) {             // the unpool epilogue exists in the generic tile kernel only (no split-K): everything else unpools in a second pass
        p.yup = want.yup;
        rc = dispatch_conv_tile(p, s);
        if (rc != PG_E_UNSUP) return rc;
        p.yup = nullptr;
    }
    // measured (tools/sweeps/sweep_thin8.py): 1.5-1.7x on 8 couts; on 16 couts only the masked 8->16 launch gains (the
    // 16x16x4 tile has no padding there), 32 input channels lose -> those stay on the generic kernel
    if (thin_shape(p, (Cout == 8 && (Cin == 8 || Cin == 16)) || (Cout == 16 && Cin == 8 && p.mask && !want.ypool)))
        rc = dispatch_thin(p, s);                       // pools in its own epilogue when p.ypool is set
    else if (k4_layer(p, KS))
        rc = launch_k4_conv(p, s);
    else
        rc = dispatch_conv_tile(p, s);
    if (rc) return rc;
    return second_pass(want, p.ypool && p.ksplit == 1, stream);      // (split-K launches defer their epilogue: no pool)
}

extern "C" int pg_conv2d_nhwc(const float* x, const float* w, const float* bias, const float* mask, float* y,
                              int N, int Hin, int Win, int Cin, int Cout, int KS, int pad, int ups,
                              float scale, float slope, float mask_slope, pg_stream_t stream)
{
    ConvP p = conv_request(x, w, bias, mask, y, N, Hin, Win, Cin, Cout, KS, pad, scale, slope, mask_slope);
    return conv2d_impl(p, ups, stream);
}

extern "C" int pg_conv2d_pixelnorm_nhwc(const float* x, const float* w, const float* bias, float* y, float* r,
                                        int N, int Hin, int Win, int Cin, int Cout, int KS, int pad, int ups,
                                        float scale, float slope, float eps, pg_stream_t stream)
{
    if (!r) return PG_E_ARG;
    ConvP p = conv_request(x, w, bias, nullptr, y, N, Hin, Win, Cin, Cout, KS, pad, scale, slope, 0.2f);
    p.pn_r = r; p.pn_eps = eps;
    return conv2d_impl(p, ups, stream);
}

extern "C" int pg_conv2d_pnbwd_nhwc(const float* x, const float* w, const float* ysaved, const float* r, float* y,
                                    int N, int Hin, int Win, int Cin, int Cout, int KS, int pad,
                                    float scale, float slope, pg_stream_t stream)
{
    if (!ysaved) return PG_E_ARG;
    ConvP p = conv_request(x, w, nullptr, nullptr, y, N, Hin, Win, Cin, Cout, KS, pad, scale, 1.0f, slope);
    p.pnb_y = ysaved; p.pnb_r = r;
    return conv2d_impl(p, 0, stream);
}

extern "C" int pg_conv2d_unpool_nhwc(const float* x, const float* w, const float* upmask, float* y, float* yup,
                                     int N, int Hin, int Win, int Cin, int Cout, int KS, int pad, int flags,
                                     float scale, float up_mul, float mask_slope, pg_stream_t stream)
{
    if (!yup) return PG_E_ARG;
    ConvP p = conv_request(x, w, nullptr, nullptr, y, N, Hin, Win, Cin, Cout, KS, pad, scale, 1.0f, mask_slope);
    p.yup = yup; p.upmask = upmask; p.up_mul = up_mul;
    return conv2d_impl(p, flags & PG_FLAG_MASK_BYTES, stream);
}

extern "C" int pg_conv2d_pool_nhwc(const float* x, const float* w, const float* bias, const float* mask, float* y,
                                   float* ypool, const float* pool_other, float pool_a, float pool_b, int pool_only,
                                   int N, int Hin, int Win, int Cin, int Cout, int KS, int pad, int ups,
                                   float scale, float slope, float mask_slope, pg_stream_t stream)
{
    if (!ypool) return PG_E_ARG;
    ConvP p = conv_request(x, w, bias, mask, y, N, Hin, Win, Cin, Cout, KS, pad, scale, slope, mask_slope);
    p.ypool = ypool; p.pool_other = pool_other; p.pool_a = pool_a; p.pool_b = pool_b; p.pool_only = pool_only;
    return conv2d_impl(p, ups, stream);
}

// Backward-data conv / weight gradient of a DBlock's c2 layer whose incoming gradient is the POOL ADJOINT of the coarser
// block's gradient g: instead of materialising gz2 = gmul * upsample2(g) * lrelu'(a2) (16 channels at 1024^2: the largest
// tensor of the backward sweep, written once and read twice), both consumers evaluate it in their input gathers from g
// (a quarter of the pixels) and the sign bytes of a2.  Block-MFMA kernels of the 8/16-channel layers only (PG_E_UNSUP otherwise).
extern "C" int pg_conv2d_unpooled_nhwc(const float* g, const float* w, const unsigned char* gbytes, float gmul, float gslope,
                                       const float* mask, float* y, int N, int Hin, int Win, int Cin, int Cout, int flags,
                                       float scale, float mask_slope, pg_stream_t stream)
{
    if (!g || !w || !gbytes || !y || N <= 0 || Hin <= 0 || Win <= 0) return PG_E_ARG;
    if ((Hin | Win) & 1) return PG_E_ARG;
    if (!(Cout == 8 && (Cin == 8 || Cin == 16)) || (Win & 31) || (Hin & 7) || !is_pow2(Hin) || !is_pow2(Win)) return PG_E_UNSUP;
    if ((long long)N * Hin * Win * Cin >= (1ll << 31)) return PG_E_UNSUP;
    ConvP p = conv_request(g, w, nullptr, mask, y, N, Hin, Win, Cin, Cout, 3, 1, scale, 1.f, mask_slope);
    p.ups = 1; p.Hout = Hin; p.Wout = Win;
    p.mask_bytes = (flags & PG_FLAG_MASK_BYTES) ? 1 : 0;
    p.gbytes = gbytes; p.gmul = gmul; p.gslope = gslope;
    return dispatch_thin(p, (hipStream_t)stream);
}

// A DBlock's first conv with the block's fromRGB layer evaluated in its input gather (reference network.py:145 in front of :33-36):
//   x0 = lrelu(rgb_scale * conv1x1(img, rgb_w) + rgb_b)  (never written; its sign bytes -> x_signs),  y = lrelu(scale * conv3x3(x0, w) + bias)
// for forward passes whose fromRGB output is not needed in fp32 afterwards (no weight gradient of this conv follows: the G step's pass
// through D).  The 8 -> 8 layer of the 1024^2 stage (row-streaming kernel); PG_E_UNSUP otherwise.
extern "C" int pg_conv2d_fromrgb_nhwc(const float* img, const float* rgb_w, const float* rgb_b, float rgb_scale, float rgb_slope,
                                      unsigned char* x_signs, const float* w, const float* bias, float* y, unsigned char* y_signs,
                                      int N, int C, int H, int W, int Cmid, int Cout, float scale, float slope, pg_stream_t stream)
{
    if (!img || !rgb_w || !w || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Cmid <= 0 || Cout <= 0) return PG_E_ARG;
    return pgk::launch_conv_strip_fromrgb(img, rgb_w, rgb_b, rgb_scale, rgb_slope, x_signs, w, bias, y, y_signs, N, C, H, W, Cmid, Cout,
                                          scale, slope, (hipStream_t)stream);
}

// The generator's last conv (+ bias + LeakyReLU + PixelNorm, network.py:33-41) with the block's toRGB layer (network.py:49, :138 at
// alpha = 1) in the same epilogue: the normalised activation is written for the backward pass as before and the image
//   img[n][c][h][w] = t_scale * sum_co t_w[c][co] * y[n][h][w][co] + t_b[c]
// leaves with it, instead of a second launch that reads y back.  8 -> 8 on strip-sized maps (the 1024^2 stage); PG_E_UNSUP otherwise.
extern "C" int pg_conv2d_pixelnorm_torgb_nhwc(const float* x, const float* w, const float* bias, float* y, float* r,
                                              const float* t_w, const float* t_b, float t_scale, float* img,
                                              int N, int C, int H, int W, int Cin, int Cout, float scale, float slope, float eps,
                                              pg_stream_t stream)
{
    if (!x || !w || !y || !r || !t_w || !img || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return PG_E_ARG;
    return pgk::launch_conv_strip_pn_torgb(x, w, bias, y, r, t_w, t_b, t_scale, img, N, C, H, W, Cin, Cout, scale, slope, eps,
                                           (hipStream_t)stream);
}

// The entry block's backward-data conv (adjoint of c1, x LeakyReLU' of fromRGB's output from its sign bytes) with fromRGB's own
// backward-data (the adjoint of the 1x1 conv of network.py:145) in the same epilogue: the gradient with respect to the IMAGE leaves
// with -- or, y == NULL, instead of -- the 8-channel gradient gf, which only fromRGB's weight gradient reads afterwards.
// Also (img, rgb_dw[, rgb_db] given): fromRGB's WEIGHT gradient accumulated in the same epilogue (one commit per workgroup) -- in the batched
// adjoint sweep nobody else reads the 8-channel gradient, so it is not written at all there (y == NULL).
extern "C" int pg_conv2d_masked_fromrgb_bwd_nhwc(const float* gz, const float* wt, const unsigned char* mask_bytes, float mask_slope, float* y,
                                                 const float* rgb_w, float rgb_scale, float* gimg,
                                                 const float* img, float* rgb_dw, float* rgb_db,
                                                 int N, int C, int H, int W, int Cin, int Cout, float scale, pg_stream_t stream)
{
    if (!gz || !wt || !mask_bytes || N <= 0 || C <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return PG_E_ARG;
    if ((!gimg && !rgb_dw) || (gimg && !rgb_w) || (rgb_dw && !img) || (rgb_db && !rgb_dw)) return PG_E_ARG;
    return pgk::launch_conv_strip_masked_rgb_bwd(gz, wt, mask_bytes, mask_slope, y, rgb_w, rgb_scale, gimg, img, rgb_dw, rgb_db,
                                                 N, C, H, W, Cin, Cout, scale, (hipStream_t)stream);
}

extern "C" const char* pg_debug_last_conv_kernel(void) { return g_last_kernel; }

extern "C" int pg_debug_set_tuning(int key, int value)
{
    if (key < 0 || key >= 4) return PG_E_ARG;
    g_tune[key] = value;                                    // (values nothing interprets select nothing: see the enums)
    return 0;
}

extern "C" int pg_pack_dgrad_weights_batched(const float* wbase, float* wtbase, int nlayers, const int64_t* off,
                                             const int* ks, const int* cout, const int* cin, pg_stream_t stream)
{
    if (!wbase || !wtbase || nlayers <= 0 || !off || !ks || !cout || !cin) return PG_E_ARG;
    for (int l0 = 0; l0 < nlayers; l0 += PACK_MAX_LAYERS) {
        PackDesc d;
        d.n = nlayers - l0 < PACK_MAX_LAYERS ? nlayers - l0 : PACK_MAX_LAYERS;
        int total = 0;
        for (int l = 0; l < d.n; ++l) {
            const int i = l0 + l;
            if (ks[i] <= 0 || cout[i] <= 0 || cin[i] <= 0 || off[i] < 0) return PG_E_ARG;
            d.first_block[l] = total;
            d.off[l] = off[i]; d.ks[l] = ks[i]; d.cout[l] = cout[i]; d.cin[l] = cin[i];
            total += ((cin[i] + 31) / 32) * ((cout[i] + 31) / 32) * ks[i] * ks[i];
        }
        d.first_block[d.n] = total;
        hipLaunchKernelGGL(pack_dgrad_batched_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, wbase, wtbase, d);
    }
    return (int)hipGetLastError();
}

extern "C" int pg_pack_dgrad_weights(const float* w, float* wt, int KS, int Cout, int Cin, pg_stream_t stream)
{
    if (!w || !wt || KS <= 0 || Cout <= 0 || Cin <= 0) return PG_E_ARG;
    dim3 grid((Cin + 31) / 32, (Cout + 31) / 32, KS * KS);
    hipLaunchKernelGGL(pack_dgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, w, wt, KS, Cout, Cin);
    return (int)hipGetLastError();
}
