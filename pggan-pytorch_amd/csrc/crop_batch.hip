// The real-image batch of a training step cut from uint8 spectrogram STRIPS that live in HBM, in one launch:
//   pg_crop_batch_u8 : gather by (strip, start column) -> pyramid level -> mirror -> fade-in blend -> dynamic range -> fp32
// pg_real_batch_u8 (csrc/real_batch.hip) with the S x S image replaced by the window [u, u + S) of a strip [C][S][pitch]; the
// arithmetic is that file's, restated: the level in fp32, the fade and the range change in fp64 with numpy's unfused order, rounded
// once to fp32, the mirror by reading 2x2 blocks reversed.  What is new is the address: a window row starts at ANY byte of a
// 16-byte aligned strip row, so the 8 source bytes of a thread are cut out of the one or two aligned 8-byte words that hold them
// (v_alignbyte_b32).  The second word is loaded only when the window leans into it; both lie inside the row's pitch, which is a
// multiple of 16: nothing outside the strip is read, and the padding bytes a word may bring along are shifted out.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip.h"
#include "pggan_hip_crop.h"

// numpy never fuses a multiply with the following add (see io_steps.hip): for the whole translation unit
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double rounded(double v) { asm volatile("" : "+v"(v)); return v; }

struct Prep {            // dataset.py:62 / utils.py:25-29, resolved on the host
    int fade, rescale;
    double one_minus_alpha, min_in, scale, min_out;
};

// one 2x2 block {00, 01, 10, 11} of level bytes -> the four fp32 outputs (real_batch.hip's prepare_block)
__device__ __forceinline__ void prepare_block(double v[4], const Prep& p)
{
    if (p.fade) {
        const double t = (v[0] + v[1] + v[2] + v[3]) / 4.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] + rounded((t - v[i]) * p.one_minus_alpha);
    }
    if (p.rescale) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = rounded((v[i] - p.min_in) * p.scale) + p.min_out;
    }
}

// the 8 bytes at `a`, which need not be aligned: the aligned 8-byte word that holds a[0], and the next one if a[7] is in it
__device__ __forceinline__ uint2 load8_unaligned(const uint8_t* a)
{
    const unsigned s = (unsigned)(reinterpret_cast<uintptr_t>(a) & 7);
    const uint2* w = reinterpret_cast<const uint2*>(a - s);
    const uint2 lo = w[0];
    uint2 hi = make_uint2(0u, 0u);
    if (s) hi = w[1];
    const unsigned w0 = s & 4 ? lo.y : lo.x, w1 = s & 4 ? hi.x : lo.y, w2 = s & 4 ? hi.y : hi.x;
    return make_uint2(__builtin_amdgcn_alignbyte(w1, w0, s & 3), __builtin_amdgcn_alignbyte(w2, w1, s & 3));
}

// depthdiff == 0, r >= 8: a thread owns two rows x 8 output columns of one plane -- two to four aligned 8-byte loads, four 16-byte
// stores (out is [n][C][r][r] from a 16-byte aligned base: real_batch_rows_kernel's store addresses)
__global__ __launch_bounds__(256) void crop_batch_rows_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                              const int64_t* __restrict__ idx, const int64_t* __restrict__ pos,
                                                              const uint8_t* __restrict__ flip, float* __restrict__ out,
                                                              long long total, int C, int lr, int shift, Prep p)
{
    const int r = 1 << lr, lx = lr - 3, ly = lr - 1;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int xu = (int)(t & ((1 << lx) - 1));
        const int y2 = (int)((t >> lx) & ((1 << ly) - 1));
        const long long pl = t >> (lx + ly);                                 // output plane j * C + c
        const long long j = pl / C;
        const int c = (int)(pl - j * C);
        const int mirrored = flip ? flip[j] != 0 : 0;
        const int xs = mirrored ? r - 8 - 8 * xu : 8 * xu;                   // window columns [xs, xs + 8)
        const int64_t* e = table + PG_CROP_TABLE_WORDS * idx[j];
        const long long pitch = e[1];
        const uint8_t* row = src + e[0] + ((long long)c * r + 2 * y2) * pitch + (pos[j] >> shift) + xs;
        uint2 a = load8_unaligned(row);
        uint2 b = load8_unaligned(row + pitch);
        if (mirrored) {                                                      // byte k <-> byte 7 - k
            a = make_uint2(__builtin_bswap32(a.y), __builtin_bswap32(a.x));
            b = make_uint2(__builtin_bswap32(b.y), __builtin_bswap32(b.x));
        }
        float o0[8], o1[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                        // 2x2 block k: columns 2k, 2k + 1
            const unsigned wa = k < 2 ? a.x : a.y, wb = k < 2 ? b.x : b.y;
            const int sh = 16 * (k & 1);
            double v[4] = {(double)((wa >> sh) & 0xffu), (double)((wa >> (sh + 8)) & 0xffu),
                           (double)((wb >> sh) & 0xffu), (double)((wb >> (sh + 8)) & 0xffu)};
            prepare_block(v, p);
            o0[2 * k] = (float)v[0]; o0[2 * k + 1] = (float)v[1];
            o1[2 * k] = (float)v[2]; o1[2 * k + 1] = (float)v[3];
        }
        float4* d0 = reinterpret_cast<float4*>(out + (pl << (2 * lr)) + ((long long)(2 * y2) << lr) + 8 * xu);
        float4* d1 = reinterpret_cast<float4*>(reinterpret_cast<float*>(d0) + r);
        d0[0] = make_float4(o0[0], o0[1], o0[2], o0[3]); d0[1] = make_float4(o0[4], o0[5], o0[6], o0[7]);
        d1[0] = make_float4(o1[0], o1[1], o1[2], o1[3]); d1[1] = make_float4(o1[4], o1[5], o1[6], o1[7]);
    }
}

// level pixel (y, x) of a window whose rows are `pitch` bytes apart: the byte itself, or pyramid_level_u8_kernel's four samples
// with stride st = 1 << dd
__device__ __forceinline__ double level_pixel(const uint8_t* __restrict__ win, long long pitch, int dd, int y, int x, float lo, float hi)
{
    if (dd == 0) return (double)win[y * pitch + x];
    const uint8_t* q = win + ((long long)y << dd) * pitch + ((long long)x << dd);
    float v = (((float)q[0] + (float)q[1]) + (float)q[pitch]) + (float)q[pitch + 1];
    v = rintf(v * 0.25f);
    v = fminf(fmaxf(v, lo), hi);
    return (double)(uint8_t)v;
}

// r < 8 or depthdiff > 0 (a strided gather): a thread owns one 2x2 block of one output plane, byte loads, two 8-byte stores
__global__ __launch_bounds__(256) void crop_batch_blocks_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ table,
                                                                const int64_t* __restrict__ idx, const int64_t* __restrict__ pos,
                                                                const uint8_t* __restrict__ flip, float* __restrict__ out,
                                                                long long total, int C, int S, int dd, int lr, int shift,
                                                                float lo, float hi, Prep p)
{
    const int r = 1 << lr, lh = lr - 1;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
        const int x2 = (int)(t & ((1 << lh) - 1));
        const int y2 = (int)((t >> lh) & ((1 << lh) - 1));
        const long long pl = t >> (2 * lh);
        const long long j = pl / C;
        const int c = (int)(pl - j * C);
        const int mirrored = flip ? flip[j] != 0 : 0;
        const int xa = mirrored ? r - 1 - 2 * x2 : 2 * x2, xb = mirrored ? xa - 1 : xa + 1;   // level columns of output columns 2 x2, 2 x2 + 1
        const int64_t* e = table + PG_CROP_TABLE_WORDS * idx[j];
        const long long pitch = e[1];
        const uint8_t* win = src + e[0] + (long long)c * S * pitch + (pos[j] >> shift);
        double v[4] = {level_pixel(win, pitch, dd, 2 * y2, xa, lo, hi), level_pixel(win, pitch, dd, 2 * y2, xb, lo, hi),
                       level_pixel(win, pitch, dd, 2 * y2 + 1, xa, lo, hi), level_pixel(win, pitch, dd, 2 * y2 + 1, xb, lo, hi)};
        prepare_block(v, p);
        float* d = out + (pl << (2 * lr)) + ((long long)(2 * y2) << lr) + 2 * x2;             // even column, even r: 8-byte aligned
        *reinterpret_cast<float2*>(d) = make_float2((float)v[0], (float)v[1]);
        *reinterpret_cast<float2*>(d + r) = make_float2((float)v[2], (float)v[3]);
    }
}

inline int grid_for(long long total, int block = 256, int cap = 4096)
{
    long long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

extern "C" int pg_crop_batch_u8(const uint8_t* src, const int64_t* table, int64_t M, int C, int S, int shift, int depthdiff,
                                const int64_t* idx, const int64_t* pos, const uint8_t* flip, int n, float* out,
                                double alpha, double min_in, double max_in, double min_out, double max_out, pg_stream_t stream)
{
    if (!src || !table || !idx || !pos || !out || M <= 0 || n <= 0 || S <= 0 || depthdiff < 0 || depthdiff > 30 || shift < 0 || shift > 30
        || C < 1 || C > 3) return PG_E_ARG;
    if (S & (S - 1)) return PG_E_ALIGN;
    const int r = S >> depthdiff;
    if (r < 2) return PG_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15) return PG_E_ALIGN;
    int lr = 0;
    while ((1 << lr) < r) ++lr;
    Prep p;
    p.rescale = !(min_in == min_out && max_in == max_out);                   // utils.py:25 `if range_in != range_out`
    p.scale = p.rescale ? (max_out - min_out) / (max_in - min_in) : 1.0;
    p.fade = alpha < 1.0;                                                    // dataset.py:62
    p.one_minus_alpha = 1.0 - alpha;
    p.min_in = min_in;
    p.min_out = min_out;
    const long long planes = (long long)n * C;
    if (depthdiff == 0 && r >= 8) {
        const long long total = planes * (r / 2) * (r / 8);
        hipLaunchKernelGGL(crop_batch_rows_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                           src, table, idx, pos, flip, out, total, C, lr, shift, p);
    } else {
        const long long total = planes * (r / 2) * (r / 2);
        hipLaunchKernelGGL(crop_batch_blocks_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                           src, table, idx, pos, flip, out, total, C, S, depthdiff, lr, shift, (float)min_in, (float)max_in, p);
    }
    return (int)hipGetLastError();
}
