// The real-image batch of a training step in one launch, from uint8 images that live in HBM:
//   pg_real_batch_u8, pg_real_batch_2ch_u8 : gather by index from a stack [M][C][S][S]
//   pg_crop_batch_u8                       : gather by (strip, start column) from spectrogram strips [C][S][pitch]
//   -> pyramid level -> mirror -> fade-in blend -> dynamic range -> fp32
// i.e. pg_pyramid_level_u8 (dataset.py:243-250), a flip of the last axis and pg_real_prepare_u8 (dataset.py:54-67,109-113,
// utils.py:24-30) of csrc/io_steps.hip fused behind an index_select, bit for bit: the level in fp32 (sums of four bytes and
// the division by 4 are exact, rintf is np.round), the fade and the range change in fp64 with numpy's unfused order, rounded once
// to fp32.  The 2x2 block mean of the fade is exact in fp64 and the mirror maps 2x2 blocks onto 2x2 blocks, so mirror and fade
// commute bit for bit: a thread of a mirrored image reads its blocks reversed and stores them straight.
// There is one rows kernel and one blocks kernel; a SOURCE (Stack, Strips) says where a window's rows start, how far apart they are
// and how 8 of their bytes are loaded, and nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip.h"
#include "pggan_hip_phase.h"
#include "pggan_hip_crop.h"

// numpy never fuses a multiply with the following add (see io_steps.hip): for the whole translation unit
#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ double rounded(double v) { asm volatile("" : "+v"(v)); return v; }

struct Prep {            // dataset.py:62 / utils.py:25-29, resolved on the host
    int fade, rescale;
    double one_minus_alpha, min_in, scale, min_out;
};

// one 2x2 block {00, 01, 10, 11} of level bytes -> the four fp32 outputs (real_prepare_u8_kernel's arithmetic)
__device__ __forceinline__ void prepare_block(double v[4], const Prep& p)
{
    if (p.fade) {
        const double t = (v[0] + v[1] + v[2] + v[3]) / 4.0;               // reshape(...).mean((2,4)) of uint8 -> float64
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] + rounded((t - v[i]) * p.one_minus_alpha);   // dataset.py:112
    }
    if (p.rescale) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = rounded((v[i] - p.min_in) * p.scale) + p.min_out; // utils.py:29
    }
}

// Image idx[j] of a stack [M][C][S][S], S = 1 << ls.  Planes are S*S bytes, rows S bytes and the rows kernel reads columns that are
// multiples of 8 of an S >= 8: every load is 8-byte aligned from nothing more than an 8-byte aligned base.
struct Stack {
    const uint8_t* __restrict__ src;
    const int64_t* __restrict__ idx;
    int ls;
    typedef int pitch_t;
    __device__ __forceinline__ const uint8_t* row(long long j, int C, int c, int y, pitch_t& pitch) const
    {
        pitch = 1 << ls;
        return src + (((long long)idx[j] * C + c) << (2 * ls)) + ((long long)y << ls);
    }
    static __device__ __forceinline__ uint2 load8(const uint8_t* a) { return *reinterpret_cast<const uint2*>(a); }
};

// The window of columns [u, u + S), u = pos[j] >> shift, of strip idx[j] of one stored level (include/pggan_hip_crop.h), S = 1 << ls.
// A window row starts at ANY byte of a 16-byte aligned strip row, so the 8 source bytes of a thread are cut out of the one or two
// aligned 8-byte words that hold them (v_alignbyte_b32).  The second word is loaded only when the window leans into it; both lie
// inside the row's pitch, which is a multiple of 16: nothing outside the strip is read, and the padding bytes a word may bring along
// are shifted out.
struct Strips {
    const uint8_t* __restrict__ src;
    const int64_t* __restrict__ table;
    const int64_t* __restrict__ idx;
    const int64_t* __restrict__ pos;
    int ls, shift;
    typedef long long pitch_t;
    __device__ __forceinline__ const uint8_t* row(long long j, int C, int c, int y, pitch_t& pitch) const
    {
        const int64_t* e = table + PG_CROP_TABLE_WORDS * idx[j];
        pitch = e[1];
        return src + e[0] + (((long long)c << ls) + y) * pitch + (pos[j] >> shift);
    }
    // the 8 bytes at `a`, which need not be aligned: the aligned 8-byte word that holds a[0], and the next one if a[7] is in it
    static __device__ __forceinline__ uint2 load8(const uint8_t* a)
    {
        const unsigned s = (unsigned)(reinterpret_cast<uintptr_t>(a) & 7);
        const uint2* w = reinterpret_cast<const uint2*>(a - s);
        const uint2 lo = w[0];
        uint2 hi = make_uint2(0u, 0u);
        if (s) hi = w[1];
        const unsigned w0 = s & 4 ? lo.y : lo.x, w1 = s & 4 ? hi.x : lo.y, w2 = s & 4 ? hi.y : hi.x;
        return make_uint2(__builtin_amdgcn_alignbyte(w1, w0, s & 3), __builtin_amdgcn_alignbyte(w2, w1, s & 3));
    }
};

// depthdiff == 0, r >= 8: a thread owns two rows x 8 output columns of one plane -- two 8-byte loads (Strips: two to four), four
// 16-byte stores: out is [n][C][r][r] from a 16-byte aligned base and columns are multiples of 8 (32 bytes per 8 floats).
template <class Source>
__global__ __launch_bounds__(256) void real_batch_rows_kernel(Source source, const uint8_t* __restrict__ flip, float* __restrict__ out,
                                                              long long total, int C, int lr, Prep p)
{
    const int r = 1 << lr, lx = lr - 3, ly = lr - 1;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long long)gridDim.x * blockDim.x) {
        const int xu = (int)(u & ((1 << lx) - 1));
        const int y2 = (int)((u >> lx) & ((1 << ly) - 1));
        const long long pl = u >> (lx + ly);                                 // output plane j * C + c
        const long long j = pl / C;
        const int c = (int)(pl - j * C);
        const int mirrored = flip ? flip[j] != 0 : 0;
        const int xs = mirrored ? r - 8 - 8 * xu : 8 * xu;                   // source columns [xs, xs + 8)
        typename Source::pitch_t pitch;
        const uint8_t* row = source.row(j, C, c, 2 * y2, pitch) + xs;
        uint2 a = Source::load8(row);
        uint2 b = Source::load8(row + pitch);
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

// level pixel (y, x) of a window whose rows are `pitch` bytes apart: the byte itself, or pyramid_level_u8_kernel's four samples with
// stride st = 1 << dd
template <class pitch_t>
__device__ __forceinline__ double level_pixel(const uint8_t* __restrict__ win, pitch_t pitch, int dd, int y, int x, float lo, float hi)
{
    if (dd == 0) return (double)win[(long long)y * pitch + x];
    const uint8_t* q = win + ((long long)y << dd) * pitch + ((long long)x << dd);
    float v = (((float)q[0] + (float)q[1]) + (float)q[pitch]) + (float)q[pitch + 1];
    v = rintf(v * 0.25f);
    v = fminf(fmaxf(v, lo), hi);
    return (double)(uint8_t)v;
}

// r < 8 or depthdiff > 0 (a strided gather): a thread owns one 2x2 block of one output plane, byte loads, two 8-byte stores
template <class Source>
__global__ __launch_bounds__(256) void real_batch_blocks_kernel(Source source, const uint8_t* __restrict__ flip, float* __restrict__ out,
                                                                long long total, int C, int dd, int lr, float lo, float hi, Prep p)
{
    const int r = 1 << lr, lh = lr - 1;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (long long)gridDim.x * blockDim.x) {
        const int x2 = (int)(u & ((1 << lh) - 1));
        const int y2 = (int)((u >> lh) & ((1 << lh) - 1));
        const long long pl = u >> (2 * lh);
        const long long j = pl / C;
        const int c = (int)(pl - j * C);
        const int mirrored = flip ? flip[j] != 0 : 0;
        const int xa = mirrored ? r - 1 - 2 * x2 : 2 * x2, xb = mirrored ? xa - 1 : xa + 1;   // level columns of output columns 2 x2, 2 x2 + 1
        typename Source::pitch_t pitch;
        const uint8_t* win = source.row(j, C, c, 0, pitch);
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

// n windows of C planes S x S from `source` (whose `ls` is filled in here); the kernels take any C (a plane is a plane), the entry
// points state which they accept
template <class Source>
int launch_real_batch(Source source, int C, int S, int depthdiff, const uint8_t* flip, int n, float* out,
                      double alpha, double min_in, double max_in, double min_out, double max_out, pg_stream_t stream)
{
    if (S & (S - 1)) return PG_E_ALIGN;
    const int r = S >> depthdiff;
    if (r < 2) return PG_E_ALIGN;
    int lr = 0;
    while ((1 << lr) < r) ++lr;
    source.ls = lr + depthdiff;
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
        hipLaunchKernelGGL(real_batch_rows_kernel<Source>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                           source, flip, out, total, C, lr, p);
    } else {
        const long long total = planes * (r / 2) * (r / 2);
        hipLaunchKernelGGL(real_batch_blocks_kernel<Source>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream,
                           source, flip, out, total, C, depthdiff, lr, (float)min_in, (float)max_in, p);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int pg_real_batch_u8(const uint8_t* src, int64_t M, int C, int S, int depthdiff, const int64_t* idx, const uint8_t* flip,
                                int n, float* out, double alpha, double min_in, double max_in, double min_out, double max_out,
                                pg_stream_t stream)
{
    if (!src || !idx || !out || M <= 0 || n <= 0 || S <= 0 || depthdiff < 0 || depthdiff > 30 || (C != 1 && C != 3)) return PG_E_ARG;
    return launch_real_batch(Stack{src, idx, 0}, C, S, depthdiff, flip, n, out, alpha, min_in, max_in, min_out, max_out, stream);
}

// the (log-magnitude, instantaneous frequency) stacks of include/pggan_hip_phase.h
extern "C" int pg_real_batch_2ch_u8(const uint8_t* src, int64_t M, int S, int depthdiff, const int64_t* idx, const uint8_t* flip, int n,
                                    float* out, double alpha, double min_in, double max_in, double min_out, double max_out,
                                    pg_stream_t stream)
{
    if (!src || !idx || !out || M <= 0 || n <= 0 || S <= 0 || depthdiff < 0 || depthdiff > 30) return PG_E_ARG;
    return launch_real_batch(Stack{src, idx, 0}, 2, S, depthdiff, flip, n, out, alpha, min_in, max_in, min_out, max_out, stream);
}

// the strips of include/pggan_hip_crop.h
extern "C" int pg_crop_batch_u8(const uint8_t* src, const int64_t* table, int64_t M, int C, int S, int shift, int depthdiff,
                                const int64_t* idx, const int64_t* pos, const uint8_t* flip, int n, float* out,
                                double alpha, double min_in, double max_in, double min_out, double max_out, pg_stream_t stream)
{
    if (!src || !table || !idx || !pos || !out || M <= 0 || n <= 0 || S <= 0 || depthdiff < 0 || depthdiff > 30 || shift < 0 || shift > 30
        || C < 1 || C > 3) return PG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15) return PG_E_ALIGN;
    return launch_real_batch(Strips{src, table, idx, pos, 0, shift}, C, S, depthdiff, flip, n, out, alpha, min_in, max_in, min_out, max_out, stream);
}
