// Differentiable augmentation of D's inputs (include/pggan_hip_augment.h): per image an x-flip, an integer shift with zero padding, a
// cutout rectangle and a gain on chosen channels, as ONE gather -- and its exact transpose, which is the same gather with the shift
// negated and the cutout tested on the other side.  Plus the kernel that makes the parameter table from uniform draws and the sign
// count the adaptive controller reads.
//
// Load form.  A thread owns four consecutive output columns (one 16-byte store).  Their four source pixels are consecutive too, but
// start at any column: rather than one misaligned 16-byte load or four 4-byte loads, the thread loads the one or two ALIGNED 16-byte
// words of the source row that hold them and picks four of the eight dwords -- which four is the same for a whole image, a scalar branch
// (csrc/real_batch.hip does the same for bytes with v_alignbyte).  W is a multiple of 4 and planes are 16-byte aligned, so an aligned word lies wholly inside a row or wholly
// outside it: a word outside stands as zeros, which is exactly the zero padding (its load is redirected to a word inside the plane and
// discarded) -- nothing outside the source plane is read, for any table entry.  Lanes of a wave read consecutive words (descending under a flip), each word at most twice.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip.h"
#include "pggan_hip_augment.h"

// the gain is ONE fp32 add and the table arithmetic is a product followed by its floor: nothing may be fused, for the whole translation unit
#pragma clang fp contract(off)

namespace {

inline int grid_for(long long total, int block = 256, int cap = 4096)
{
    long long g = (total + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (int)g;
}

// log2 of a power of two in 4 .. PG_AUGMENT_MAX_SIZE, -1 otherwise
inline int log2_size(int v)
{
    if (v < 4 || v > PG_AUGMENT_MAX_SIZE || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// A table row with its entries clamped to what can matter (a shift beyond the image empties it like a shift by its size; a cutout edge beyond the
// image is the image's edge), so that everything behind fits 32 bits for any int32 in the table.  Uniform over a workgroup: a workgroup works on
// ONE plane, the row is read through the scalar cache and every test on it is a scalar test.
struct Row {
    int flip, gain_on, dy, dx, y0, y1, x0, x1;
    float gain;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ Row load_row(const int* __restrict__ table, int n, int H, int W)
{
    const int* t = table + PG_AUGMENT_COLS * (long long)n;
    Row r;
    r.flip = t[0] & PG_AUGMENT_FLIP;
    r.gain_on = t[0] & PG_AUGMENT_GAIN;
    r.dy = clampi(t[1], -H, H);
    r.dx = clampi(t[2], -W, W);
    r.y0 = clampi(t[3], 0, H); r.y1 = clampi(t[4], 0, H);
    r.x0 = clampi(t[5], 0, W); r.x1 = clampi(t[6], 0, W);
    r.gain = __int_as_float(t[7]);
    return r;
}

// ADJOINT == false: out = apply(x);  true: out (gx) = adjoint(x (gy)).  blockIdx.y walks the planes n * C + c, blockIdx.x the plane's H * W / 4
// pieces of four columns; both loop when the grid is capped.
template <bool ADJOINT>
__global__ __launch_bounds__(256) void augment_kernel(const uint32_t* __restrict__ x, const int* __restrict__ table,
                                                      uint32_t* __restrict__ out, int planes, int C, int lh, int lw, unsigned channel_mask)
{
    const int H = 1 << lh, W = 1 << lw, lq = lw - 2, work = 1 << (lh + lq);
    for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
        const int n = (int)((unsigned)pl / (unsigned)C), c = pl - n * C;
        const Row r = load_row(table, n, H, W);
        const bool gain_on = !ADJOINT && r.gain_on && ((channel_mask >> c) & 1u);
        const bool no_cut = r.y0 >= r.y1 || r.x0 >= r.x1;
        // output column j + k reads source column c0 + k, or c0 + 3 - k under a flip, c0 = base - j (flip) or base + j: its two low bits, the
        // position of the four sources in their aligned words, are the same for the whole image (j is a multiple of 4)
        const int base = r.flip ? W - 4 - r.dx : (ADJOINT ? r.dx : -r.dx);
        const int s = base & 3;
        const uint32_t* xp = x + ((long long)pl << (lh + lw));
        uint32_t* op = out + ((long long)pl << (lh + lw));
        for (int u = blockIdx.x * blockDim.x + threadIdx.x; u < work; u += gridDim.x * blockDim.x) {
            const int j = 4 * (u & ((1 << lq) - 1)), i = u >> lq;
            const int rr = ADJOINT ? i + r.dy : i - r.dy;                       // source row
            const int c0 = r.flip ? base - j : base + j;                        // lowest source column of the four
            const bool row_in = rr >= 0 && rr < H;
            const int w0 = c0 & ~3;                                             // column of the aligned word that holds c0 (floor, also below 0)
            // (named registers, no local array: an array indexed by ``s`` is moved to LDS by the compiler, with a wait behind every load)
            // both words are loaded from addresses clamped INTO the plane and zeroed afterwards where they lie outside it: no load sits in a
            // divergent branch, so the two are in flight together
            const bool lo_in = row_in && w0 >= 0 && w0 < W, hi_in = row_in && w0 + 4 >= 0 && w0 + 4 < W;
            const uint32_t* row = xp + (clampi(rr, 0, H - 1) << lw);
            // (the empty asm keeps every dword of a word live, so that each word stays ONE 16-byte load: left alone, the compiler narrows the
            //  loads to the dwords a case of the switch below uses -- 8-byte loads at 4-byte offsets)
            uint4 lo = *reinterpret_cast<const uint4*>(row + clampi(w0, 0, W - 4));
            uint4 hi = make_uint4(0u, 0u, 0u, 0u);
            if (s) {                                                            // (a scalar branch: s is the image's)
                hi = *reinterpret_cast<const uint4*>(row + clampi(w0 + 4, 0, W - 4));
                asm volatile("" : "+v"(lo.x), "+v"(lo.y), "+v"(lo.z), "+v"(lo.w), "+v"(hi.x), "+v"(hi.y), "+v"(hi.z), "+v"(hi.w));
            } else {
                asm volatile("" : "+v"(lo.x), "+v"(lo.y), "+v"(lo.z), "+v"(lo.w));
            }
            if (!lo_in) lo = make_uint4(0u, 0u, 0u, 0u);
            if (!hi_in) hi = make_uint4(0u, 0u, 0u, 0u);
            uint32_t v0, v1, v2, v3;                                            // source columns c0 .. c0 + 3 (zeros outside the row)
            switch (s) {                                                        // (a scalar branch)
            case 0: v0 = lo.x; v1 = lo.y; v2 = lo.z; v3 = lo.w; break;
            case 1: v0 = lo.y; v1 = lo.z; v2 = lo.w; v3 = hi.x; break;
            case 2: v0 = lo.z; v1 = lo.w; v2 = hi.x; v3 = hi.y; break;
            default: v0 = lo.w; v1 = hi.x; v2 = hi.y; v3 = hi.z; break;
            }
            uint32_t o0 = r.flip ? v3 : v0, o1 = r.flip ? v2 : v1, o2 = r.flip ? v1 : v2, o3 = r.flip ? v0 : v3;
            const int step = r.flip ? -1 : 1, first = r.flip ? c0 + 3 : c0;     // output column j + k reads source column first + k step
            if (gain_on) {                                                      // the gain goes to source pixels only: not to the padding
                const auto add = [&](uint32_t& o, int col) {
                    if (row_in && col >= 0 && col < W) o = __float_as_uint(__uint_as_float(o) + r.gain);
                };
                add(o0, first); add(o1, first + step); add(o2, first + 2 * step); add(o3, first + 3 * step);
            }
            if (!no_cut) {
                // the cutout lives in the coordinates of the augmented image: the output pixel here, the source pixel in the adjoint
                const int ci = ADJOINT ? rr : i;
                if (ci >= r.y0 && ci < r.y1) {
                    const auto cut = [&](uint32_t& o, int cj) {
                        if (cj >= r.x0 && cj < r.x1) o = 0u;
                    };
                    if (ADJOINT) { cut(o0, first); cut(o1, first + step); cut(o2, first + 2 * step); cut(o3, first + 3 * step); }
                    else { cut(o0, j); cut(o1, j + 1); cut(o2, j + 2); cut(o3, j + 3); }
                }
            }
            *reinterpret_cast<uint4*>(op + (i << lw) + j) = make_uint4(o0, o1, o2, o3);
        }
    }
}

int launch_augment(bool adjoint, const float* x, const int* table, float* out, int64_t N, int C, int H, int W, int channel_mask,
                   pg_stream_t stream)
{
    if (!x || !table || !out || N < 1 || C < 1 || C > 32 || H < 1 || W < 1) return PG_E_ARG;
    const int lh = log2_size(H), lw = log2_size(W);
    if (lh < 0 || lw < 0) return PG_E_UNSUP;
    if (N > (int64_t)1 << 24) return PG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(table)) & 15) return PG_E_ALIGN;
    const long long count = (long long)N * C * H * W;
    if (reinterpret_cast<uintptr_t>(x) < reinterpret_cast<uintptr_t>(out + count) && reinterpret_cast<uintptr_t>(out) < reinterpret_cast<uintptr_t>(x + count))
        return PG_E_ARG;                                                      // a gather cannot run in place
    const int planes = (int)(N * C), work = (H * W) >> 2;                     // (N <= 2^24, C <= 32: below 2^31)
    const int block = work >= 256 ? 256 : work < 64 ? 64 : work;              // (work is a power of two)
    const dim3 grid(grid_for(work, block, 512), planes < 65535 ? planes : 65535);
    const uint32_t* xs = reinterpret_cast<const uint32_t*>(x);
    uint32_t* os = reinterpret_cast<uint32_t*>(out);
    if (adjoint)
        hipLaunchKernelGGL(augment_kernel<true>, grid, dim3(block), 0, (hipStream_t)stream, xs, table, os, planes, C, lh, lw, 0u);
    else
        hipLaunchKernelGGL(augment_kernel<false>, grid, dim3(block), 0, (hipStream_t)stream, xs, table, os, planes, C, lh, lw,
                           (unsigned)channel_mask);
    return (int)hipGetLastError();
}

struct Policy {
    int H, W, flip;
    float ry, rx, ch, cw, gain, p;
};

// one axis of the cutout: `len` masked pixels around the centre `centre` of an axis of `size`, clipped; the whole axis when len >= size
__device__ __forceinline__ void cut_axis(int centre, int len, int size, int& lo, int& hi)
{
    if (len >= size) { lo = 0; hi = size; return; }
    lo = max(centre - len / 2, 0);
    hi = min(centre - len / 2 + len, size);
}

__global__ __launch_bounds__(256) void augment_table_kernel(const float* __restrict__ U, int* __restrict__ table, long long rows, Policy q)
{
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const float4 ua = reinterpret_cast<const float4*>(U)[2 * row], ub = reinterpret_cast<const float4*>(U)[2 * row + 1];
    const float u0 = ua.x, u1 = ua.y, u2 = ua.z, u3 = ua.w, u4 = ub.x, u5 = ub.y, u6 = ub.z, u7 = ub.w;
    const float fH = (float)q.H, fW = (float)q.W;
    int flags = 0, dy = 0, dx = 0, y0 = 0, y1 = 0, x0 = 0, x1 = 0;
    float b = 0.f;
    if (q.flip && u0 < q.p && u1 < 0.5f) flags |= PG_AUGMENT_FLIP;
    if (u2 < q.p) {
        const int my = (int)floorf(q.ry * fH), mx = (int)floorf(q.rx * fW);
        dy = min((int)floorf(u3 * (float)(2 * my + 1)), 2 * my) - my;           // (the product may round up to 2 my + 1: clamped)
        dx = min((int)floorf(u4 * (float)(2 * mx + 1)), 2 * mx) - mx;
    }
    if (u5 < q.p) {
        const int hc = (int)floorf(q.ch * fH + 0.5f), wc = (int)floorf(q.cw * fW + 0.5f);
        if (hc > 0 && wc > 0) {
            const float t = u6 * 4096.f, f = floorf(t);
            const int cy = (int)floorf((f * (1.f / 4096.f)) * fH), cx = (int)floorf((t - f) * fW);
            cut_axis(cy, hc, q.H, y0, y1);
            cut_axis(cx, wc, q.W, x0, x1);
        }
    }
    if (q.gain > 0.f && u7 < q.p) {
        flags |= PG_AUGMENT_GAIN;
        const float t = 2.f * u1, ug = t - floorf(t);
        b = (2.f * ug - 1.f) * q.gain;
    }
    int4* o = reinterpret_cast<int4*>(table) + 2 * row;
    o[0] = make_int4(flags, dy, dx, y0);
    o[1] = make_int4(y1, x0, x1, (int)__float_as_uint(b));
}

// one workgroup: integer partial sums per thread (strided), an LDS tree in a fixed order, thread 0 adds to the accumulator
__global__ __launch_bounds__(256) void score_signs_kernel(const float* __restrict__ s, int n, double* __restrict__ acc)
{
    __shared__ int part[256];
    int sum = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = s[i];
        sum += (v > 0.f) - (v < 0.f);
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        acc[0] = acc[0] + (double)part[0];
        acc[1] = acc[1] + (double)n;
    }
}

inline bool unit(float v) { return v >= 0.f && v <= 1.f; }                     // (false for a NaN)

}  // namespace

extern "C" int pg_augment_apply(const float* x, const int* table, float* out, int64_t N, int C, int H, int W, int channel_mask,
                                pg_stream_t stream)
{
    return launch_augment(false, x, table, out, N, C, H, W, channel_mask, stream);
}

extern "C" int pg_augment_adjoint(const float* gy, const int* table, float* gx, int64_t N, int C, int H, int W, pg_stream_t stream)
{
    return launch_augment(true, gy, table, gx, N, C, H, W, 0, stream);
}

extern "C" int pg_augment_table(const float* U, int64_t rows, int H, int W, float ry, float rx, float ch, float cw, float gain, int flip,
                                float p, int* table, pg_stream_t stream)
{
    if (!U || !table || rows < 1 || rows > (int64_t)1 << 24 || H < 1 || W < 1 || !unit(ry) || !unit(rx) || !unit(ch) || !unit(cw) || !unit(p)
        || !(gain >= 0.f)) return PG_E_ARG;
    if (log2_size(H) < 0 || log2_size(W) < 0) return PG_E_UNSUP;
    if ((reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(table)) & 15) return PG_E_ALIGN;
    const Policy q = {H, W, flip != 0, ry, rx, ch, cw, gain, p};
    hipLaunchKernelGGL(augment_table_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, U, table,
                       (long long)rows, q);
    return (int)hipGetLastError();
}

extern "C" int pg_score_signs(const float* s, int64_t n, double* acc, pg_stream_t stream)
{
    if (!s || !acc || n < 1 || n > PG_AUGMENT_MAX_SCORES) return PG_E_ARG;
    if (reinterpret_cast<uintptr_t>(acc) & 7) return PG_E_ALIGN;
    hipLaunchKernelGGL(score_signs_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, s, (int)n, acc);
    return (int)hipGetLastError();
}
