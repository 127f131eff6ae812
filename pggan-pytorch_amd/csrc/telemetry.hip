// Statistics of the training process itself, taken where the numbers already are:
//   pg_scalar_stats_push     : up to 8 small fp32 device tensors (the four losses of an iteration) -> their means, folded into a running
//                              record on the device.  One launch of one workgroup per iteration, no host synchronisation; the host
//                              reads the record once per tick.
//   pg_segment_stats_plan    : host only.  Cuts S segments (offset, length) of a flat buffer into chunks of PG_SEG_CHUNK floats.
//   pg_segment_stats_f32     : one workgroup per chunk -> one partial {sum, sumsq, maxabs, n_nonfinite} of its finite elements.
//   pg_segment_stats_finish  : one wave per segment adds its partials in ascending chunk order.
// The reference has neither (its loss monitors read every loss on the host every iteration); the definition is this project's own,
// restated for the CPU in tests/telemetry_ref.py.
//
// Everything is fp64 and every order of summation is fixed: the same inputs give the same bits, and a segment's numbers depend on
// nothing but its own elements (a chunk never spans two segments).  No atomics anywhere (the library is built with
// -munsafe-fp-atomics).  Contraction is off for the whole file, so that what is written is what is evaluated; x * x of an fp32 x is
// exact in fp64 (48 significant bits), a fused form would give the same sums.
//
// Memory bound by design: the segment pass reads each float once with 16-byte loads (8 per thread and chunk, all of them independent),
// the fp64 work per element is one convert, two adds, one multiply and a compare.  Non-finite elements are replaced by 0.0 on their
// way into the sums (adding +0.0 changes no finite sum: a partial sum here is never -0.0) and counted.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "pggan_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int SLOTS = PG_STATS_MAX_SOURCES;
constexpr int REC = PG_STATS_RECORD;            // doubles per slot
constexpr int CHUNK = PG_SEG_CHUNK;
static_assert(SLOTS == 8 && REC == 8, "the record layout below is 8 slots of 8 doubles");
static_assert(CHUNK % 1024 == 0, "a chunk is whole passes of 256 threads x 4 floats");

struct Sources {
    const float* p[SLOTS];
    int n[SLOTS];
};

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool finite_bits64(double x)
{
    return ((unsigned)(__double_as_longlong(x) >> 32) & 0x7ff00000u) != 0x7ff00000u;
}

// Wave w of the four takes slots w and w + 4.  The value of a source is its mean: lane l adds elements l, l + 64, l + 128, ... in that
// order from 0.0, the lanes combine by shuffles with offsets 32, 16, 8, 4, 2, 1 (lane i takes lane i + offset), lane 0 divides by n.
// Lane 0 then folds the value into the slot's record {n_finite, sum, sumsq, min, max, last, n_nonfinite, first_bad}.
__global__ __launch_bounds__(256) void scalar_stats_push_kernel(double* __restrict__ record, Sources src, int K, int reset)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = wave; k < K; k += 4) {
        double* r = record + k * REC;
        const float* p = src.p[k];
        double acc = 0.0;
        if (p) {
            const int n = src.n[k];
            for (int i = lane; i < n; i += 64) acc += (double)p[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
            acc = acc / (double)n;
        }
        if (lane != 0) continue;
        double nf = 0.0, sum = 0.0, sumsq = 0.0, lo = INFINITY, hi = -INFINITY, last = NAN, bad = 0.0, first = -1.0;
        if (!reset) { nf = r[0]; sum = r[1]; sumsq = r[2]; lo = r[3]; hi = r[4]; last = r[5]; bad = r[6]; first = r[7]; }
        if (p) {
            if (finite_bits64(acc)) {
                nf += 1.0;
                sum += acc;
                sumsq += acc * acc;
                lo = acc < lo ? acc : lo;
                hi = acc > hi ? acc : hi;
            } else {
                if (first < 0.0) first = nf + bad;       // the index of this push among the slot's pushes since the reset
                bad += 1.0;
            }
            last = acc;
        }
        if (p || reset) { r[0] = nf; r[1] = sum; r[2] = sumsq; r[3] = lo; r[4] = hi; r[5] = last; r[6] = bad; r[7] = first; }
    }
}

struct Part { double s, q; float m; int bad; };

__device__ __forceinline__ void take(Part& a, float x)
{
    const bool ok = finite_bits(x);
    const double d = ok ? (double)x : 0.0;
    a.s += d;
    a.q += d * d;
    a.m = fmaxf(a.m, ok ? fabsf(x) : 0.f);
    a.bad += ok ? 0 : 1;
}

// One workgroup per chunk (offset, length <= CHUNK).  Thread t takes the 16-byte groups t, t + 256, ... of the chunk in that order, each
// component of a group into an accumulator of its own; the four combine as (c0 + c1) + (c2 + c3).  The up to three elements behind the
// last whole group go to threads 0, 1, 2, one each, added after that.  Then the lanes of a wave by shuffles (offsets 32 ... 1), then the
// four waves as (w0 + w1) + (w2 + w3).  A chunk whose offset is not a multiple of 4 elements (pg_segment_stats_plan never makes one) or
// that does not lie inside [0, n_flat) is not an out-of-bounds access: the first is read element by element, the second is clipped.
__global__ __launch_bounds__(256) void segment_stats_kernel(const float* __restrict__ flat, long long n_flat,
                                                            const long long* __restrict__ chunks, double* __restrict__ partials)
{
    __shared__ double red[4][4];
    const int tid = threadIdx.x;
    const long long c = blockIdx.x;
    long long off = chunks[2 * c], len = chunks[2 * c + 1];
    if (off < 0) off = 0;
    if (off > n_flat) off = n_flat;
    if (len > n_flat - off) len = n_flat - off;
    if (len > CHUNK) len = CHUNK;
    if (len < 0) len = 0;
    const float* p = flat + off;
    Part a[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j].s = 0.0; a[j].q = 0.0; a[j].m = 0.f; a[j].bad = 0; }
    const int n = (int)len;
    const bool vec = (off & 3) == 0;
    const int nvec = vec ? n >> 2 : 0;
    const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll 4
    for (int g = tid; g < nvec; g += 256) {
        const float4 v = p4[g];
        take(a[0], v.x);
        take(a[1], v.y);
        take(a[2], v.z);
        take(a[3], v.w);
    }
    Part t;
    t.s = (a[0].s + a[1].s) + (a[2].s + a[3].s);
    t.q = (a[0].q + a[1].q) + (a[2].q + a[3].q);
    t.m = fmaxf(fmaxf(a[0].m, a[1].m), fmaxf(a[2].m, a[3].m));
    t.bad = (a[0].bad + a[1].bad) + (a[2].bad + a[3].bad);
    if (vec) {
        if (4 * nvec + tid < n) take(t, p[4 * nvec + tid]);          // the ragged tail: at most three scalar loads in the workgroup
    } else {
        for (int i = tid; i < n; i += 256) take(t, p[i]);
    }
    double s = t.s, q = t.q, m = (double)t.m, b = (double)t.bad;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_down(s, o, 64);
        q += __shfl_down(q, o, 64);
        m = fmax(m, __shfl_down(m, o, 64));
        b += __shfl_down(b, o, 64);
    }
    if ((tid & 63) == 0) { red[tid >> 6][0] = s; red[tid >> 6][1] = q; red[tid >> 6][2] = m; red[tid >> 6][3] = b; }
    __syncthreads();
    if (tid < 4) {
        const double r = tid == 2 ? fmax(fmax(red[0][2], red[1][2]), fmax(red[2][2], red[3][2]))
                                  : (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        partials[4 * c + tid] = r;
    }
}

// One wave per segment.  The partials of the segment's chunks are staged in LDS 64 at a time (one coalesced load per lane); lane j < 4
// then folds component j over them from the first chunk to the last: sum, sumsq and n_nonfinite by addition from 0.0, maxabs by maximum.
__global__ __launch_bounds__(64) void segment_stats_finish_kernel(const double* __restrict__ partials, const long long* __restrict__ ranges,
                                                                  long long nchunks, double* __restrict__ out)
{
    __shared__ double sh[4][64];
    const int lane = threadIdx.x;
    const long long seg = blockIdx.x;
    long long first = ranges[2 * seg], count = ranges[2 * seg + 1];
    if (first < 0) first = 0;
    if (first > nchunks) first = nchunks;
    if (count > nchunks - first) count = nchunks - first;
    double acc = 0.0;
    for (long long base = 0; base < count; base += 64) {
        const int m = (int)(count - base < 64 ? count - base : 64);
        if (lane < m) {
            const double* q = partials + 4 * (first + base + lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) sh[j][lane] = q[j];
        }
        __syncthreads();
        if (lane < 4) {
            if (lane == 2) for (int i = 0; i < m; ++i) acc = fmax(acc, sh[2][i]);
            else for (int i = 0; i < m; ++i) acc += sh[lane][i];
        }
        __syncthreads();
    }
    if (lane < 4) out[4 * seg + lane] = acc;
}

}  // namespace

extern "C" int pg_scalar_stats_push(double* record, const float* const* sources, const int* lengths, int K, int reset, pg_stream_t stream)
{
    if (!record || K < 1 || K > SLOTS || (!sources && !reset)) return PG_E_ARG;
    if (((uintptr_t)record) & 7) return PG_E_ALIGN;
    Sources src;
    bool any = reset != 0;
    for (int k = 0; k < SLOTS; ++k) {
        src.p[k] = (sources && k < K) ? sources[k] : nullptr;
        src.n[k] = 0;
        if (src.p[k]) {
            if (!lengths || lengths[k] < 1 || lengths[k] > PG_STATS_MAX_LENGTH) return PG_E_ARG;
            if (((uintptr_t)src.p[k]) & 3) return PG_E_ALIGN;
            src.n[k] = lengths[k];
            any = true;
        }
    }
    if (!any) return 0;                                       // every slot skipped and no reset: nothing to launch
    hipLaunchKernelGGL(scalar_stats_push_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, record, src, K, reset ? 1 : 0);
    return (int)hipGetLastError();
}

extern "C" int pg_segment_stats_plan(const int64_t* offsets, const int64_t* lengths, int S, int64_t n_flat, int64_t* chunks,
                                     int64_t capacity, int64_t* ranges, int64_t* nchunks)
{
    if (!offsets || !lengths || !nchunks || S < 1 || n_flat < 1 || (chunks && !ranges)) return PG_E_ARG;
    int64_t total = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t off = offsets[s], len = lengths[s];
        if (len < 1 || off < 0 || off > n_flat || len > n_flat - off) return PG_E_ARG;
        if (off & 3) return PG_E_ALIGN;
        const int64_t cnt = (len + CHUNK - 1) / CHUNK;
        if (chunks) {
            if (total + cnt > capacity) return PG_E_ARG;
            for (int64_t i = 0; i < cnt; ++i) {
                chunks[2 * (total + i)] = off + i * CHUNK;
                chunks[2 * (total + i) + 1] = len - i * CHUNK < CHUNK ? len - i * CHUNK : CHUNK;
            }
            ranges[2 * s] = total;
            ranges[2 * s + 1] = cnt;
        }
        total += cnt;
    }
    if (total > 0x7fffffffLL) return PG_E_UNSUP;
    *nchunks = total;
    return 0;
}

extern "C" int pg_segment_stats_f32(const float* flat, int64_t n_flat, const int64_t* chunks, int64_t nchunks, double* partials,
                                    pg_stream_t stream)
{
    if (!flat || !chunks || !partials || n_flat < 1 || nchunks < 1 || nchunks > 0x7fffffffLL) return PG_E_ARG;
    if ((((uintptr_t)flat) & 15) || (((uintptr_t)chunks) & 7) || (((uintptr_t)partials) & 7)) return PG_E_ALIGN;
    hipLaunchKernelGGL(segment_stats_kernel, dim3((unsigned)nchunks), dim3(256), 0, (hipStream_t)stream, flat, (long long)n_flat,
                       (const long long*)chunks, partials);
    return (int)hipGetLastError();
}

extern "C" int pg_segment_stats_finish(const double* partials, int64_t nchunks, const int64_t* ranges, int S, double* out,
                                       pg_stream_t stream)
{
    if (!partials || !ranges || !out || nchunks < 1 || S < 1) return PG_E_ARG;
    if ((((uintptr_t)partials) & 7) || (((uintptr_t)ranges) & 7) || (((uintptr_t)out) & 7)) return PG_E_ALIGN;
    hipLaunchKernelGGL(segment_stats_finish_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, partials,
                       (const long long*)ranges, (long long)nchunks, out);
    return (int)hipGetLastError();
}
