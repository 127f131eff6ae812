// Rate conversion in front of the sound ends (include/pggan_hip_resample.h): x [nsamp][channels] float32 or int16
// at rate_in -> the mono float32 waveform at rate_out = rate_in L / M, a polyphase filter whose table taps [L][T] is plain data from
// the host (sound.ResampleTable).  The project's own definition, restated in numpy in tests/resample_ref.py; the kernel equals
// sound.resample(device='cpu') bit for bit: fp64 products and sums without contraction in ascending tap order, one rounding to
// float32, no atomics, one writer per output.
//
// One launch, output-stationary: a workgroup owns a RUN of consecutive outputs, one per thread.
//   signal  The run's outputs read the mixed-down samples q0 - half + 1 .. q_last + half, about run M / L + T of them.  They are mixed
//           down once (the float32 bits of csrc/sound.hip) into LDS as float32 and widened at use: half the LDS of fp64, and the
//           conversion is exact.  Both edges are predication: a sample outside [0, nsamp) is never loaded, and every thread clips its
//           tap range [jlo, jhi) so that the terms outside the signal are skipped, not added as zeros.
//   table   The layout is the definition's, [r][j]: the C-ABI, the numpy twin and the kernel read one array and no second copy has
//           to be kept in step.  Consecutive outputs have phases r = (r0 + i M) mod L: a workgroup walks min(L, run) DIFFERENT rows at
//           the same j, and in [r][j] those lie T x 8 bytes apart -- 64 lanes would ask the vector cache for 64 lines per load, 16
//           bytes of each used, with more lines alive per CU (a line per lane and wave) than its 32 KiB hold.  [j][r] puts one j of
//           all phases into 8 L bytes, but the lanes' phases step by M mod L through it, and a coalesced load there needs a
//           permutation by M.  Instead the rows pass through LDS in pieces of JC taps: eight or more neighbouring lanes fetch one
//           row's piece as consecutive 16-byte loads (whole lines from L2, where the table of at most a few hundred KB lives, each
//           byte fetched once per workgroup), and every thread then reads ITS row's piece with ds_read_b64.  The piece of row u starts
//           at u x pitch doubles with an ODD pitch: 2 pitch dwords is 2 mod 4, so 32 consecutive rows fall on 32 different bank
//           pairs of the 64 -- conflict-free where threads hold consecutive rows (L > run), and where the rows are the phases
//           themselves (L < run) equal rows broadcast.  With L < run the L rows are staged once in natural order and shared: 48000 ->
//           16000 (L = 1) stages its one row whole.
//   LDS     SIG_CAP floats + TAP_CAP doubles + the row numbers = 51 KB: three workgroups (12 waves) per CU of 160 KiB.  The run is
//           THREADS outputs unless their span would pass SIG_CAP (a ratio M / L above ~4 at T = 4096, or a custom table with a
//           large M): then the host shortens it, down to one output, whose T <= 4096 samples always fit.
// 64-bit indices throughout: an hour of 48 kHz stereo is 3.5e8 input values, and n M passes 2^31 long before that.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_resample.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;                   // the longest run: one output per thread
constexpr int SIG_CAP = 5120;                  // float32 samples of the run's span (PG_RESAMPLE_MAX_TAPS + 1024)
constexpr int TAP_CAP = 15 * THREADS;          // doubles of the staged pieces: 256 rows x (14 taps + 1 of padding)

static_assert(SIG_CAP > PG_RESAMPLE_MAX_TAPS + 1, "a run of one output must fit");

__device__ __forceinline__ float sample(const float* x, long long i) { return x[i]; }
__device__ __forceinline__ float sample(const int16_t* x, long long i) { return (float)x[i] / 32768.0f; }     // exact

// dataset.py:287-288: s.sum(axis=1) / 2 in float32, in channel order (the bits of csrc/sound.hip)
template <typename S>
__device__ __forceinline__ float mixed(const S* __restrict__ x, long long k, int channels)
{
    if (channels == 1) return sample(x, k);
    float acc = 0.f;
    for (int c = 0; c < channels; ++c) acc += sample(x, k * channels + c);
    return acc / 2.0f;
}

template <typename S>
__global__ __launch_bounds__(THREADS) void resample_kernel(const S* __restrict__ x, long long nsamp, int channels,
                                                           const double* __restrict__ taps, int L, int M, int T,
                                                           float* __restrict__ out, long long n_out, int run)
{
    __shared__ float sig[SIG_CAP];
    __shared__ double piece[TAP_CAP];
    __shared__ int row_of[THREADS];
    const int tid = threadIdx.x;
    const long long n0 = (long long)blockIdx.x * run;
    const int cnt = (int)(n_out - n0 < run ? n_out - n0 : run);            // >= 1: the grid is ceil(n_out / run)
    const int half = T >> 1;
    const long long p0 = n0 * M, q0 = p0 / L;
    const long long q_last = (p0 + (long long)(cnt - 1) * M) / L;
    const long long k0 = q0 - half + 1;                                    // sig[u] is sample k0 + u
    const int span = (int)(q_last - q0) + T;                               // <= SIG_CAP - 1 by the host's choice of run

    for (int u = tid; u < span; u += THREADS) {
        const long long k = k0 + u;
        sig[u] = k >= 0 && k < nsamp ? mixed(x, k, channels) : 0.f;        // (outside: never loaded, and never used below)
    }

    // this thread's output: its sample offset, its table row and the taps that meet the signal
    int off = 0, r = 0, jlo = 0, jhi = 0;
    if (tid < cnt) {
        const long long p = p0 + (long long)tid * M, q = p / L;
        r = (int)(p - q * L);
        off = (int)(q - q0);
        jlo = q < half - 1 ? (int)(half - 1 - q) : 0;                      // k = q - half + 1 + j >= 0
        const long long room = nsamp - q + half - 1;                       // k < nsamp  <=>  j < room (q < nsamp: room >= half)
        jhi = room < T ? (int)room : T;
    }
    // the rows that pass through LDS: all L in natural order when several outputs share one, else one per output
    const bool natural = L < cnt;
    const int rows = natural ? L : cnt;
    const int slot = natural ? r : tid;
    row_of[tid] = r;
    const int pitch = (TAP_CAP / rows - 1) | 1;                            // odd, rows x pitch <= TAP_CAP
    const int jc = pitch - 1 < T ? pitch - 1 : T;                          // taps per piece: even, >= 14
    const int pairs = jc >> 1;
    int lanes = 1, shift = 0;                                              // lanes per row: the power of two that covers a piece
    while (lanes < pairs && lanes < THREADS) { lanes <<= 1; ++shift; }
    const int lx = tid & (lanes - 1), ly = tid >> shift, rows_per_pass = THREADS >> shift;
    __syncthreads();

    double acc = 0.0;
    for (int j0 = 0; j0 < T; j0 += jc) {
        for (int u = ly; u < rows; u += rows_per_pass) {
            const double* src = taps + (size_t)(natural ? u : row_of[u]) * (size_t)T + j0;
            double* dst = piece + u * pitch;
            for (int h = lx; h < pairs && j0 + 2 * h < T; h += lanes) {    // (T and j0 are even: a pair never straddles the row's end)
                const double2 v = *reinterpret_cast<const double2*>(src + 2 * h);
                dst[2 * h] = v.x;
                dst[2 * h + 1] = v.y;
            }
        }
        __syncthreads();
        const int a = jlo > j0 ? jlo : j0, b = jhi < j0 + jc ? jhi : j0 + jc;
        const double* w = piece + slot * pitch - j0;
        const float* s = sig + off;
        for (int j = a; j < b; ++j)                                        // ascending j; product, then sum (contraction is off)
            acc = acc + w[j] * (double)s[j];
        __syncthreads();
    }
    if (tid < cnt) out[n0 + tid] = (float)acc;
}

}  // namespace

extern "C" int pg_resample_mono(const void* x, int format, int64_t nsamp, int channels, const double* taps, int L, int M, int T,
                                float* out, int64_t n_out, pg_stream_t stream)
{
    if (!x || !taps || !out || nsamp < 1 || channels < 1 || L < 1 || M < 1 || T < 2 || (T & 1)) return PG_E_ARG;
    if (format != PG_RESAMPLE_F32 && format != PG_RESAMPLE_I16) return PG_E_ARG;
    const __int128 up = (__int128)nsamp * L;
    if ((__int128)n_out != (up + M - 1) / M) return PG_E_ARG;
    if (((uintptr_t)x | (uintptr_t)taps | (uintptr_t)out) & 15) return PG_E_ALIGN;
    if (L > PG_RESAMPLE_MAX_PHASES || T > PG_RESAMPLE_MAX_TAPS) return PG_E_UNSUP;
    const __int128 limit = (__int128)1 << 60;                              // n M and k channels stay inside int64
    if (up + M >= limit || (__int128)nsamp * channels >= limit) return PG_E_UNSUP;
    // the longest run whose span (q_last - q0) + T <= floor(((run - 1) M + L - 1) / L) + T stays below SIG_CAP
    int64_t run = 1 + (int64_t)(SIG_CAP - T - 1) * L / M;
    if (run > THREADS) run = THREADS;
    const int64_t blocks = (n_out + run - 1) / run;
    if (blocks > 0x7fffffff) return PG_E_UNSUP;
    if (format == PG_RESAMPLE_F32)
        hipLaunchKernelGGL(resample_kernel<float>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, (const float*)x,
                           (long long)nsamp, channels, taps, L, M, T, out, (long long)n_out, (int)run);
    else
        hipLaunchKernelGGL(resample_kernel<int16_t>, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, (const int16_t*)x,
                           (long long)nsamp, channels, taps, L, M, T, out, (long long)n_out, (int)run);
    return (int)hipGetLastError();
}
