// What csrc/phase.hip (magnitude + instantaneous frequency on the transform's own bins) and csrc/mel.hip (the same on warped rows)
// both need: the analysis of one frame in LDS up to the per-bin magnitude and IF, and the scan of one spectrum row along time.  The
// including file sets `#pragma clang fp contract(off)` BEFORE this header and csrc/fft_r2.h, as for the transform: every expression
// here is evaluated as written, so a kernel built on these pieces gives the bits phase.hip gave when they were its own lines.
#ifndef PGGAN_CSRC_PHASE_COMMON_H
#define PGGAN_CSRC_PHASE_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_phase.h"
#include "fft_r2.h"

namespace phase_common {

using namespace fft_r2;

static_assert(PG_PHASE_MIN_N == FFT_MIN_N && PG_PHASE_MAX_N == FFT_MAX_N, "the header states the transform's limits");

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_MAX_W = 1024;
constexpr int SCAN_CHUNK = SCAN_MAX_W / SCAN_THREADS;

constexpr double PI = 3.14159265358979323846;                              // numpy's np.pi

__device__ __forceinline__ double phase_over_pi(double re, double im)
{
    return (re == 0.0 && im == 0.0) ? 0.0 : atan2(im, re) / PI;
}

__device__ __forceinline__ double wrap(double d) { return d - 2.0 * floor(d / 2.0 + 0.5); }

__device__ __forceinline__ long long reflect(long long j, long long nsamp)
{
    if (j < 0) j = -j;                                                     // np.pad(mode='reflect'); nsamp > n_fft/2 keeps both in range
    if (j >= nsamp) j = 2 * (nsamp - 1) - j;
    return j;
}

// Frames t and t - 1 of sample row yb as the real and the imaginary part of one forward transform: fills the twiddle table, loads
// the windowed frames and runs the stages.  On return (behind a barrier) bin k of Z = FFT(x_t + i x_{t-1}) lives at brev_pos(k).
__device__ __forceinline__ void transform_frame_pair(double* re, double* im, double* twc, double* tws, const float* __restrict__ yb,
                                                     long long nsamp, int t, int n_fft, int logn, int hop)
{
    const int half = n_fft >> 1;
    fill_twiddles(twc, tws, n_fft, half);
    for (int n = threadIdx.x; n < n_fft; n += FFT_THREADS) {
        const double w = hann(twc, n, half);
        const long long j = (long long)t * hop + n - half;                 // index into the unpadded signal, as gl_pieces_kernel
        re[n] = w * (double)yb[reflect(j, nsamp)];
        im[n] = t > 0 ? w * (double)yb[reflect(j - hop, nsamp)] : 0.0;
    }
    __syncthreads();
    for (int s = logn - 1; s >= 0; --s) fft_stage<true>(re, im, twc, tws, s, logn, half);
}

// |S_k| of frame t and the wrapped difference of its phase to frame t - 1's (phi[k][-1] = 0), from the transform of the pair
__device__ __forceinline__ void separate_bin(const double* re, const double* im, int k, int t, int n_fft, int logn, double* mag, double* ifreq)
{
    const int p = brev_pos(k, logn), pm = brev_pos((n_fft - k) & (n_fft - 1), logn);
    const double zr = re[p], zi = im[p], mr = re[pm], mi = im[pm];
    const double xr = (zr + mr) * 0.5, xi = (zi - mi) * 0.5;               // frame t
    double prev = 0.0;                                                     // phi[k][-1] = 0
    if (t > 0) prev = phase_over_pi((zi + mi) * 0.5, (mr - zr) * 0.5);     // frame t - 1
    *mag = hypot(xr, xi);
    *ifreq = wrap(phase_over_pi(xr, xi) - prev);
}

struct Range {                                                             // adjust_dynamic_range (utils.py:24-30), resolved on the host
    double lo_in, scale, lo_out;
    __device__ __forceinline__ double operator()(float v) const { return ((double)v - lo_in) * scale + lo_out; }
};

__device__ __forceinline__ double if_of_level(double q) { return q / (double)(PG_PHASE_IF_LEVELS / 2) - 1.0; }
__device__ __forceinline__ double mag_of_value(double v) { return expm1(fmax(v, 0.0)); }   // a generator can undershoot; a negative magnitude would flip the phase

// The row of W values of bin k of sample b: thread i sums its `chunk` = max(1, W / 256) consecutive IF values ifreq_at(t), the partial
// sums are scanned in LDS (Hillis-Steele, two buffers), then every value gets the sum of the chunks before it and is written as
// mag_at(t) (cospi c, sinpi c).  csum [n][H][W] (may be NULL) receives the running sum c itself.  sb is sample b's spectrum [W][H + 1].
template <class IfAt, class MagAt>
__device__ __forceinline__ void scan_row(double (*part)[SCAN_THREADS], double* __restrict__ sb, double* __restrict__ csum, int b, int k,
                                         int H, int W, IfAt ifreq_at, MagAt mag_at)
{
    const int chunk = W > SCAN_THREADS ? W / SCAN_THREADS : 1;             // W is a power of two: 1, 2 or 4
    const int t0 = threadIdx.x * chunk;
    double c[SCAN_CHUNK];
    double run = 0.0;
#pragma unroll
    for (int i = 0; i < SCAN_CHUNK; ++i) {
        if (i < chunk && t0 + i < W) run = run + ifreq_at(t0 + i);
        c[i] = run;
    }
    part[0][threadIdx.x] = t0 < W ? run : 0.0;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
        const double v = part[cur][threadIdx.x];
        part[cur ^ 1][threadIdx.x] = threadIdx.x >= d ? part[cur][threadIdx.x - d] + v : v;
        cur ^= 1;
        __syncthreads();
    }
    const double before = threadIdx.x > 0 ? part[cur][threadIdx.x - 1] : 0.0;
#pragma unroll
    for (int i = 0; i < SCAN_CHUNK; ++i) {
        if (i < chunk && t0 + i < W) {
            const double mag = mag_at(t0 + i);
            const double ph = before + c[i];
            if (csum) csum[((size_t)b * H + k) * (size_t)W + t0 + i] = ph;
            double sn, cs;
            sincospi(ph, &sn, &cs);
            double* o = sb + ((size_t)(t0 + i) * (H + 1) + k) * 2;
            o[0] = mag * cs; o[1] = mag * sn;
        }
    }
}

// the zero Nyquist bin of sample b's spectrum
__device__ __forceinline__ void zero_nyquist(double* __restrict__ sb, int H, int W)
{
    for (int t = threadIdx.x; t < W; t += SCAN_THREADS) {
        double* o = sb + ((size_t)t * (H + 1) + H) * 2;
        o[0] = 0.0; o[1] = 0.0;
    }
}

}  // namespace phase_common

#endif  // PGGAN_CSRC_PHASE_COMMON_H
