// In-place complex radix-2 FFT of up to 2048 points over split re[] / im[] arrays of doubles in LDS, shared by the transforms of
// csrc/griffinlim.hip (Griffin-Lim's rounds) and csrc/phase.hip (magnitude + instantaneous frequency).  One workgroup of
// FFT_THREADS threads per transform.  Forward: decimation in frequency, natural order in -> bit-reversed order out (bin k lives at
// brev(k)); inverse: the same forward-twiddle butterfly network as decimation in time, bit-reversed in -> natural order out, fed the
// CONJUGATE of the spectrum, whose real part is then n_fft x the real inverse transform.  So neither direction needs a permutation
// pass, and one twiddle table e^{-2 pi i q / n_fft}, q < n_fft/2, from sincospi serves both and the periodic Hann window
// (cos(2 pi n / N) = -cos(2 pi (n - N/2) / N)).  LDS of a user: 2 x 8 N (re, im) + 2 x 4 N (the table) = 24 N bytes.
//
// Everything is fp64; the including file sets `#pragma clang fp contract(off)` BEFORE this header, so that no product is fused into
// a following sum here either.
#ifndef PGGAN_CSRC_FFT_R2_H
#define PGGAN_CSRC_FFT_R2_H

#include <hip/hip_runtime.h>

namespace fft_r2 {

constexpr int FFT_MIN_N = 8;
constexpr int FFT_MAX_N = 2048;                                            // STFT_MAX_N of sound.hip: image heights 4 .. 1024
constexpr int FFT_THREADS = 256;

// twc[q] = cos(2 pi q / N), tws[q] = sin(2 pi q / N), q < N/2; ends with a barrier
__device__ __forceinline__ void fill_twiddles(double* twc, double* tws, int n_fft, int half)
{
    for (int q = threadIdx.x; q < half; q += FFT_THREADS) {
        double sn, cs;
        sincospi(2.0 * (double)q / (double)n_fft, &sn, &cs);
        twc[q] = cs; tws[q] = sn;
    }
    __syncthreads();
}

__device__ __forceinline__ double hann(const double* twc, int n, int half)
{
    const double cs = n < half ? twc[n] : -twc[n - half];                  // cos(2 pi n / N)
    return 0.5 - 0.5 * cs;                                                 // periodic Hann: scipy.signal.hann(n_fft, sym=False)
}

// one radix-2 stage over the n_fft/2 butterflies of half-span m = 1 << s; w = e^{-2 pi i pos / (2 m)}.
// DIF: (a, b) -> (a + b, (a - b) w); DIT: (a, b) -> (a + w b, a - w b)
template <bool DIF>
__device__ __forceinline__ void fft_stage(double* re, double* im, const double* twc, const double* tws, int s, int logn, int half)
{
    const int m = 1 << s;
    for (int j = threadIdx.x; j < half; j += FFT_THREADS) {
        const int pos = j & (m - 1);
        const int i0 = ((j >> s) << (s + 1)) | pos, i1 = i0 + m;
        const int q = pos << (logn - 1 - s);                               // pos * N / (2 m) < N / 2
        const double wr = twc[q], wi = -tws[q];
        const double ar = re[i0], ai = im[i0], br = re[i1], bi = im[i1];
        if (DIF) {
            const double dr = ar - br, di = ai - bi;
            re[i0] = ar + br; im[i0] = ai + bi;
            re[i1] = dr * wr - di * wi; im[i1] = dr * wi + di * wr;
        } else {
            const double tr = br * wr - bi * wi, ti = br * wi + bi * wr;
            re[i0] = ar + tr; im[i0] = ai + ti;
            re[i1] = ar - tr; im[i1] = ai - ti;
        }
    }
    __syncthreads();
}

// position of bin k (0 <= k < N) in the bit-reversed image
__device__ __forceinline__ int brev_pos(int k, int logn) { return (int)(__brev((unsigned)k) >> (32 - logn)); }

inline bool bad_n(int n_fft) { return n_fft < FFT_MIN_N || n_fft > FFT_MAX_N || (n_fft & (n_fft - 1)); }

inline int log2_of(int n_fft)
{
    int logn = 0;
    while ((1 << logn) < n_fft) ++logn;
    return logn;
}

}  // namespace fft_r2

#endif  // PGGAN_CSRC_FFT_R2_H
