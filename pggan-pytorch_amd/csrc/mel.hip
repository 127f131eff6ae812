// Warped-row magnitude + instantaneous frequency (include/pggan_hip_mel.h): the 'melif' sound ends.
//   analysis   waveforms -> log1p of the weighted mean magnitude and the magnitude-weighted circular mean of the IF over every
//              row's band of linear bins, M rows from H = n_fft/2 >= M bins
//   spectrum   a generated two-channel image of M rows -> the complex spectrum of H bins: every bin interpolates the magnitude and
//              (along the shorter arc) the IF of its two neighbouring rows, then the running sum as in csrc/phase.hip
// The quantiser, the pieces, the overlap-add and the normalisation are the existing entry points.  After Engel et al. 2019 (GANSynth,
// "IF-Mel + H"); the project's own definition, restated in numpy in tests/melif_ref.py.
//
// Both kernels are the kernels of csrc/phase.hip with the warp put in (csrc/phase_common.h holds what they share): the table is
// plain data from the host (phase.MelTable), nothing here knows the mel scale, and nothing checks the table -- the wrapper does, once,
// when the table is built.  fp64 without contraction, no atomics, one writer per element, a fixed order: bit-identical from run to
// run, and with the identity table bit-identical to pg_phase_analyse_f64 / pg_phase_spectrum_f64 (a one-bin row copies its bin; a bin
// with frac 0 or 1 copies its row).
//
// LDS of the analysis: that of analyse_kernel, 24 N bytes (48 KB at N = 2048).  Behind the last stage's barrier the twiddle table is
// dead, and its two halves of N/2 doubles are exactly the |S_k| and ifreq_k of the H = N/2 bins; once every bin is separated the
// transform is dead too and holds |S_k| (cospi, sinpi) ifreq_k: H evaluations of sincospi per frame, however many rows share a bin.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_mel.h"

#pragma clang fp contract(off)

#include "phase_common.h"

namespace {

using namespace phase_common;

// y [batch][nsamp], logmag / ifreq [batch][rows][frames]; grid (frames, batch).  Thread m sums row m over its band.
template <int MAXN>
__global__ __launch_bounds__(FFT_THREADS) void mel_analyse_kernel(const float* __restrict__ y, long long nsamp, double* __restrict__ logmag,
                                                                  double* __restrict__ ifreq, int n_fft, int logn, int hop, int rows, int frames,
                                                                  const int32_t* __restrict__ band_start, const int32_t* __restrict__ band_count,
                                                                  const int32_t* __restrict__ band_offset, const double* __restrict__ weights)
{
    __shared__ double re[MAXN], im[MAXN];
    __shared__ double twc[MAXN / 2], tws[MAXN / 2];
    const int t = blockIdx.x, b = blockIdx.y;
    const int half = n_fft >> 1;
    constexpr int PER = MAXN / 2 / FFT_THREADS;                            // bins, and at most rows, per thread: 1 or 4
    int bs[PER], bn[PER], bo[PER];                                         // this thread's rows of the table: fetched now, needed behind the transform
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int m = threadIdx.x + i * FFT_THREADS;
        bs[i] = m < rows ? band_start[m] : 0;
        bn[i] = m < rows ? band_count[m] : 0;
        bo[i] = m < rows ? band_offset[m] : 0;
    }
    transform_frame_pair(re, im, twc, tws, y + (size_t)b * nsamp, nsamp, t, n_fft, logn, hop);
    // Every bin once: |S_k|, ifreq_k and |S_k| (cospi, sinpi) ifreq_k, which the rows that share the bin then only weigh.  They take the
    // place of the twiddle table (the last stage ended with a barrier: nobody reads a twiddle any more) and, in natural order and behind
    // a barrier of their own, of the transform itself.
    double* mag = twc;
    double* fr = tws;
    double ur[PER], ui[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int k = threadIdx.x + i * FFT_THREADS;
        if (k < half) {
            double a, f, sn, cs;
            separate_bin(re, im, k, t, n_fft, logn, &a, &f);
            sincospi(f, &sn, &cs);
            mag[k] = a; fr[k] = f;
            ur[i] = a * cs; ui[i] = a * sn;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int k = threadIdx.x + i * FFT_THREADS;
        if (k < half) { re[k] = ur[i]; im[k] = ui[i]; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int m = threadIdx.x + i * FFT_THREADS;
        if (m >= rows) break;                                              // (rows <= n_fft/2 <= PER x FFT_THREADS)
        const int s = bs[i], n = bn[i];
        double a, g;
        if (n == 1) {                                                      // the bin itself, exactly
            a = mag[s];
            g = fr[s];
        } else {
            const double* w = weights + bo[i];
            double zr = 0.0, zi = 0.0;
            a = 0.0;
            for (int j = 0; j < n; ++j) {
                a = a + w[j] * mag[s + j];
                zr = zr + w[j] * re[s + j];
                zi = zi + w[j] * im[s + j];
            }
            g = phase_over_pi(zr, zi);
        }
        const size_t o = ((size_t)b * rows + m) * (size_t)frames + t;
        logmag[o] = log1p(a);
        ifreq[o] = g;
    }
}

// img [n][2][rows][W], spec [n][W][H + 1] complex; grid (H + 1, n): workgroup (k, b) owns the row of W values of bin k, made from
// image rows lower[k] and lower[k] + 1; the workgroup of bin H writes the zero Nyquist bin.  frac is uniform in a workgroup.
__global__ __launch_bounds__(SCAN_THREADS) void mel_spectrum_kernel(const float* __restrict__ img, double* __restrict__ spec,
                                                                    double* __restrict__ csum, int rows, int H, int W,
                                                                    const int32_t* __restrict__ lower, const double* __restrict__ frac, Range rm,
                                                                    Range rf)
{
    __shared__ double part[2][SCAN_THREADS];
    const int k = blockIdx.x, b = blockIdx.y;
    double* sb = spec + (size_t)b * W * (size_t)(H + 1) * 2;
    if (k == H) {
        zero_nyquist(sb, H, W);
        return;
    }
    const double f = frac[k];
    const int i = lower[k] + (f == 1.0 ? 1 : 0);                           // f == 0 reads row i alone, f == 1 row i + 1 alone
    const float* mrow = img + (((size_t)b * 2 + 0) * rows + i) * (size_t)W;
    const float* frow = img + (((size_t)b * 2 + 1) * rows + i) * (size_t)W;
    if (f == 0.0 || f == 1.0) {
        scan_row(part, sb, csum, b, k, H, W, [&](int t) { return if_of_level(rf(frow[t])); }, [&](int t) { return mag_of_value(rm(mrow[t])); });
        return;
    }
    scan_row(part, sb, csum, b, k, H, W,
             [&](int t) {
                 const double g0 = if_of_level(rf(frow[t])), g1 = if_of_level(rf(frow[W + t]));
                 return g0 + f * wrap(g1 - g0);                            // along the shorter arc
             },
             [&](int t) {
                 const double a0 = mag_of_value(rm(mrow[t])), a1 = mag_of_value(rm(mrow[W + t]));
                 return (1.0 - f) * a0 + f * a1;
             });
}

}  // namespace

extern "C" int pg_mel_analyse_f64(const float* y, int64_t nsamp, int batch, double* logmag, double* ifreq, int n_fft, int hop, int rows,
                                  int frames, const int32_t* band_start, const int32_t* band_count, const int32_t* band_offset,
                                  const double* weights, pg_stream_t stream)
{
    if (!y || !logmag || !ifreq || nsamp <= 0 || hop <= 0 || frames <= 0 || batch <= 0 || batch > 65535) return PG_E_ARG;
    if (!band_start || !band_count || !band_offset || !weights) return PG_E_ARG;
    if (bad_n(n_fft)) return PG_E_UNSUP;
    if (rows < 2 || rows > n_fft / 2 || nsamp <= n_fft / 2) return PG_E_ARG;   // reflect padding needs more samples than the pad
    if ((int64_t)(frames - 1) * hop > nsamp) return PG_E_ARG;              // frames <= 1 + nsamp / hop
    if ((int64_t)frames * batch > (1 << 22)) return PG_E_ARG;              // grid size in threads stays below 2^32
    const int logn = log2_of(n_fft);
    if (n_fft <= 512)
        hipLaunchKernelGGL(mel_analyse_kernel<512>, dim3(frames, batch), dim3(FFT_THREADS), 0, (hipStream_t)stream, y, (long long)nsamp,
                           logmag, ifreq, n_fft, logn, hop, rows, frames, band_start, band_count, band_offset, weights);
    else
        hipLaunchKernelGGL(mel_analyse_kernel<FFT_MAX_N>, dim3(frames, batch), dim3(FFT_THREADS), 0, (hipStream_t)stream, y, (long long)nsamp,
                           logmag, ifreq, n_fft, logn, hop, rows, frames, band_start, band_count, band_offset, weights);
    return (int)hipGetLastError();
}

extern "C" int pg_mel_spectrum_f64(const float* img, double* spec, double* csum, int n, int rows, int H, int W, const int32_t* lower,
                                   const double* frac, double m_lo_in, double m_scale, double m_lo_out, double f_lo_in, double f_scale,
                                   double f_lo_out, pg_stream_t stream)
{
    if (!img || !spec || !lower || !frac || n <= 0 || n > 65535 || H <= 0 || W <= 0) return PG_E_ARG;
    if (H > FFT_MAX_N / 2 || bad_n(2 * H)) return PG_E_UNSUP;
    if (rows < 2 || rows > H) return PG_E_ARG;
    if (W > SCAN_MAX_W || (W & (W - 1))) return PG_E_ARG;
    const Range rm = {m_lo_in, m_scale, m_lo_out}, rf = {f_lo_in, f_scale, f_lo_out};
    hipLaunchKernelGGL(mel_spectrum_kernel, dim3(H + 1, n), dim3(SCAN_THREADS), 0, (hipStream_t)stream, img, spec, csum, rows, H, W, lower,
                       frac, rm, rf);
    return (int)hipGetLastError();
}
