// Magnitude + instantaneous frequency (include/pggan_hip_phase.h): the two sound ends that keep the phase.
//   analysis   waveforms -> log1p(|STFT|) and the wrapped frame-to-frame difference of the phase in units of pi (IF)
//   quantiser  both planes -> the two-channel uint8 image a DeviceImageDataset stack is made of
//   spectrum   a generated two-channel image -> the complex spectrum: magnitude from channel 0, the running sum of channel 1 as phase
//   pieces     complex spectrum -> windowed inverse transforms, the summands of pg_overlap_add_f64 (csrc/griffinlim.hip)
// After Engel et al. 2019 (GANSynth).  This is the project's own definition, not the reference's (which has abslog / reallog / raw
// only); tests/magif_ref.py restates it in numpy on oracle/sound_steps.py's STFT.
//
// Everything is fp64 without contraction, as csrc/griffinlim.hip: the host twin and the test reference are fp64 and the work is bound
// by launch latency.  No atomics, one writer per output element, a fixed order of operations: bit-identical from run to run.
//
// The analysis needs the phases of frames t and t - 1 in the same workgroup (a second launch that differences phi in place would
// have rows read and written by neighbouring threads).  Both frames are real, so they ride ONE complex transform: z = x_t + i x_{t-1},
// Z = FFT(z), and with Z' = Z[N - k]
//     X_t[k]     = (Z + conj Z') / 2   = ((zr + zr') + i (zi - zi')) / 2
//     X_{t-1}[k] = (Z - conj Z') / 2i  = ((zi + zi') + i (zr' - zr)) / 2
// At k = 0 and k = N/2, Z' is Z itself: the imaginary parts are x - x = +0 exactly, as an rfft gives them, so the DC and Nyquist rows
// sit exactly on 0 or +-pi and wrap() maps both signs of pi to the same IF.  The halving is exact.  The error of either spectrum is a
// few ulp of max|Z|, not of its own bin: inside the bound the tests weigh phases with (the phase of a quiet bin is only as well
// defined as the bin is loud).  Frame 0 has no predecessor: phi[-1] = 0 by definition, not the phase of a transform of zeros.
// LDS and banks: as gl_pieces_kernel (24 N bytes; 48 KB at N = 2048, 12 KB for the N <= 512 instantiation).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_phase.h"

#pragma clang fp contract(off)

#include "phase_common.h"

namespace {

using namespace phase_common;                                              // the frame pair, the bin separation, the row scan: shared with mel.hip

// y [batch][nsamp], logmag / ifreq [batch][bins][frames]; grid (frames, batch)
template <int MAXN>
__global__ __launch_bounds__(FFT_THREADS) void analyse_kernel(const float* __restrict__ y, long long nsamp, double* __restrict__ logmag,
                                                              double* __restrict__ ifreq, int n_fft, int logn, int hop, int bins, int frames)
{
    __shared__ double re[MAXN], im[MAXN];
    __shared__ double twc[MAXN / 2], tws[MAXN / 2];
    const int t = blockIdx.x, b = blockIdx.y;
    transform_frame_pair(re, im, twc, tws, y + (size_t)b * nsamp, nsamp, t, n_fft, logn, hop);
    for (int k = threadIdx.x; k < bins; k += FFT_THREADS) {
        double mag, fr;
        separate_bin(re, im, k, t, n_fft, logn, &mag, &fr);
        const size_t o = ((size_t)b * bins + k) * (size_t)frames + t;
        logmag[o] = log1p(mag);
        ifreq[o] = fr;
    }
}

// channel 0: clip(rint((logmag - lo) / (hi - lo) * 255), 0, 255); channel 1: rint((ifreq + 1) * 128) mod 256 (rint: half to even)
__global__ __launch_bounds__(256) void quantise_kernel(const double* __restrict__ logmag, const double* __restrict__ ifreq,
                                                       uint8_t* __restrict__ out, long long total, long long plane, double lo, double span)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / plane, e = i - b * plane;
        const double m = rint((logmag[i] - lo) / span * 255.0);
        const double f = rint((ifreq[i] + 1.0) * (double)(PG_PHASE_IF_LEVELS / 2));
        const double fm = f - (double)PG_PHASE_IF_LEVELS * floor(f / (double)PG_PHASE_IF_LEVELS);     // exact: f is an integer
        uint8_t* ob = out + (size_t)b * 2 * plane;
        ob[e] = (uint8_t)(int)fmin(fmax(m, 0.0), 255.0);
        ob[plane + e] = (uint8_t)(int)fm;
    }
}

// img [n][2][H][W], spec [n][W][H + 1] complex; grid (H + 1, n): workgroup (k, b) owns the row of W values of bin k (scan_row of
// csrc/phase_common.h), the workgroup of bin H writes the zero Nyquist bin.  csum [n][H][W] (may be NULL) receives the running sum
// itself, the phase in units of pi before it is reduced by sincospi.
__global__ __launch_bounds__(SCAN_THREADS) void spectrum_kernel(const float* __restrict__ img, double* __restrict__ spec,
                                                                double* __restrict__ csum, int H, int W, Range rm, Range rf)
{
    __shared__ double part[2][SCAN_THREADS];
    const int k = blockIdx.x, b = blockIdx.y;
    double* sb = spec + (size_t)b * W * (size_t)(H + 1) * 2;
    if (k == H) {
        zero_nyquist(sb, H, W);
        return;
    }
    const float* mrow = img + (((size_t)b * 2 + 0) * H + k) * (size_t)W;
    const float* frow = img + (((size_t)b * 2 + 1) * H + k) * (size_t)W;
    scan_row(part, sb, csum, b, k, H, W, [&](int t) { return if_of_level(rf(frow[t])); }, [&](int t) { return mag_of_value(rm(mrow[t])); });
}

// spec [batch][frames][n_fft/2 + 1] complex, pieces [batch][frames][n_fft]; grid (frames, batch).  The second half of gl_pieces_kernel
// with a complex spectrum: bins above N/2 are the Hermitian extension, irfft ignores the imaginary parts of DC and Nyquist, the image
// is stored conjugated at the bit-reversed positions (csrc/fft_r2.h).
template <int MAXN>
__global__ __launch_bounds__(FFT_THREADS) void pieces_kernel(const double* __restrict__ spec, double* __restrict__ pieces, int n_fft, int logn,
                                                             int frames)
{
    __shared__ double re[MAXN], im[MAXN];
    __shared__ double twc[MAXN / 2], tws[MAXN / 2];
    const int t = blockIdx.x, b = blockIdx.y;
    const int half = n_fft >> 1;
    fill_twiddles(twc, tws, n_fft, half);
    const double* sp = spec + ((size_t)b * frames + t) * (size_t)(half + 1) * 2;
    for (int k = threadIdx.x; k <= half; k += FFT_THREADS) {
        const int p = brev_pos(k, logn);
        const double vr = sp[2 * k];
        const double vi = (k == 0 || k == half) ? 0.0 : sp[2 * k + 1];
        re[p] = vr; im[p] = -vi;
        if (k != 0 && k != half) {
            const int pm = brev_pos(n_fft - k, logn);
            re[pm] = vr; im[pm] = vi;
        }
    }
    __syncthreads();
    for (int s = 0; s < logn; ++s) fft_stage<false>(re, im, twc, tws, s, logn, half);
    double* pc = pieces + ((size_t)b * frames + t) * (size_t)n_fft;
    const double inv_n = 1.0 / (double)n_fft;                               // a power of two: exact
    for (int n = threadIdx.x; n < n_fft; n += FFT_THREADS)
        pc[n] = (hann(twc, n, half) * (2.0 / 3.0)) * (re[n] * inv_n);       // window * 2/3 times irfft, as the host's product
}

}  // namespace

extern "C" int pg_phase_analyse_f64(const float* y, int64_t nsamp, int batch, double* logmag, double* ifreq, int n_fft, int hop, int bins,
                                    int frames, pg_stream_t stream)
{
    if (!y || !logmag || !ifreq || nsamp <= 0 || hop <= 0 || bins <= 0 || frames <= 0 || batch <= 0 || batch > 65535) return PG_E_ARG;
    if (bad_n(n_fft)) return PG_E_UNSUP;
    if (bins > n_fft / 2 + 1 || nsamp <= n_fft / 2) return PG_E_ARG;       // reflect padding needs more samples than the pad
    if ((int64_t)(frames - 1) * hop > nsamp) return PG_E_ARG;              // frames <= 1 + nsamp / hop
    if ((int64_t)frames * batch > (1 << 22)) return PG_E_ARG;              // grid size in threads stays below 2^32
    const int logn = log2_of(n_fft);
    if (n_fft <= 512)
        hipLaunchKernelGGL(analyse_kernel<512>, dim3(frames, batch), dim3(FFT_THREADS), 0, (hipStream_t)stream, y, (long long)nsamp, logmag,
                           ifreq, n_fft, logn, hop, bins, frames);
    else
        hipLaunchKernelGGL(analyse_kernel<FFT_MAX_N>, dim3(frames, batch), dim3(FFT_THREADS), 0, (hipStream_t)stream, y, (long long)nsamp,
                           logmag, ifreq, n_fft, logn, hop, bins, frames);
    return (int)hipGetLastError();
}

extern "C" int pg_phase_quantise_u8(const double* logmag, const double* ifreq, uint8_t* out, int batch, int64_t plane, double lo, double hi,
                                    pg_stream_t stream)
{
    if (!logmag || !ifreq || !out || batch <= 0 || plane <= 0 || !(hi > lo)) return PG_E_ARG;
    const int64_t total = (int64_t)batch * plane;
    int64_t g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(quantise_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, logmag, ifreq, out, (long long)total,
                       (long long)plane, lo, hi - lo);
    return (int)hipGetLastError();
}

extern "C" int pg_phase_spectrum_f64(const float* img, double* spec, double* csum, int n, int H, int W, double m_lo_in, double m_scale, double m_lo_out,
                                     double f_lo_in, double f_scale, double f_lo_out, pg_stream_t stream)
{
    if (!img || !spec || n <= 0 || n > 65535 || H <= 0 || W <= 0) return PG_E_ARG;
    if (H > FFT_MAX_N / 2 || bad_n(2 * H)) return PG_E_UNSUP;
    if (W > SCAN_MAX_W || (W & (W - 1))) return PG_E_ARG;
    const Range rm = {m_lo_in, m_scale, m_lo_out}, rf = {f_lo_in, f_scale, f_lo_out};
    hipLaunchKernelGGL(spectrum_kernel, dim3(H + 1, n), dim3(SCAN_THREADS), 0, (hipStream_t)stream, img, spec, csum, H, W, rm, rf);
    return (int)hipGetLastError();
}

extern "C" int pg_phase_pieces_f64(const double* spec, double* pieces, int n_fft, int frames, int batch, pg_stream_t stream)
{
    if (!spec || !pieces || frames <= 0 || batch <= 0 || batch > 65535) return PG_E_ARG;
    if (bad_n(n_fft)) return PG_E_UNSUP;
    if ((int64_t)frames * batch > (1 << 22)) return PG_E_ARG;              // grid size in threads stays below 2^32
    const int logn = log2_of(n_fft);
    if (n_fft <= 512)
        hipLaunchKernelGGL(pieces_kernel<512>, dim3(frames, batch), dim3(FFT_THREADS), 0, (hipStream_t)stream, spec, pieces, n_fft, logn,
                           frames);
    else
        hipLaunchKernelGGL(pieces_kernel<FFT_MAX_N>, dim3(frames, batch), dim3(FFT_THREADS), 0, (hipStream_t)stream, spec, pieces, n_fft,
                           logn, frames);
    return (int)hipGetLastError();
}
