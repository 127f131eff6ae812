// Sound end of the output step on the device: SoundSaver.image_to_sound / reconstruct_from_magnitude, reference
// output_postprocess.py:92-127 -- the padded and range-adjusted spectrum (:109-118), Griffin-Lim's rounds of lbr.stft / np.angle /
// lbr.istft (:95-101), the single lbr.istft of 'reallog' (:116), signal / |signal|.max() (:126) with the nearest upsample (:152) and the
// float32 cast of the WAV writer (:136).  librosa's transforms are the published definitions restated in oracle/sound_steps.py (parity
// unpinned, see there): periodic Hann window, reflect padding by n_fft/2, frame t = padded[t hop, t hop + n_fft), rFFT; inverse: irfft,
// window x 2/3, overlap-add, the centring pad cut off.
//
// Everything is fp64 without contraction: the host path and the oracle are fp64, the work is bound by launch latency and not by rate
// (a round is 2 x frames x batch transforms of <= 2048 points), and Griffin-Lim does not amplify round-off, which lets the tests hold
// the whole iteration to 1e-9.  No atomics: every output element has one writer and a fixed summation order, so results are
// bit-identical from run to run.
//
// The transform (gl_pieces_kernel; its radix-2 stages, twiddle table and window are csrc/fft_r2.h, shared with csrc/phase.hip): one
// workgroup per (frame, sample), the frame as split re[] / im[] arrays of doubles in LDS, a
// complex radix-2 FFT of n_fft points in place.  Forward: decimation in frequency, natural order in -> bit-reversed order out.  The
// phase projection works on the bit-reversed image (bin k lives at brev(k)) and stores the CONJUGATE of the Hermitian-extended
// spectrum; the inverse is then the same forward-twiddle butterfly network as decimation in time, bit-reversed in -> natural order
// out, whose real part is n_fft x the real inverse transform.  So neither direction needs a permutation pass and one twiddle table
// e^{-2 pi i q / n_fft}, q < n_fft/2, from sincospi serves both and the window (cos(2 pi n / N) = -cos(2 pi (n - N/2) / N)).
// LDS: 2 x 8 N + 2 x 4 N = 24 N bytes = 48 KB at N = 2048 (12 KB for the N <= 512 instantiation).
// Banks (64 x 4 B; ds_read_b64 / ds_write_b64 of 8-byte elements, conflicts counted per 32-lane half = 32 doubles = one bank row):
// lane j of a stage with half-span m touches element i0 = 2 m (j / m) + j % m and i0 + m in separate instructions.  For m >= 32 the
// 32 lanes of a half read 32 consecutive doubles: conflict-free.  For m = 1 .. 16 they read runs of m doubles every 2 m, i.e. half of
// two bank rows: 2-way, in 5 of the up to 11 stages.  A skew of the image would have to differ per stage to remove that; the stages
// are bound by the fp64 butterfly and the barrier, so the image stays linear.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip.h"

#pragma clang fp contract(off)

#include "fft_r2.h"

namespace {

using namespace fft_r2;                                                    // fft_stage, hann, the twiddle table: shared with phase.hip

constexpr int GL_MIN_N = FFT_MIN_N;
constexpr int GL_MAX_N = FFT_MAX_N;                                        // STFT_MAX_N of sound.hip: image heights 4 .. 1024
constexpr int GL_THREADS = FFT_THREADS;

// x [batch][nsamp] (NULL: the spectrum is spec itself, taken as real), spec [batch][frames][n_fft/2 + 1], pieces [batch][frames][n_fft]
template <int MAXN>
__global__ __launch_bounds__(GL_THREADS) void gl_pieces_kernel(const double* __restrict__ x, long long nsamp, const double* __restrict__ spec,
                                                               double* __restrict__ pieces, int n_fft, int logn, int hop, int frames)
{
    __shared__ double re[MAXN], im[MAXN];
    __shared__ double twc[MAXN / 2], tws[MAXN / 2];
    const int t = blockIdx.x, b = blockIdx.y;
    const int half = n_fft >> 1;
    fill_twiddles(twc, tws, n_fft, half);
    if (x) {
        const double* xb = x + (size_t)b * nsamp;
        for (int n = threadIdx.x; n < n_fft; n += GL_THREADS) {
            long long j = (long long)t * hop + n - half;                   // index into the unpadded signal, as stft_image_kernel
            if (j < 0) j = -j;                                             // np.pad(mode='reflect'); nsamp > half keeps both in range
            if (j >= nsamp) j = 2 * (nsamp - 1) - j;
            re[n] = hann(twc, n, half) * xb[j];
            im[n] = 0.0;
        }
        __syncthreads();
        for (int s = logn - 1; s >= 0; --s) fft_stage<true>(re, im, twc, tws, s, logn, half);
    }
    // bins 0 .. N/2 keep the target magnitude and the phase of S (np.angle(0) = 0: S == 0 -> the phase factor (1, 0)); bins above N/2 are
    // the Hermitian extension; irfft ignores the imaginary parts of DC and Nyquist.  Stored conjugated (see the head of the file).  Bin k
    // is read at brev(k) by the thread that rewrites it; the positions brev(N - k) it also writes are read by nobody.
    const double* sp = spec + ((size_t)b * frames + t) * (size_t)(half + 1);
    for (int k = threadIdx.x; k <= half; k += GL_THREADS) {
        const int p = (int)(__brev((unsigned)k) >> (32 - logn));
        const double mag = sp[k];
        double vr = mag, vi = 0.0;
        if (x) {
            const double sr = re[p], si = im[p];
            double ur = 1.0, ui = 0.0;
            if (sr != 0.0 || si != 0.0) { const double a = hypot(sr, si); ur = sr / a; ui = si / a; }
            vr = mag * ur; vi = mag * ui;
        }
        if (k == 0 || k == half) vi = 0.0;
        re[p] = vr; im[p] = -vi;
        if (k != 0 && k != half) {
            const int pm = (int)(__brev((unsigned)(n_fft - k)) >> (32 - logn));
            re[pm] = vr; im[pm] = vi;
        }
    }
    __syncthreads();
    for (int s = 0; s < logn; ++s) fft_stage<false>(re, im, twc, tws, s, logn, half);
    double* pc = pieces + ((size_t)b * frames + t) * (size_t)n_fft;
    const double inv_n = 1.0 / (double)n_fft;                               // a power of two: exact
    for (int n = threadIdx.x; n < n_fft; n += GL_THREADS)
        pc[n] = (hann(twc, n, half) * (2.0 / 3.0)) * (re[n] * inv_n);       // window * 2/3 times irfft, as the host's product
}

// gather form of y[t hop : t hop + N] += pieces[t]; x = y[N/2 : -N/2]: sample j sums, in ascending t from 0.0 as the host loop does,
// the frames that cover padded index q = j + N/2: t hop <= q <= t hop + N - 1
__global__ __launch_bounds__(256) void overlap_add_kernel(const double* __restrict__ pieces, double* __restrict__ x, long long nsamp,
                                                          int n_fft, int hop, int frames)
{
    const int b = blockIdx.y;
    const double* pb = pieces + (size_t)b * frames * (size_t)n_fft;
    for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < nsamp; j += (long long)gridDim.x * blockDim.x) {
        const long long q = j + n_fft / 2;
        long long t0 = q - (n_fft - 1);
        t0 = t0 > 0 ? (t0 + hop - 1) / hop : 0;
        long long t1 = q / hop;
        if (t1 > frames - 1) t1 = frames - 1;
        double acc = 0.0;
        for (long long t = t0; t <= t1; ++t) acc += pb[t * n_fft + (q - t * hop)];
        x[(size_t)b * nsamp + j] = acc;
    }
}

__global__ __launch_bounds__(1024) void peak_kernel(const double* __restrict__ x, long long nsamp, double* __restrict__ peak)
{
    __shared__ double sm[16];
    const double* xb = x + (size_t)blockIdx.x * nsamp;
    double m = 0.0;
    for (long long i = threadIdx.x; i < nsamp; i += blockDim.x) m = fmax(m, fabs(xb[i]));
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, sm[w]);
        peak[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(256) void normalize_kernel(const double* __restrict__ x, float* __restrict__ out, long long nsamp, int repeat,
                                                        const double* __restrict__ peak)
{
    const int b = blockIdx.y;
    const double pk = peak[b];
    const long long total = nsamp * repeat;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x)
        out[(size_t)b * total + o] = (float)(x[(size_t)b * nsamp + o / repeat] / pk);   // fp64 quotient, then round to nearest fp32
}

// MODE 0 'abslog': the adjusted value itself is the magnitude (the reference does not invert log(1 + |s|)); MODE 1 'reallog':
// (exp(|v|) - 1) * sign(v).  Row H is the zero padding, adjusted like every other value (127.5 for (-1, 1) -> (0, 255)).
// One thread per output element, bins fastest: the stores are contiguous, the loads walk a column of the image (rows of neighbouring
// frames share cache lines); this runs once per snapshot.
template <int MODE>
__global__ __launch_bounds__(256) void spectrum_kernel(const float* __restrict__ img, double* __restrict__ spec, long long total, int H, int W,
                                                       double lo_in, double scale, double lo_out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(i % (H + 1));
        const long long r = i / (H + 1);
        const int t = (int)(r % W);
        const long long b = r / W;
        const double s = k < H ? (double)img[((size_t)b * H + k) * W + t] : 0.0;
        double v = (s - lo_in) * scale + lo_out;                            // adjust_dynamic_range, utils.py:24-30
        if (MODE == 1) {
            const double sg = v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : 0.0;
            v = (exp(fabs(v)) - 1.0) * sg;
        }
        spec[i] = v;
    }
}

unsigned blocks_for(int64_t n)
{
    int64_t g = (n + 255) / 256;
    return (unsigned)(g > 4096 ? 4096 : g);
}

}  // namespace

extern "C" int pg_gl_spectrum_f64(const float* img, double* spec, int n, int H, int W, double lo_in, double scale, double lo_out,
                                  int mode, pg_stream_t stream)
{
    if (!img || !spec || n <= 0 || H <= 0 || W <= 0) return PG_E_ARG;
    if (mode != PG_SOUND_ABSLOG && mode != PG_SOUND_REALLOG) return PG_E_ARG;
    if (H > GL_MAX_N / 2 || bad_n(2 * H)) return PG_E_UNSUP;
    const int64_t total = (int64_t)n * W * (H + 1);
    if (mode == PG_SOUND_ABSLOG)
        hipLaunchKernelGGL(spectrum_kernel<0>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, img, spec, (long long)total, H, W,
                           lo_in, scale, lo_out);
    else
        hipLaunchKernelGGL(spectrum_kernel<1>, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, img, spec, (long long)total, H, W,
                           lo_in, scale, lo_out);
    return (int)hipGetLastError();
}

extern "C" int pg_gl_pieces_f64(const double* x, int64_t nsamp, const double* spec, double* pieces, int n_fft, int hop, int frames,
                                int batch, pg_stream_t stream)
{
    if (!spec || !pieces || nsamp <= 0 || hop <= 0 || frames <= 0 || batch <= 0 || batch > 65535) return PG_E_ARG;
    if (bad_n(n_fft)) return PG_E_UNSUP;
    if (nsamp <= n_fft / 2 || nsamp != (int64_t)hop * (frames - 1)) return PG_E_ARG;   // reflect padding; frames = 1 + nsamp / hop
    if ((int64_t)frames * batch > (1 << 22)) return PG_E_ARG;                            // grid size in threads stays below 2^32
    int logn = 0;
    while ((1 << logn) < n_fft) ++logn;
    if (n_fft <= 512)
        hipLaunchKernelGGL(gl_pieces_kernel<512>, dim3(frames, batch), dim3(GL_THREADS), 0, (hipStream_t)stream, x, (long long)nsamp, spec,
                           pieces, n_fft, logn, hop, frames);
    else
        hipLaunchKernelGGL(gl_pieces_kernel<GL_MAX_N>, dim3(frames, batch), dim3(GL_THREADS), 0, (hipStream_t)stream, x, (long long)nsamp, spec,
                           pieces, n_fft, logn, hop, frames);
    return (int)hipGetLastError();
}

extern "C" int pg_overlap_add_f64(const double* pieces, double* x, int64_t nsamp, int n_fft, int hop, int frames, int batch,
                                  pg_stream_t stream)
{
    if (!pieces || !x || nsamp <= 0 || hop <= 0 || frames <= 0 || batch <= 0 || batch > 65535) return PG_E_ARG;
    if (bad_n(n_fft)) return PG_E_UNSUP;
    if (nsamp != (int64_t)hop * (frames - 1)) return PG_E_ARG;
    hipLaunchKernelGGL(overlap_add_kernel, dim3(blocks_for(nsamp), batch), dim3(256), 0, (hipStream_t)stream, pieces, x, (long long)nsamp,
                       n_fft, hop, frames);
    return (int)hipGetLastError();
}

extern "C" int pg_wave_normalize_f32(const double* x, float* out, int64_t nsamp, int repeat, int batch, double* peak, pg_stream_t stream)
{
    if (!x || !out || !peak || nsamp <= 0 || repeat <= 0 || batch <= 0 || batch > 65535) return PG_E_ARG;
    hipLaunchKernelGGL(peak_kernel, dim3(batch), dim3(1024), 0, (hipStream_t)stream, x, (long long)nsamp, peak);
    hipLaunchKernelGGL(normalize_kernel, dim3(blocks_for(nsamp * repeat), batch), dim3(256), 0, (hipStream_t)stream, x, out, (long long)nsamp,
                       repeat, peak);
    return (int)hipGetLastError();
}
