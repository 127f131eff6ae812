/*
 * pggan_hip_resample.h — C-ABI of the rate conversion in front of the sound ends of libpggan_hip.so (csrc/resample.hip): a recording
 * at rate_in Hz -> the mono float32 waveform at rate_out Hz that the STFT kernels take, by a polyphase windowed-sinc filter.  The
 * reference hands its `frequency` to librosa.load, which resamples every file before the transform (dataset.py:19, :273, :286).
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged.  The binding
 * parses this header into tables of its own (_lib.RESAMPLE_SIGNATURES / RESAMPLE_CONSTANTS); the wrappers are in sound.py.
 *
 * Definition (restated for the CPU in tests/resample_ref.py; sound.resample(device='cpu') is the numpy twin).
 * The project's own and UNPINNED: librosa and resampy are not in the image; the default parameters are resampy's published
 * 'kaiser_best'.  Rates are positive integers; g = gcd(rate_in, rate_out), L = rate_out / g, M = rate_in / g.
 *   table    PLAIN DATA, built on the host in numpy float64 (sound.resample_table; sound.ResampleTable takes any finite [L][T] table,
 *            the kernel knows no filter):
 *              c = rolloff * min(1, L / M),  W = zeros / c,  half = ceil(W),  T = 2 half
 *              for phase r in [0, L) and tap j in [0, T):  tau = (r + L (half - 1 - j)) / L (exact integers, one division),
 *              u = tau / W,  taps[r][j] = c sinc(c tau) (i0(beta sqrt(1 - u u)) / i0(beta) if |u| < 1 else 0)
 *            defaults zeros = 64, rolloff = 0.9475937167399596, beta = 14.769656459379492: 44100 -> 16000 has L = 160, M = 441,
 *            T = 374; 48000 -> 16000 has L = 1, T = 406; 16000 -> 44100 has L = 441, T = 136.
 *   mix-down m[k] float32, the bits of csrc/sound.hip: the sample itself for one channel, the float32 sum in channel order divided by
 *            2.0f for more; int16 input is converted v / 32768 to float32 first (exact).
 *   output   n_out = ceil(nsamp L / M).  For n in [0, n_out), in int64:  p = n M,  q = p div L,  r = p mod L;  acc = 0.0;  for
 *            j = 0 .. T - 1 ascending, k = q - half + 1 + j:  if 0 <= k < nsamp then acc = acc + taps[r][j] * (double)m[k] -- an fp64
 *            product, then an fp64 sum, no contraction.  Terms outside the signal are SKIPPED and nothing outside it is loaded.
 *            out[n] = (float)acc, one rounding.
 * No atomics, one writer per output and a fixed order of operations: the same bits from run to run, and the bits of the numpy twin.
 * Nothing is allocated.
 */
#ifndef PGGAN_HIP_RESAMPLE_H
#define PGGAN_HIP_RESAMPLE_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `format` of x */
#define PG_RESAMPLE_F32 0
#define PG_RESAMPLE_I16 1
/* the caps on L and T (PG_E_UNSUP beyond them): 44100 -> 16001 has L = 16001 */
#define PG_RESAMPLE_MAX_PHASES 4096
#define PG_RESAMPLE_MAX_TAPS   4096

/* pg_resample_mono:  x [nsamp][channels] float32 or int16 (`format`) -> out [n_out] float32 mono at L / M times the rate, one launch.
 *                    taps [L][T] fp64 row-major, as defined above: the kernel reads this layout as it stands.
 *                    PG_E_ARG: a null pointer, nsamp < 1, channels < 1, an unknown format, L < 1, M < 1, T odd or < 2,
 *                    n_out != ceil(nsamp L / M).  PG_E_ALIGN: x, taps or out not 16-byte aligned.  PG_E_UNSUP: L >
 *                    PG_RESAMPLE_MAX_PHASES, T > PG_RESAMPLE_MAX_TAPS (or a signal of more than 2^60 values).                      */
int pg_resample_mono(const void* x, int format, int64_t nsamp, int channels,
                     const double* taps, int L, int M, int T,
                     float* out, int64_t n_out, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_RESAMPLE_H */
