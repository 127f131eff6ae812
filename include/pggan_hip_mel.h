/*
 * pggan_hip_mel.h — C-ABI of the warped-row ('melif') sound ends of libpggan_hip.so (csrc/mel.hip): magnitude + instantaneous
 * frequency as in include/pggan_hip_phase.h, with the image's M rows spaced on a mel axis and made from the H = n_fft/2 >= M linear
 * bins of a LONGER transform (Engel et al. 2019, "GANSynth": the "IF-Mel + H" representation).  A 256 x 256 image of a 2048-point
 * linear axis spends half of the image on the octave below the Nyquist frequency; the mel axis gives the low octaves their rows back.
 *
 * An ADDITION to the product boundary: include/pggan_hip.h, its PG_ABI_VERSION and its conventions (row-major contiguous tensors,
 * 16-byte aligned bases, asynchronous launches on `stream`, 0 = ok, <0 = PG_E_*, >0 = hipError_t) hold here unchanged, and
 * include/pggan_hip_phase.h is not touched.  The binding parses this header into tables of its own (_lib.MEL_SIGNATURES /
 * MEL_CONSTANTS); the wrappers are in phase.py.
 *
 * Definitions (restated for the CPU in tests/melif_ref.py).  S, logmag, ifreq, wrap, the STFT and the uint8
 * image are those of pggan_hip_phase.h; k = 0 .. H - 1 (the Nyquist bin is left out), m = 0 .. M - 1.  All fp64 without contraction,
 * no atomics, every output element has one writer and a fixed order of operations: the same bits from run to run.  Nothing is
 * allocated.
 *   table     PLAIN DATA, built on the host (phase.mel_table: numpy fp64 from mel(f) = 1127 log1p(f / 700), triangles with a
 *             half-width of at least one bin, rows normalised to sum 1; phase.MelTable takes any arrays of this shape, the
 *             identity included).  The kernels know nothing about the mel scale and do NOT check the table's contents:
 *               band_start, band_count, band_offset  int32 [M]: row m weighs the bins band_start[m] .. + band_count[m] - 1, all
 *                         inside [0, H), band_count >= 1, with weights[band_offset[m] ..]
 *               weights   fp64 [sum of band_count]
 *               lower     int32 [H] in [0, M - 2] and frac fp64 [H] in [0, 1]: bin k lies between rows lower[k] and lower[k] + 1
 *   analysis  a_m = sum_k W_mk |S_k| in ascending k from 0.0;  mel logmag = log1p(a_m);  z_m = sum_k W_mk (|S_k| cospi ifreq_k,
 *             |S_k| sinpi ifreq_k), the magnitude-weighted circular mean;  mel ifreq = atan2(Im z, Re z) / pi, and 0 where z == 0.
 *             A row whose band is ONE bin copies that bin's logmag and ifreq unchanged.
 *   synthesis a_m = expm1(max(v_m, 0)) and g_m = q_m / 128 - 1 from the image as pg_phase_spectrum_f64 takes them;  for bin k with
 *             (i, f) = (lower[k], frac[k]):  mag_k = (1 - f) a_i + f a_{i+1},  d_k = g_i + f wrap(g_{i+1} - g_i) (the shorter arc).
 *             f == 0 reads row i ALONE and f == 1 row i + 1 alone, so that a non-finite neighbour cannot leak in and a bin that
 *             sits on a row is that row exactly (the last bin of every table sits on row M - 1).  c_k[t] = sum_{s <= t} d_k[s],
 *             spec = mag_k (cospi c, sinpi c), bin H is 0.  Pieces, overlap-add and normalisation are pg_phase_pieces_f64,
 *             pg_overlap_add_f64 and pg_wave_normalize_f32 with n_fft = 2 H, not 2 M.
 * With the identity table (M = H, one-bin rows, frac 0 and the last bin 1) both entry points give the bits of pg_phase_analyse_f64
 * (bins = H) and pg_phase_spectrum_f64.
 */
#ifndef PGGAN_HIP_MEL_H
#define PGGAN_HIP_MEL_H

#include "pggan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The longest band the wrapper's own tables reach is 43 bins (128 rows of 1024 bins at 16 kHz); the kernels take any length. */

/* pg_mel_analyse_f64:  y [batch][nsamp] fp32 mono -> logmag, ifreq [batch][rows][frames] fp64, one launch: the analysis kernel of
 *                      pg_phase_analyse_f64 (one workgroup per (frame, sample), frames t and t - 1 in one complex transform) with
 *                      the warp applied while |S_k| and ifreq_k of all H bins are still in LDS, where they take the place of the
 *                      twiddle table and of the transform -- the linear planes never reach HBM.  Thread m sums row m.  n_fft a
 *                      power of two in PG_PHASE_MIN_N .. PG_PHASE_MAX_N (PG_E_UNSUP otherwise); 2 <= rows <= n_fft/2, nsamp >
 *                      n_fft/2, hop >= 1, 1 <= frames <= 1 + nsamp / hop, frames x batch <= 2^22, 1 <= batch <= 65535, no null
 *                      pointer (PG_E_ARG).
 * pg_mel_spectrum_f64: img [n][2][rows][W] fp32 -> spec [n][W frames][H + 1 bins][2] fp64 (re, im), csum [n][H][W] fp64 (may be
 *                      NULL) the running sum c, one launch: the scan of pg_phase_spectrum_f64 (one workgroup per (bin, sample))
 *                      with the fetch of the bin's one or two rows in front of it.  2 H a power of two in PG_PHASE_MIN_N ..
 *                      PG_PHASE_MAX_N (PG_E_UNSUP otherwise); 2 <= rows <= H, W a power of two <= 1024, 1 <= n <= 65535, no null
 *                      pointer but csum (PG_E_ARG).                                                                           */
int pg_mel_analyse_f64(const float* y, int64_t nsamp, int batch, double* logmag, double* ifreq, int n_fft, int hop, int rows, int frames,
                       const int32_t* band_start, const int32_t* band_count, const int32_t* band_offset, const double* weights,
                       pg_stream_t stream);
int pg_mel_spectrum_f64(const float* img, double* spec, double* csum, int n, int rows, int H, int W, const int32_t* lower,
                        const double* frac, double m_lo_in, double m_scale, double m_lo_out, double f_lo_in, double f_scale,
                        double f_lo_out, pg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PGGAN_HIP_MEL_H */
