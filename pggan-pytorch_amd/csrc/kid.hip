// The tile sums of the cubic polynomial kernel between two sets of feature vectors (include/pggan_hip_kid.h):
//   pg_kid_tilesums_f64 : sums[a][b] = sum over the pairs of a 64 x 64 tile of ((gamma x_i . y_j + coef0)^3), in fp64
// for the unbiased MMD^2 estimator `kid` (metrics.kid_statistic).  The Gram matrix never exists: the kernel function and the reduction sit
// behind the GEMM, and what leaves the device is one fp64 value per tile.  fp64 without contraction, no atomics, one writer per output
// and a fixed order (stated in the header): two calls give the same bits.
//
// One workgroup of 4 waves per tile (a, b); the grid is (B, A), and in the self form the workgroups below the diagonal return at once
// (their value is written by the mirror tile).  The features are walked in chunks of KC = 32.  Thread (sr, sq) = (tid >> 3, tid & 7)
// loads the four floats of features 4 sq .. 4 sq + 3 of rows sr and sr + 32 of both sides one chunk ahead -- 8 lanes cover the 128
// bytes a row has in a chunk -- and stores them as doubles, or exact zeros for a row at or past M / N or a feature at or past F, into
// Xs / Ys [TILE][LDP] (a diagonal tile stages one side and reads it twice).  The images are ROW-major, as the tensors are: the operand
// of lane l for k-step k0 is row (l & 15), feature k0 + (l >> 4).  LDP = KC + 2 doubles: consecutive rows start 4 banks (of 64) apart,
// so the 16 rows x 2 features that half a wave reads in one 8-byte access fall on 64 distinct banks (the 16-byte stores, 16 a chunk
// against 32 matrix instructions a wave, are not conflict-free and do not matter).  Wave (wr, wc) owns the 32 x 32 quarter (wr, wc)
// as 2 x 2 MFMA tiles.  The instruction computes D = A B + C with A [16][4] and B [4][16]: lane l supplies A[l & 15][l >> 4] and
// B[l >> 4][l & 15] and holds D[(l >> 4) + 4 g][l & 15] in element g of its result -- NOT the fp32 16x16 map (csrc/embed.hip says
// the same of fd_cov_kernel).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_kid.h"

#pragma clang fp contract(off)

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int TILE = PG_KID_TILE;
constexpr int KC = 32;                     // features of one staged chunk
constexpr int LDP = KC + 2;                // row pitch of the staged operands, in doubles
static_assert(TILE == 64 && KC == 32 && PG_KID_MIN_F % 16 == 0, "the kernel is written for 64 x 64 tiles and 32-feature chunks");

inline bool misaligned(const void* p, uintptr_t a = 16) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// grid (B, A): the sum of tile (blockIdx.y, blockIdx.x)
__global__ __launch_bounds__(256) void kid_tile_kernel(const float* __restrict__ x, int64_t M, const float* __restrict__ y, int64_t N, int F,
                                                       double gamma, double coef0, int self, int skip, double* __restrict__ sums)
{
    __shared__ __attribute__((aligned(16))) double Xs[TILE * LDP];
    __shared__ __attribute__((aligned(16))) double Ys[TILE * LDP];
    __shared__ double wsum[4];
    const int a = blockIdx.y, b = blockIdx.x;
    if (self && b < a) return;                                 // (the whole workgroup: no barrier is left waiting)
    const bool diag = self && a == b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int sr = tid >> 3, sc = 4 * (tid & 7);
    const int64_t i0 = (int64_t)a * TILE, j0 = (int64_t)b * TILE;
    const int nchunks = (F + KC - 1) / KC;
    const double* const Bsrc = diag ? Xs : Ys;
    float4 ra[2], rb[2];

    auto load = [&](int chunk) {
        const int f = chunk * KC + sc;                         // F % 16 == 0: the four features of a thread are inside or outside together
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t i = i0 + sr + 32 * h, j = j0 + sr + 32 * h;
            ra[h] = rb[h] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (f < F && i < M) ra[h] = *reinterpret_cast<const float4*>(x + i * F + f);
            if (!diag && f < F && j < N) rb[h] = *reinterpret_cast<const float4*>(y + j * F + f);
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            double2* p = reinterpret_cast<double2*>(Xs + (sr + 32 * h) * LDP + sc);
            p[0] = make_double2((double)ra[h].x, (double)ra[h].y);
            p[1] = make_double2((double)ra[h].z, (double)ra[h].w);
            if (!diag) {
                double2* q = reinterpret_cast<double2*>(Ys + (sr + 32 * h) * LDP + sc);
                q[0] = make_double2((double)rb[h].x, (double)rb[h].y);
                q[1] = make_double2((double)rb[h].z, (double)rb[h].w);
            }
        }
    };

    v4d acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int fk = lane >> 4, fc = lane & 15;
    const double* const ar = Xs + (wr * 32 + fc) * LDP + fk;
    const double* const br = Bsrc + (wc * 32 + fc) * LDP + fk;
    load(0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        store();
        __syncthreads();
        if (chunk + 1 < nchunks) load(chunk + 1);
#pragma unroll
        for (int k0 = 0; k0 < KC; k0 += 4) {                   // (features at or past F are staged as zeros: they add +0.0)
            const double a0 = ar[k0], a1 = ar[16 * LDP + k0], b0 = br[k0], b1 = br[16 * LDP + k0];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    // the kernel function, THEN the mask: a row of zeros has k = coef0^3
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t i = i0 + wr * 32 + p * 16 + fk + 4 * g, j = j0 + wc * 32 + q * 16 + fc;
                const double t = gamma * acc[p][q][g] + coef0;
                const double k = (t * t) * t;
                const bool keep = i < M && j < N && !(skip && i == j);
                s += keep ? k : 0.0;
            }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        const double total = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        const int64_t B = gridDim.x;
        sums[(int64_t)a * B + b] = total;
        if (self && a != b) sums[(int64_t)b * B + a] = total;  // (self form: the matrix is square, B tiles a side)
    }
}

}  // namespace

extern "C" int pg_kid_tilesums_f64(const float* x, int64_t M, const float* y, int64_t N, int F, double gamma, double coef0, int skip_diagonal,
                                   double* sums, pg_stream_t stream)
{
    const int self = y == nullptr;
    if (self) N = M;
    if (!x || !sums || M < 1 || N < 1 || F < PG_KID_MIN_F || F > PG_KID_MAX_F || (F & 15) || (skip_diagonal && !self)) return PG_E_ARG;
    if (misaligned(x) || (y && misaligned(y)) || misaligned(sums, 8)) return PG_E_ALIGN;
    const int64_t A = (M + TILE - 1) / TILE, B = (N + TILE - 1) / TILE;
    if (A > 65535 || B > ((int64_t)1 << 30)) return PG_E_UNSUP;
    hipLaunchKernelGGL(kid_tile_kernel, dim3((unsigned)B, (unsigned)A), dim3(256), 0, (hipStream_t)stream, x, M, self ? x : y, N, F, gamma,
                       coef0, self, skip_diagonal ? 1 : 0, sums);
    return (int)hipGetLastError();
}
