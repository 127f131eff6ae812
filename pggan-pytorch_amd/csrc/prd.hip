// Precision / recall / density / coverage over k-NN balls (include/pggan_hip_prd.h): all-pairs exact squared L2
// distances between two sets of uint8 images of which only a reduction leaves the workgroup:
//   pg_prd_kth_u8  : per row, the k smallest distances of every block of PG_PRD_TILE columns (the diagonal excluded by index)
//   pg_prd_ball_u8 : per row and per column, the number of pairs with d2 <= the radius of the column / of the row
// One main loop, two epilogues.  Everything is integer arithmetic: exact and the same bits from run to run.
//
// Expansion (csrc/nn_search.hip): with x' = x - 128 (one XOR 0x80808080 per dword), d2 = |a'|^2 - 2 a'.b' + |b'|^2.  The cross term is a
// [rows x D] . [D x columns] product on v_mfma_i32_32x32x32_i8 (set a = A operand / rows, set b = B operand / columns); both norms are
// v_dot4_i32_i8 of the dwords a staging thread holds in registers on their way to LDS, every byte of the tile once.  No norm pass.
//
// Tile.  A workgroup of 4 waves owns TILE x TILE = 128 x 128 pairs and walks ALL of D (the epilogue needs the complete distance) in chunks
// of CHUNK = 128 bytes of every image; wave (wr, wc) owns the 64 x 64 quarter (wr, wc) as 2 x 2 MFMA tiles.  Both operands of a chunk
// (2 x 128 images x 128 bytes) are staged through LDS, already shifted, in fragment order and double buffered (2 x 32 KiB): thread
// (sq, sp) = (tid >> 3, tid & 7) loads the 16-byte piece sp of rows 32 t + sq, t = 0 .. 3, of both sets -- eight threads read the 128
// contiguous bytes of a row -- one chunk ahead of the MFMAs (two in the WIDE instantiation below), and stores piece sp = 4 h + i of row r of 32-row tile t at slot
// [side][t][i][32 h + (r ^ 2 sp)] (the XOR spreads the eight pieces of a row, which would share a bank, over the 16-byte slots of a bank
// row; a reading half-wave has h and i fixed, so it still reads 32 distinct consecutive slots).  Lane (c, h) = (lane & 31, lane >> 5)
// reads piece i of row c of a tile: lane half h element j is d = 64 h + 16 i + j on both sides, which is all the product needs.  The
// result register e of lane (c, h) is row (e & 3) + 8 (e >> 2) + 4 h against column c.  One barrier per chunk: the buffer a chunk's
// stores go to was last read before the previous barrier.
//
// Bounds.  |a' b'| <= 2^14 and a chunk adds 128 products to an element: the int32 accumulator holds WIDEN_CHUNKS = 512 chunks = 65536
// terms <= 2^30.  Images of more than 65536 bytes take the WIDE instantiation, which adds the tile into 64 int64 totals per lane every
// 512 chunks (64 int32 + 64 int64 accumulators: one wave per SIMD, accumulators in AGPRs; the resource report says no spill) and,
// having no second wave on its SIMD to hide a load behind, keeps the loads of TWO chunks in flight in two register sets; images
// up to 65536 bytes keep the int32 tile alone.  A thread's norm partial of a chunk is <= 16 * 2^14 per piece and is added to an int64.
// Tail.  A 16-byte piece at or past D is never loaded and is ZERO IN THE SHIFTED domain.  Rows >= Na and columns >= Nb read the last
// valid image instead; their results are neither written nor counted.
//
// Rasterisation (speed only; any bijection is correct): the launch is a 1-D grid; block ids that are equal modulo 8 (they share an
// XCD's L2) get a contiguous range of tile ids, and tile ids walk bands of BAND row tiles column by column, so that the workgroups
// resident on an XCD at one time share a few row panels and a few column panels.
//
// Epilogue kth.  Four passes of 32 rows (result registers 8 eh .. 8 eh + 7 of MFMA tile row x, both wave rows): the waves write the
// pass's distances into LDS as T[32][128] int64 (the staging buffers are free by then; column ^ 8 (row & 3) keeps writes and reads off
// shared banks), INT64_MAX for columns >= N and for the column whose GLOBAL index is the row's.  Eight threads per row then each
// keep the k smallest of 16 columns (q, q + 8, ...) sorted in registers, and k rounds of a minimum over the eight by (value, q) hand out
// the row's k smallest in ascending order, the winner dropping its head: one LDS transpose per wave and pass, no atomics.
// Epilogue ball.  Row counts: a ballot of the comparison over the wave, the popcount of the lane half that holds the row, both column
// tiles added; column counts: lane sums over the 32 result registers, the two halves added by one shuffle.  Waves combine in LDS
// counters (integer adds); then one global 32-bit atomic add per row and per column of the tile with a non-zero count.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pggan_hip_prd.h"
#include "u8l2.h"

namespace {

using namespace u8l2;                      // v4i, v16i, SHIFT, I64_MAX, shifted, sumsq16, load16, grid_for

constexpr int CHUNK = 128;                 // bytes of every image per step: 4 MFMAs of 32
constexpr int TILE = PG_PRD_TILE;          // rows and columns per workgroup
constexpr int WIDEN_CHUNKS = 512;          // 65536 terms per int32 accumulator lifetime (see Bounds)
constexpr int BUF = 2048;                  // 16-byte slots of one staging buffer: [side 2][tile 4][piece 4][lane 64]
constexpr int BAND = 8;                    // row tiles per rasterisation band
// the epilogues' LDS, in 8-byte words of the staging area: T [32][128] | norms a [128] | norms b [128] | radii a [128] | 4 x [128] int32
constexpr int LDS_NORM = 4096, LDS_RAD = LDS_NORM + 2 * TILE, LDS_CNT = LDS_RAD + TILE;
static_assert(TILE == 128, "the tile kernel is written for 128 x 128");

struct BallArgs {
    const long long* rad_a;
    const long long* rad_b;
    int* a_cnt;
    int* a_hit;
    int* b_cnt;
    int* b_hit;
};

// MODE 0: kth (a == b, Na == Nb, cand, k; TOPK >= k registers per scanning thread), MODE 1: ball
template <int MODE, bool WIDE, int TOPK>
__global__ __launch_bounds__(256) void prd_tile_kernel(const uint8_t* __restrict__ a, long long Na, const uint8_t* __restrict__ b,
                                                       long long Nb, long long D, int nchunks, int tiles_a, int tiles_b,
                                                       long long* __restrict__ cand, int k, BallArgs ball)
{
    __shared__ v4i lds[2 * BUF];                                             // 64 KiB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, h = lane >> 5, wr = wave >> 1, wc = wave & 1;

    // block id -> tile: ids equal modulo 8 take a contiguous range (bijective for any grid), ranges walk bands column by column
    int ta, tb;
    {
        const int nwg = (int)gridDim.x, bid = (int)blockIdx.x;
        const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
        const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
        const int per_band = BAND * tiles_b;
        const int band = id / per_band, rem = id % per_band;
        const int rows = tiles_a - band * BAND < BAND ? tiles_a - band * BAND : BAND;
        ta = band * BAND + rem % rows;
        tb = rem / rows;
    }
    const long long row0 = (long long)ta * TILE, col0 = (long long)tb * TILE;

    // staging: thread -> (row sq of every 32-row tile, 16-byte piece sp of the chunk)
    const int sq = tid >> 3, sp = tid & 7;
    const uint8_t* pa[4];
    const uint8_t* pb[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const long long ra = row0 + 32 * t + sq < Na ? row0 + 32 * t + sq : Na - 1;
        const long long rb = col0 + 32 * t + sq < Nb ? col0 + 32 * t + sq : Nb - 1;
        pa[t] = a + ra * D + 16 * sp;
        pb[t] = b + rb * D + 16 * sp;
    }
    const int wslot = (sp & 3) * 64 + (sp >> 2) * 32 + (sq ^ (sp << 1));   // piece sp = 4 h + i of row sq -> [i][32 h + (sq ^ 2 sp)]

    v16i acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[x][y][e] = 0;
    long long tot[WIDE ? 2 : 1][WIDE ? 2 : 1][WIDE ? 16 : 1];
    if (WIDE) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 2; ++y)
#pragma unroll
                for (int e = 0; e < 16; ++e) tot[WIDE ? x : 0][WIDE ? y : 0][WIDE ? e : 0] = 0;
    }
    long long sna[4] = {0, 0, 0, 0}, snb[4] = {0, 0, 0, 0};

    // the three phases of a chunk.  fetch: 2 x 4 global loads of 16 bytes into a register set; stage: a register set -> one LDS buffer,
    // shifted, its norm partials on the way; compute: the 16 MFMAs of this wave from one LDS buffer
    auto fetch = [&](uint4 (&ga)[4], uint4 (&gb)[4], int chunk) {
        const long long k0 = (long long)chunk * CHUNK;
        const bool valid = k0 + 16 * sp < D;
#pragma unroll
        for (int t = 0; t < 4; ++t) { ga[t] = load16(pa[t] + k0, valid); gb[t] = load16(pb[t] + k0, valid); }
    };
    auto stage = [&](const uint4 (&ga)[4], const uint4 (&gb)[4], int buf) {
        v4i* dst = lds + buf * BUF;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const v4i va = shifted(ga[t]), vb = shifted(gb[t]);
            dst[t * 256 + wslot] = va;
            dst[1024 + t * 256 + wslot] = vb;
            sna[t] += sumsq16(va, 0);
            snb[t] += sumsq16(vb, 0);
        }
    };
    auto compute = [&](int j) {
        const v4i* cur = lds + (j & 1) * BUF;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rs = i * 64 + h * 32 + (c ^ ((4 * h + i) << 1));
            const v4i a0 = cur[(2 * wr) * 256 + rs], a1 = cur[(2 * wr + 1) * 256 + rs];
            const v4i b0 = cur[1024 + (2 * wc) * 256 + rs], b1 = cur[1024 + (2 * wc + 1) * 256 + rs];
            acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (WIDE && (j % WIDEN_CHUNKS) == WIDEN_CHUNKS - 1) {
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        tot[WIDE ? x : 0][WIDE ? y : 0][WIDE ? e : 0] += acc[x][y][e];
                        acc[x][y][e] = 0;
                    }
        }
    };

    uint4 ga0[4], gb0[4];
    fetch(ga0, gb0, 0);
    if (!WIDE) {
        // loads one chunk ahead of the MFMAs: two waves per SIMD hide the rest
        stage(ga0, gb0, 0);
        __syncthreads();
        for (int j = 0; j < nchunks; ++j) {
            const bool more = j + 1 < nchunks;
            if (more) fetch(ga0, gb0, j + 1);
            compute(j);
            if (more) stage(ga0, gb0, (j + 1) & 1);
            __syncthreads();
        }
    } else {
        // one wave per SIMD: loads TWO chunks ahead, even chunks through register set 0 and odd ones through set 1 (the loop is
        // unrolled by two so that the sets are named at compile time); chunk j + 1 is staged while chunks j + 2 and j + 3 are in flight
        uint4 ga1[4], gb1[4];
        if (1 < nchunks) fetch(ga1, gb1, 1);
        stage(ga0, gb0, 0);
        if (2 < nchunks) fetch(ga0, gb0, 2);
        __syncthreads();
        for (int j = 0; j < nchunks; j += 2) {
            compute(j);
            if (j + 1 < nchunks) stage(ga1, gb1, 1);
            if (j + 3 < nchunks) fetch(ga1, gb1, j + 3);
            __syncthreads();
            if (j + 1 < nchunks) {
                compute(j + 1);
                if (j + 2 < nchunks) stage(ga0, gb0, 0);
                if (j + 4 < nchunks) fetch(ga0, gb0, j + 4);
                __syncthreads();
            }
        }
    }

    // ---- epilogues: the staging buffers are free (every wave is past the last barrier of the loop)
    long long* w64 = reinterpret_cast<long long*>(lds);
    long long* nrm = w64 + LDS_NORM;                                         // [0, 128): rows of the tile, [128, 256): columns
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        long long va = sna[t], vb = snb[t];
#pragma unroll
        for (int off = 1; off < 8; off <<= 1) { va += __shfl_xor(va, off); vb += __shfl_xor(vb, off); }
        if (sp == 0) { nrm[32 * t + sq] = va; nrm[TILE + 32 * t + sq] = vb; }
    }
    // the cross term of result register e of MFMA tile (x, y), complete
#define PRD_CROSS(x, y, e) ((WIDE ? tot[WIDE ? (x) : 0][WIDE ? (y) : 0][WIDE ? (e) : 0] : 0LL) + (long long)acc[x][y][e])

    if (MODE == 0) {
        __syncthreads();
        long long* T = w64;
        long long nbv[2];
        long long gcol[2];
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            nbv[y] = nrm[TILE + 64 * wc + 32 * y + c];
            gcol[y] = col0 + 64 * wc + 32 * y + c;
        }
        const int srow = tid >> 3, q = tid & 7;                              // scanning: row of the pass, column residue
#pragma unroll
        for (int x = 0; x < 2; ++x) {
#pragma unroll
            for (int eh = 0; eh < 2; ++eh) {
#pragma unroll
                for (int e8 = 0; e8 < 8; ++e8) {
                    const int e = 8 * eh + e8;
                    const int r16 = (e8 & 3) + 8 * (e8 >> 2) + 4 * h;        // row within the pass's 16 of this wave row
                    const int R = 64 * wr + 32 * x + 16 * eh + r16;          // row of the tile
                    const int lrow = 16 * wr + r16;
                    const long long grow = row0 + R, na = nrm[R];
#pragma unroll
                    for (int y = 0; y < 2; ++y) {
                        const long long v = na + nbv[y] - 2 * PRD_CROSS(x, y, e);
                        const int C = 64 * wc + 32 * y + c;
                        T[lrow * TILE + (C ^ ((lrow & 3) << 3))] = (gcol[y] < Nb && gcol[y] != grow) ? v : I64_MAX;
                    }
                }
                __syncthreads();
                long long best[TOPK];
#pragma unroll
                for (int j = 0; j < TOPK; ++j) best[j] = I64_MAX;
#pragma unroll 4
                for (int j = 0; j < TILE / 8; ++j) {
                    const long long v = T[srow * TILE + ((8 * j + q) ^ ((srow & 3) << 3))];
                    if (v < best[TOPK - 1]) {
#pragma unroll
                        for (int i = TOPK - 1; i >= 0; --i) {
                            const bool above = i > 0 && v < best[i > 0 ? i - 1 : 0];       // the new value goes further down
                            if (above) best[i] = best[i > 0 ? i - 1 : 0];
                            else if (v < best[i]) best[i] = v;
                        }
                    }
                }
                const long long grow = row0 + 64 * (srow >> 4) + 32 * x + 16 * eh + (srow & 15);
                for (int round = 0; round < k; ++round) {
                    long long bv = best[0];
                    int bq = q;
#pragma unroll
                    for (int off = 1; off < 8; off <<= 1) {
                        const long long ov = __shfl_xor(bv, off);
                        const int oq = __shfl_xor(bq, off);
                        if (ov < bv || (ov == bv && oq < bq)) { bv = ov; bq = oq; }
                    }
                    if (bq == q) {                                           // the one winner of the eight drops its head
#pragma unroll
                        for (int i = 0; i < TOPK - 1; ++i) best[i] = best[i + 1];
                        best[TOPK - 1] = I64_MAX;
                    }
                    if (q == 0 && grow < Na) cand[(grow * tiles_b + tb) * k + round] = bv;
                }
                __syncthreads();                                             // T is rewritten by the next pass
            }
        }
    } else {
        long long* rad = w64 + LDS_RAD;
        int* cnt = reinterpret_cast<int*>(w64 + LDS_CNT);                    // a_cnt | a_hit | b_hit | b_cnt of the tile, [128] each
        const bool use_a = ball.rad_a != nullptr, use_b = ball.rad_b != nullptr;
        if (tid < TILE) rad[tid] = use_a ? ball.rad_a[row0 + tid < Na ? row0 + tid : Na - 1] : 0;
        cnt[tid] = 0;
        cnt[256 + tid] = 0;
        __syncthreads();
        long long nbv[2], rbv[2];
        bool cvalid[2];
        int col_b[2] = {0, 0}, col_a[2] = {0, 0};
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int C = 64 * wc + 32 * y + c;
            const long long g = col0 + C;
            nbv[y] = nrm[TILE + C];
            cvalid[y] = g < Nb;
            rbv[y] = use_b ? ball.rad_b[g < Nb ? g : Nb - 1] : 0;
        }
#pragma unroll
        for (int x = 0; x < 2; ++x) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int R = 64 * wr + 32 * x + (e & 3) + 8 * (e >> 2) + 4 * h;
                const bool rvalid = row0 + R < Na;
                const long long na = nrm[R], ra = rad[R];
                int row_b = 0, row_a = 0;
#pragma unroll
                for (int y = 0; y < 2; ++y) {
                    const long long v = na + nbv[y] - 2 * PRD_CROSS(x, y, e);
                    const bool ok = rvalid && cvalid[y];
                    if (use_b) {
                        const bool in = ok && v <= rbv[y];
                        col_b[y] += in ? 1 : 0;
                        row_b += __popc((unsigned)(__ballot(in) >> (32 * h)));
                    }
                    if (use_a) {
                        const bool in = ok && v <= ra;
                        col_a[y] += in ? 1 : 0;
                        row_a += __popc((unsigned)(__ballot(in) >> (32 * h)));
                    }
                }
                if (c == 0) {                                                // one lane per row of the wave; the other wave column adds its own
                    if (row_b) atomicAdd(&cnt[R], row_b);
                    if (row_a) atomicAdd(&cnt[TILE + R], row_a);
                }
            }
        }
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const int C = 64 * wc + 32 * y + c;
            const int sb = col_b[y] + __shfl_xor(col_b[y], 32), sa = col_a[y] + __shfl_xor(col_a[y], 32);
            if (h == 0) {
                if (sb) atomicAdd(&cnt[2 * TILE + C], sb);
                if (sa) atomicAdd(&cnt[3 * TILE + C], sa);
            }
        }
        __syncthreads();
        if (tid < TILE) {
            const long long g = row0 + tid;
            if (g < Na) {
                if (use_b && cnt[tid]) atomicAdd(ball.a_cnt + g, cnt[tid]);
                if (use_a && cnt[TILE + tid]) atomicAdd(ball.a_hit + g, cnt[TILE + tid]);
            }
        } else {
            const int C = tid - TILE;
            const long long g = col0 + C;
            if (g < Nb) {
                if (use_b && cnt[2 * TILE + C]) atomicAdd(ball.b_hit + g, cnt[2 * TILE + C]);
                if (use_a && cnt[3 * TILE + C]) atomicAdd(ball.b_cnt + g, cnt[3 * TILE + C]);
            }
        }
    }
#undef PRD_CROSS
}

// tiles per side, chunks and the 1-D grid of a launch; false: outside what the kernel's int indices hold
inline bool geometry(int64_t Na, int64_t Nb, int64_t D, long long* tiles_a, long long* tiles_b, long long* nchunks)
{
    *tiles_a = (Na + TILE - 1) / TILE;
    *tiles_b = (Nb + TILE - 1) / TILE;
    *nchunks = (D + CHUNK - 1) / CHUNK;
    return *tiles_a <= 0x7fffffffLL / BAND && *tiles_b <= 0x7fffffffLL / BAND && *tiles_a * *tiles_b <= 0x7fffffffLL / BAND
        && *nchunks <= 0x7fffffffLL;
}

template <int MODE, int TOPK>
void launch(bool wide, unsigned grid, hipStream_t s, const uint8_t* a, long long Na, const uint8_t* b, long long Nb, long long D,
            int nchunks, int tiles_a, int tiles_b, long long* cand, int k, const BallArgs& ball)
{
    if (wide)
        hipLaunchKernelGGL((prd_tile_kernel<MODE, true, TOPK>), dim3(grid), dim3(256), 0, s, a, Na, b, Nb, D, nchunks, tiles_a, tiles_b,
                           cand, k, ball);
    else
        hipLaunchKernelGGL((prd_tile_kernel<MODE, false, TOPK>), dim3(grid), dim3(256), 0, s, a, Na, b, Nb, D, nchunks, tiles_a, tiles_b,
                           cand, k, ball);
}

}  // namespace

extern "C" int pg_prd_kth_u8(const uint8_t* x, int64_t N, int64_t D, int k, int64_t* cand, pg_stream_t stream)
{
    if (!x || !cand || D <= 0 || k < 1 || k > PG_NN_MAX_TOPK || N <= k) return PG_E_ARG;
    if (D % 16 || (uintptr_t)x % 16 || (uintptr_t)cand % 8) return PG_E_ALIGN;
    long long tiles, tiles_b, nchunks;
    if (!geometry(N, N, D, &tiles, &tiles_b, &nchunks)) return PG_E_UNSUP;
    const bool wide = nchunks > WIDEN_CHUNKS;
    const unsigned grid = (unsigned)(tiles * tiles);
    const BallArgs none = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    long long* out = reinterpret_cast<long long*>(cand);
    const hipStream_t s = (hipStream_t)stream;
    if (k == 1) launch<0, 1>(wide, grid, s, x, N, x, N, D, (int)nchunks, (int)tiles, (int)tiles, out, k, none);
    else if (k <= 4) launch<0, 4>(wide, grid, s, x, N, x, N, D, (int)nchunks, (int)tiles, (int)tiles, out, k, none);
    else launch<0, 16>(wide, grid, s, x, N, x, N, D, (int)nchunks, (int)tiles, (int)tiles, out, k, none);
    return (int)hipGetLastError();
}

extern "C" int pg_prd_ball_u8(const uint8_t* a, int64_t Na, const uint8_t* b, int64_t Nb, int64_t D, const int64_t* rad_a,
                              const int64_t* rad_b, int* a_cnt, int* a_hit, int* b_cnt, int* b_hit, pg_stream_t stream)
{
    if (!a || !b || Na <= 0 || Nb <= 0 || Na > 0x7fffffffLL || Nb > 0x7fffffffLL || D <= 0 || (!rad_a && !rad_b)) return PG_E_ARG;
    if ((rad_b && (!a_cnt || !b_hit)) || (rad_a && (!b_cnt || !a_hit))) return PG_E_ARG;
    if (D % 16 || (uintptr_t)a % 16 || (uintptr_t)b % 16 || (uintptr_t)rad_a % 8 || (uintptr_t)rad_b % 8) return PG_E_ALIGN;
    if ((rad_b && ((uintptr_t)a_cnt % 4 || (uintptr_t)b_hit % 4)) || (rad_a && ((uintptr_t)b_cnt % 4 || (uintptr_t)a_hit % 4))) return PG_E_ALIGN;
    long long tiles_a, tiles_b, nchunks;
    if (!geometry(Na, Nb, D, &tiles_a, &tiles_b, &nchunks)) return PG_E_UNSUP;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t err = hipSuccess;
    if (rad_b) {
        err = hipMemsetAsync(a_cnt, 0, (size_t)Na * sizeof(int), s);
        if (err == hipSuccess) err = hipMemsetAsync(b_hit, 0, (size_t)Nb * sizeof(int), s);
    }
    if (rad_a && err == hipSuccess) {
        err = hipMemsetAsync(b_cnt, 0, (size_t)Nb * sizeof(int), s);
        if (err == hipSuccess) err = hipMemsetAsync(a_hit, 0, (size_t)Na * sizeof(int), s);
    }
    if (err != hipSuccess) return (int)err;
    const BallArgs ball = {reinterpret_cast<const long long*>(rad_a), reinterpret_cast<const long long*>(rad_b), a_cnt, a_hit, b_cnt, b_hit};
    launch<1, 1>(nchunks > WIDEN_CHUNKS, (unsigned)(tiles_a * tiles_b), s, a, Na, b, Nb, D, (int)nchunks, (int)tiles_a, (int)tiles_b,
                 nullptr, 0, ball);
    return (int)hipGetLastError();
}
