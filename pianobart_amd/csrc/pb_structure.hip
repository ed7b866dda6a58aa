// K22: repetition structure of a piece: how much of a bar returns 1 .. 64 bars later. Per piece, for the onset sets
// O_b = {p} and the note sets N_b = {(p, f)} of its bars, the lag sums I_X[l] = sum_b |X_b ^ X_{b+l}| and T_X[l] = sum_b |X_b| + |X_{b+l}|.
//   structure_kernel   one workgroup of 16 waves per piece (grid sweep), the piece's notes in LDS as two words each:
//                        K = p << 11 | bar     (position above the bar: for two notes of one position, K_c - K_a IS the bar distance)
//                        F = the pitch field   (bit 31 is set later on the first note of its (bar, p))
//   The notes are cut into blocks of 64 in row order, and both passes work on TILES: a wave holds the 64 notes of one block in its lanes
//   and walks over the 64 notes of another block through a wave-uniform LDS address (a broadcast, four notes per 16-byte read). The
//   tiles of a pass are dealt round robin to the 16 waves. Every block knows the smallest and largest bar id it holds, and a tile whose
//   two bar ranges cannot meet is skipped: a piece in time order costs a band along the diagonal, not the square.
//     pass 1  tiles (A, J <= A), bar ranges overlapping: every note of A against the notes of earlier rows: is its (bar, p) there
//             already, is its (bar, p, f)? The answers are OR-ed into one 64-bit mask per block. A note whose (bar, p, f) is new is the
//             representative of that element of N_b, and of O_b too when its (bar, p) is new. Representatives count |O_b| and |N_b|
//             into per-bar counters; the other notes' K becomes NONE and matches nothing from then on.
//     pass 2  tiles (A, C) with some bar of C 1 .. 64 behind some bar of A: representative a against note c: x = K_c - K_a - 1 < 64
//             (unsigned) holds exactly when both are at one position and c lies 1 .. 64 bars behind a (positions differ by a multiple
//             of 2048, bars by less than 1082). Then I_N[x] counts where the pitch fields agree, I_O[x] where both are the first of
//             their (bar, p).
//     T       from the per-bar counters: the pairs (b, b + l) leave out the last l bars on one side and the first l on the other, so
//             T[l] = 2 total - (the first l bars) - (the last l bars): 128 threads, at most 64 additions each.
// Integers only; the counters and masks are LDS integer atomics (add, or, min, max), whose results do not depend on the order: equal
// inputs give equal bytes. Every LDS index is a row index below S <= 4096, a block index below 64, a bar id below pad8[0] <= 1082 or a
// lag below 64.
#include "pb_common.h"
#include "pb_api_internal.h"
#include "pb_pieces.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int ST_THREADS = 1024, ST_WAVES = ST_THREADS / 64, ST_LAGS = 64, ST_COLS = 8 + 4 * ST_LAGS;
constexpr int ST_MAX_S = 4096, ST_BLOCKS = ST_MAX_S / 64, ST_IDS = PIECE_IDS;      // the notes of a piece live in LDS
constexpr int ST_ROWS_PER_WG = 256;                                // a workgroup takes at least this many rows' worth of pieces
constexpr int C_IO = 8, C_TO = C_IO + ST_LAGS, C_IN = C_TO + ST_LAGS, C_TN = C_IN + ST_LAGS;
constexpr uint32_t NONE_C = 0xFFFFFFFFu;       // K of a note that represents nothing, read as c: K_c - K_a - 1 >= 2^32 - 2^22 - 2
constexpr uint32_t NONE_A = 0x80000000u;       // the same note (or no note) held as a: K_c - K_a - 1 >= 2^31 - 1 for every K_c
constexpr uint32_t FIRST_OF_ONSET = 0x80000000u, FIELD = 0x7FFu;

// pass 1, one earlier note of the tile: the lanes (of `later`: the notes in later rows than it) whose (bar, p) / (bar, p, f) it holds. The masks
// are wave-uniform: a compare writes its lane mask, and the accumulation is scalar.
__device__ __forceinline__ void seen(uint32_t kj, uint32_t fj, uint32_t ki, uint32_t fi, unsigned long long later, unsigned long long& mO,
                                     unsigned long long& mN) {
    const unsigned long long same = __ballot(kj == ki) & later;
    mO |= same;
    mN |= same & __ballot(fj == fi);
}

// pass 2, one note c against this lane's representative a
__device__ __forceinline__ void meet(uint32_t kc, uint32_t fc, uint32_t ka, uint32_t fa, int* row) {
    const uint32_t x = kc - ka - 1u;
    if (x < (uint32_t)ST_LAGS) {
        if (fa & fc & FIRST_OF_ONSET) atomicAdd(&row[C_IO + x], 1);
        if (((fa ^ fc) & FIELD) == 0u) atomicAdd(&row[C_IN + x], 1);
    }
}

__global__ __launch_bounds__(ST_THREADS) void structure_kernel(const uint4* __restrict__ ids, const int32_t* __restrict__ start, const Pad8 pad,
                                                               const int16_t* __restrict__ pitch_of, int32_t* __restrict__ out, int N, int S, int mode) {
    __shared__ __attribute__((aligned(16))) uint32_t K[ST_MAX_S], F[ST_MAX_S];
    __shared__ int cnt_o[ST_IDS], cnt_n[ST_IDS];   // |O_b| and |N_b| by bar id
    __shared__ int blk_lo[ST_BLOCKS], blk_hi[ST_BLOCKS];                     // the bar ids a block of 64 notes holds
    __shared__ unsigned long long dup_o[ST_BLOCKS], dup_n[ST_BLOCKS];        // bit l: note 64 blk + l has its (bar, p) / (bar, p, f) in an earlier row
    __shared__ int row[ST_COLS];                   // the output row; the lag sums are counted in place
    __shared__ int s_L, s_bar_lo, s_bar_hi;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int piece = blockIdx.x; piece < N; piece += gridDim.x) {
        const uint4* rows = ids + (long)piece * S;
        for (int i = tid; i < ST_COLS; i += ST_THREADS) row[i] = 0;
        for (int i = tid; i < ST_IDS; i += ST_THREADS) { cnt_o[i] = 0; cnt_n[i] = 0; }
        if (tid < ST_BLOCKS) { blk_lo[tid] = INT_MAX; blk_hi[tid] = -1; dup_o[tid] = 0ull; dup_n[tid] = 0ull; }
        if (tid == 0) { s_L = S; s_bar_lo = INT_MAX; s_bar_hi = -1; }
        __syncthreads();
        const int L = first_special_row<ST_THREADS>(rows, S, pad, s_L);
        const int first = first_row(start, piece);
        const int n = max(L - first, 0);                                     // notes: rows first .. L - 1, n <= S <= 4096
        const int n64 = (n + 63) & ~63, nb = n64 >> 6;                       // blocks of 64 notes, the last one filled with NONE

        for (int i = tid; i < n64; i += ST_THREADS) {                        // a wave loads whole blocks
            uint32_t k = NONE_C, f = 0u;
            if (i < n) {
                const uint4 r = rows[first + i];
                const int bar = row_id(r, 0), pit = row_id(r, 3);
                f = (uint32_t)pit;
                if (mode == 1) { const int m = pitch_of[pit]; f = m >= 0 ? (uint32_t)(m % 12) : 12u + (uint32_t)pit; }
                k = ((uint32_t)row_id(r, 1) << 11) | (uint32_t)bar;
                atomicMin(&blk_lo[i >> 6], bar);
                atomicMax(&blk_hi[i >> 6], bar);
            }
            K[i] = k;
            F[i] = f;
        }
        __syncthreads();
        if (tid < nb) { atomicMin(&s_bar_lo, blk_lo[tid]); atomicMax(&s_bar_hi, blk_hi[tid]); }

        // pass 1: tiles (A, J <= A) whose bar ranges overlap
        for (int t = wave; t < nb * nb; t += ST_WAVES) {
            const int A = t / nb, J = t - A * nb;                            // wave-uniform
            if (J > A || blk_lo[J] > blk_hi[A] || blk_lo[A] > blk_hi[J]) continue;
            const int i = A * 64 + lane;
            const uint32_t ki = i < n ? K[i] : NONE_A, fi = F[i];
            unsigned long long mO = 0ull, mN = 0ull;                        // lanes whose (bar, p) / (bar, p, f) an earlier row holds
            if (J < A) {                                                     // all of J lies in earlier rows
                for (int j = 0; j < 64; j += 4) {
                    const uint4 kj = *reinterpret_cast<const uint4*>(&K[J * 64 + j]), fj = *reinterpret_cast<const uint4*>(&F[J * 64 + j]);
                    seen(kj.x, fj.x, ki, fi, ~0ull, mO, mN);
                    seen(kj.y, fj.y, ki, fi, ~0ull, mO, mN);
                    seen(kj.z, fj.z, ki, fi, ~0ull, mO, mN);
                    seen(kj.w, fj.w, ki, fi, ~0ull, mO, mN);
                }
            } else {                                                         // the block itself: note j against the lanes behind it
                for (int j = 0; j < 64; j += 4) {
                    const uint4 kj = *reinterpret_cast<const uint4*>(&K[J * 64 + j]), fj = *reinterpret_cast<const uint4*>(&F[J * 64 + j]);
                    const unsigned long long later = ~0ull << j;             // lanes j .. 63
                    seen(kj.x, fj.x, ki, fi, later << 1, mO, mN);
                    seen(kj.y, fj.y, ki, fi, later << 2, mO, mN);
                    seen(kj.z, fj.z, ki, fi, later << 3, mO, mN);
                    seen(kj.w, fj.w, ki, fi, later << 4, mO, mN);               // j = 60: no lane is left
                }
            }
            if (lane == 0 && mO) { atomicOr(&dup_o[A], mO); atomicOr(&dup_n[A], mN); }      // mN is a subset of mO
        }
        __syncthreads();                                                     // every wave has read the K it needs before one is rewritten
        int tot_o = 0, tot_n = 0;
        for (int i = tid; i < n; i += ST_THREADS) {
            const bool dO = (dup_o[i >> 6] >> (i & 63)) & 1ull, dN = (dup_n[i >> 6] >> (i & 63)) & 1ull;
            const int bar = (int)(K[i] & 0x7FFu);
            if (!dN) { atomicAdd(&cnt_n[bar], 1); ++tot_n; } else K[i] = NONE_C;
            if (!dO) { atomicAdd(&cnt_o[bar], 1); ++tot_o; F[i] |= FIRST_OF_ONSET; }
        }
        if (tot_n) { atomicAdd(&row[2], tot_o); atomicAdd(&row[3], tot_n); }
        __syncthreads();

        // pass 2: tiles (A, C) in which some bar of C lies 1 .. 64 behind some bar of A
        for (int t = wave; t < nb * nb; t += ST_WAVES) {
            const int A = t / nb, C = t - A * nb;
            if (blk_hi[C] - blk_lo[A] < 1 || blk_lo[C] - blk_hi[A] > ST_LAGS) continue;
            const int a = A * 64 + lane;
            const uint32_t k = K[a], ka = k == NONE_C ? NONE_A : k, fa = F[a];
            if (__ballot(ka != NONE_A) == 0ull) continue;                    // a block without a representative
            for (int c = 0; c < 64; c += 4) {
                const uint4 kc = *reinterpret_cast<const uint4*>(&K[C * 64 + c]), fc = *reinterpret_cast<const uint4*>(&F[C * 64 + c]);
                meet(kc.x, fc.x, ka, fa, row);
                meet(kc.y, fc.y, ka, fa, row);
                meet(kc.z, fc.z, ka, fa, row);
                meet(kc.w, fc.w, ka, fa, row);
            }
        }
        __syncthreads();

        // T and the scalar columns
        const int b_lo = s_bar_lo, b_hi = s_bar_hi, W = b_hi >= 0 ? b_hi - b_lo + 1 : 0;
        if (tid < 2 * ST_LAGS) {
            const int l = (tid & (ST_LAGS - 1)) + 1;
            const int* cnt = tid < ST_LAGS ? cnt_o : cnt_n;
            int ends = 0;
            if (l < W) {
                for (int b = 0; b < l; ++b) ends += cnt[b_lo + b] + cnt[b_hi - b];
                ends = 2 * row[tid < ST_LAGS ? 2 : 3] - ends;
            }
            row[(tid < ST_LAGS ? C_TO : C_TN) + l - 1] = ends;
        }
        int bars = 0;
        for (int i = tid; i < ST_IDS; i += ST_THREADS) bars += cnt_o[i] > 0;
        if (bars) atomicAdd(&row[4], bars);
        if (tid == 0) { row[0] = n; row[1] = W; }
        __syncthreads();
        for (int i = tid; i < ST_COLS; i += ST_THREADS) out[(long)piece * ST_COLS + i] = row[i];
        __syncthreads();
    }
}

}  // namespace

extern "C" int pb_structure_lags(void) { return ST_LAGS; }
extern "C" int pb_structure_cols(void) { return ST_COLS; }

extern "C" int pb_piece_structure(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, int32_t* out, int32_t N,
                                  int32_t S, int32_t mode, void* stream_) {
    Pad8 pad;
    if (int e = check_pieces("pb_piece_structure", ST_MAX_S, "the note words' fields are sized for it", ids16, start, pad8, pitch_of, N, S, pad)) return e;
    PB_REQUIRE((N == 0 || out) && ((uintptr_t)out % 4 == 0), "pb_piece_structure: out must be a non-NULL int32 pointer");
    PB_REQUIRE(mode == 0 || mode == 1, "pb_piece_structure: mode = %d (0 = exact pitch, 1 = pitch class)", (int)mode);
    if (N == 0) return 0;
    hipLaunchKernelGGL(structure_kernel, dim3(piece_grid(N, S, ST_ROWS_PER_WG)), dim3(ST_THREADS), 0, (hipStream_t)stream_, (const uint4*)ids16, start, pad, pitch_of, out, (int)N, (int)S,
                       (int)mode);
    PB_LAUNCH_CHECK();
    return 0;
}
