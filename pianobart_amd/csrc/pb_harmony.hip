// K23: harmony of a piece: the pitch classes of its bars. Per piece, from the per-bar class histograms h_b[0..11] of its
// pitched notes: the pooled entropy sums of the windows of 1 and 4 bars, their keys (the diatonic set D_k that holds most of a histogram),
// and for the lags l = 1 .. 64 the sums I_H[l] = sum_b sum_c min(h_b[c], h_{b+l}[c]), T_H[l] = sum_b n_b + n_{b+l} and
// I_X[l] = sum_b max_t sum_c min(h_b[c], h_{b+l}[(c + t) % 12]), the same intersection up to transposition.
//   harmony_kernel   one workgroup per piece (grid sweep): 16 waves, or 4 where S <= 512, so that four short pieces share a CU and each
//                    other's waits (a piece is a chain of barriers and dependent loads; its arithmetic is small). A bar's histogram is
//                    six LDS words of two 16-bit counts each (a count is at most S <= 4096), indexed by bar id and built by 32-bit LDS
//                    adds of 1 << 16 (c & 1): no carry can cross.
//     counts   every note row: bar range (all notes), pitched or percussion, one LDS add per pitched note.
//     bars     one thread per bar: n_b and the piece's histogram g (summed over the wave by lane exchange, then 12 LDS adds per wave).
//     windows  w = 1, then w = 4: one thread per window: its histogram, n, X = TL[n] - sum_c TL[h[c]] from the host's int64 table (read
//              through L2: 13 reads per window), best / key, classes; then the key changes from the per-window keys kept in LDS.
//     T_H      needs no pairs: T[l] = 2 P - (the first l bars) - (the last l bars), 64 threads with at most 64 additions each.
//     pairs    the W x 64 bar pairs, the hot loop. A work item is (bar b, eight consecutive lags); a thread's eight lags never change
//              (the workgroup's size is a multiple of 8), so its 16 partial sums stay in registers. b's six words are loaded once per
//              item. A pair with an empty bar is skipped. With both bars' counts packed two to a word,
//                  sum_c min(a[c], b[c + t]) = (n_a + n_b - sum_c |a[c] - b[c + t]|) / 2     (exact: both sides of the same parity)
//              and a sum of absolute differences of packed 16-bit pairs is ONE instruction per word (v_sad_u16), so a transposition costs six
//              of them and a pair 72, plus 11 min for the smallest. The rotation is register naming: even t pairs word j of a with
//              word j + t / 2 of b, odd t with the same words of b shifted by one count (six v_perm_b32 per pair).
//              The partial sums of the eight lanes that share a lag group are added by lane exchange, then one LDS add per lag and wave.
// Integers only, no float anywhere; every sum is an integer add (registers, lane exchange, LDS atomics), whose result does not depend on the
// order: equal inputs and permuted rows give equal bytes. Every LDS index is a bar id below pad8[0] <= 1082, a bar index below W <= 1082,
// a column below 228 or a lag below 64; every table index is a count of notes of one piece, at most S <= 4096.
#include "pb_common.h"
#include "pb_api_internal.h"
#include "pb_pieces.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int HM_WIDE = 1024, HM_NARROW = 256, HM_NARROW_S = 512, HM_LAGS = 64, HM_COLS = 36 + 3 * HM_LAGS;
constexpr int HM_MAX_S = 4096, HM_IDS = PIECE_IDS, HM_WORDS = 6;   // the table and the 16-bit counts end at HM_MAX_S; six words per bar
constexpr int HM_ROWS_PER_WG = 256;                               // a workgroup takes at least this many rows' worth of pieces
constexpr int HM_GROUP = 8, HM_GROUPS = HM_LAGS / HM_GROUP;       // lags per work item of the pair loop
constexpr int C_G = 8, C_W1 = 20, C_W4 = 28, C_IH = 36, C_TH = C_IH + HM_LAGS, C_IX = C_TH + HM_LAGS;
static_assert(HM_WIDE % HM_GROUPS == 0 && HM_NARROW % HM_GROUPS == 0 && HM_GROUPS == 8, "a thread keeps its lag group; the lane exchange below is written for 8 groups");

typedef unsigned long long u64;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the six words of bar id `bar`
__device__ __forceinline__ void load_bar(const uint32_t* hist, int bar, uint32_t (&w)[HM_WORDS]) {
    const uint2* p = reinterpret_cast<const uint2*>(hist + bar * HM_WORDS);          // 24 bytes per bar: 8-byte aligned
    const uint2 a = p[0], b = p[1], c = p[2];
    w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y; w[4] = c.x; w[5] = c.y;
}
__device__ __forceinline__ void add_bar(const uint32_t* hist, int bar, int (&h)[12]) {
    uint32_t w[HM_WORDS];
    load_bar(hist, bar, w);
#pragma unroll
    for (int j = 0; j < HM_WORDS; ++j) { h[2 * j] += (int)(w[j] & 0xffffu); h[2 * j + 1] += (int)(w[j] >> 16); }
}

// best = max_k sum of h over D_k = k + {0, 2, 4, 5, 7, 9, 11}, key = the smallest k that attains it
__device__ __forceinline__ void key_of(const int (&h)[12], int& best, int& key) {
    best = -1; key = 0;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const int s = h[k] + h[(k + 2) % 12] + h[(k + 4) % 12] + h[(k + 5) % 12] + h[(k + 7) % 12] + h[(k + 9) % 12] + h[(k + 11) % 12];
        if (s > best) { best = s; key = k; }
    }
}

// one bar pair: sad[t] = sum_c |a[c] - b[(c + t) % 12]| over the packed words; returns the one of t = 0 and the smallest
__device__ __forceinline__ void pair_sads(const uint32_t (&A)[HM_WORDS], const uint32_t (&B)[HM_WORDS], uint32_t& sad0, uint32_t& sad_min) {
    uint32_t O[HM_WORDS];                                                               // b shifted by one count: O[j] = (b[2j + 1], b[2j + 2])
#pragma unroll
    for (int j = 0; j < HM_WORDS; ++j) O[j] = __builtin_amdgcn_alignbit(B[(j + 1) % HM_WORDS], B[j], 16);
#pragma unroll
    for (int t = 0; t < 12; ++t) {
        uint32_t s = 0u;
#pragma unroll
        for (int j = 0; j < HM_WORDS; ++j) s = __builtin_amdgcn_sad_u16(A[j], (t & 1) ? O[(j + t / 2) % HM_WORDS] : B[(j + t / 2) % HM_WORDS], s);
        if (t == 0) { sad0 = s; sad_min = s; } else sad_min = min(sad_min, s);
    }
}

// the windows of w bars: the eight values of a window block into row[base ..], the per-window keys into keyw (-1: empty)
template <int w, int HM_THREADS>
__device__ __forceinline__ void window_pass(const uint32_t* hist, const long long* __restrict__ TL, signed char* keyw, u64* row, int base, int b_lo, int W,
                                            int k_star, int tid) {
    const int nwin = W >= w ? W - w + 1 : 0;                                            // wave-uniform from here: the barriers are met by all
    int v_some = 0, v_n = 0, v_best = 0, v_agree = 0, v_cls = 0, v_chg = 0;
    long long v_x = 0;
    for (int b = tid; b < nwin; b += HM_THREADS) {
        int h[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < w; ++j) add_bar(hist, b_lo + b + j, h);
        int n = 0;
#pragma unroll
        for (int c = 0; c < 12; ++c) n += h[c];
        signed char k = -1;
        if (n > 0) {
            long long x = TL[n];                                                        // n and every h[c] count notes of one piece: <= S <= 4096
#pragma unroll
            for (int c = 0; c < 12; ++c) { x -= TL[h[c]]; v_cls += h[c] > 0; }
            int best, key;
            key_of(h, best, key);
            v_some += 1; v_n += n; v_x += x; v_best += best; v_agree += key == k_star;
            k = (signed char)key;
        }
        keyw[b] = k;
    }
    __syncthreads();
    for (int b = tid; b < nwin; b += HM_THREADS) {                                      // a change: the next non-empty window has another key
        const int k = keyw[b];
        if (k < 0) continue;
        int nx = b + 1;
        while (nx < nwin && keyw[nx] < 0) ++nx;
        if (nx < nwin && keyw[nx] != k) ++v_chg;
    }
    if ((tid & ~63) < nwin) {                                                           // waves that held a window
        const int some = wave_sum(v_some), n = wave_sum(v_n), best = wave_sum(v_best), agree = wave_sum(v_agree), chg = wave_sum(v_chg),
                  cls = wave_sum(v_cls);
        const long long x = wave_sum(v_x);
        if ((tid & 63) == 0 && some) {
            atomicAdd(&row[base + 1], (u64)some); atomicAdd(&row[base + 2], (u64)n); atomicAdd(&row[base + 3], (u64)x);
            atomicAdd(&row[base + 4], (u64)best); atomicAdd(&row[base + 5], (u64)agree); atomicAdd(&row[base + 6], (u64)chg);
            atomicAdd(&row[base + 7], (u64)cls);
        }
    }
    if (tid == 0) row[base] = (u64)nwin;
    __syncthreads();                                                                    // keyw is free again
}

template <int HM_THREADS>
__global__ __launch_bounds__(HM_THREADS) void harmony_kernel(const uint4* __restrict__ ids, const int32_t* __restrict__ start, const Pad8 pad,
                                                             const int16_t* __restrict__ pitch_of, const long long* __restrict__ TL,
                                                             long long* __restrict__ out, int N, int S) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[HM_IDS * HM_WORDS];           // by bar id: (h[0], h[1]), (h[2], h[3]), ..
    __shared__ int nbar[HM_IDS];                                                        // n_b by bar index
    __shared__ signed char keyw[HM_IDS];                                                // key of the window that starts at a bar index
    __shared__ u64 row[HM_COLS];                                                        // the output row; the sums are counted in place
    __shared__ int s_L, s_lo, s_hi;
    const int tid = threadIdx.x, lane = tid & 63;

    for (int i = tid; i < HM_IDS * HM_WORDS; i += HM_THREADS) hist[i] = 0u;             // once: a piece clears what it used
    for (int piece = blockIdx.x; piece < N; piece += gridDim.x) {
        const uint4* rows = ids + (long)piece * S;
        for (int i = tid; i < HM_COLS; i += HM_THREADS) row[i] = 0ull;
        if (tid == 0) { s_L = S; s_lo = INT_MAX; s_hi = -1; }
        __syncthreads();
        const int L = first_special_row<HM_THREADS>(rows, S, pad, s_L);
        const int first = first_row(start, piece);
        const int n = max(L - first, 0);                                                // notes: rows first .. L - 1, n <= S <= 4096

        // counts
        int lo = INT_MAX, hi = -1, pitched = 0;
        for (int i = tid; i < n; i += HM_THREADS) {
            const uint4 r = rows[first + i];
            const int bar = row_id(r, 0), m = pitch_of[row_id(r, 3)];                   // both ids below their pad8: the row is no special one
            lo = min(lo, bar); hi = max(hi, bar);
            if (m >= 0) { const int c = m % 12; atomicAdd(&hist[bar * HM_WORDS + (c >> 1)], 1u << (16 * (c & 1))); ++pitched; }
        }
        if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
        if ((tid & ~63) < n) { const int p = wave_sum(pitched); if (lane == 0 && p) atomicAdd(&row[2], (u64)p); }
        __syncthreads();
        const int b_lo = s_hi >= 0 ? s_lo : 0, W = s_hi >= 0 ? s_hi - b_lo + 1 : 0;     // b_lo + W <= pad8[0] <= 1082

        // bars: n_b and g
        if ((tid & ~63) < W) {
            int g[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int b = tid; b < W; b += HM_THREADS) {
                int h[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                add_bar(hist, b_lo + b, h);
                int nb = 0;
#pragma unroll
                for (int c = 0; c < 12; ++c) { nb += h[c]; g[c] += h[c]; }
                nbar[b] = nb;
            }
#pragma unroll
            for (int c = 0; c < 12; ++c) { const int s = wave_sum(g[c]); if (lane == 0 && s) atomicAdd(&row[C_G + c], (u64)s); }
        }
        __syncthreads();
        int g[12], sc, k_star;
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = (int)row[C_G + c];
        key_of(g, sc, k_star);                                                          // all zero (P = 0): key 0, best 0
        const int P = (int)row[2];

        window_pass<1, HM_THREADS>(hist, TL, keyw, row, C_W1, b_lo, W, k_star, tid);
        window_pass<4, HM_THREADS>(hist, TL, keyw, row, C_W4, b_lo, W, k_star, tid);

        // T_H
        if (tid < HM_LAGS) {
            const int l = tid + 1;
            int t = 0;
            if (l < W) {
                for (int b = 0; b < l; ++b) t += nbar[b] + nbar[W - 1 - b];
                t = 2 * P - t;
            }
            row[C_TH + tid] = (u64)t;
        }

        // pairs: item = (bar index, lag group), the group is tid % 8 throughout
        if ((tid & ~63) < W * HM_GROUPS) {
            const int q = tid & (HM_GROUPS - 1), l0 = q * HM_GROUP + 1;
            int acc_h[HM_GROUP], acc_x[HM_GROUP];
#pragma unroll
            for (int j = 0; j < HM_GROUP; ++j) { acc_h[j] = 0; acc_x[j] = 0; }
            for (int item = tid; item < W * HM_GROUPS; item += HM_THREADS) {
                const int b = item >> 3;
                if (b + l0 >= W) continue;
                const int na = nbar[b];
                if (na == 0) continue;
                uint32_t A[HM_WORDS];
                load_bar(hist, b_lo + b, A);
#pragma unroll
                for (int j = 0; j < HM_GROUP; ++j) {
                    const int bp = b + l0 + j;
                    if (bp < W) {
                        const int nb = nbar[bp];
                        if (nb != 0) {
                            uint32_t B[HM_WORDS], sad0, sad_min;
                            load_bar(hist, b_lo + bp, B);
                            pair_sads(A, B, sad0, sad_min);
                            acc_h[j] += (na + nb - (int)sad0) >> 1;
                            acc_x[j] += (na + nb - (int)sad_min) >> 1;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < HM_GROUP; ++j) {                                        // the eight lanes of a lag group: lane % 8
#pragma unroll
                for (int o = 32; o >= HM_GROUPS; o >>= 1) { acc_h[j] += __shfl_xor(acc_h[j], o); acc_x[j] += __shfl_xor(acc_x[j], o); }
                if (lane < HM_GROUPS && acc_x[j]) {                                     // I_X >= I_H
                    atomicAdd(&row[C_IH + l0 - 1 + j], (u64)acc_h[j]);
                    atomicAdd(&row[C_IX + l0 - 1 + j], (u64)acc_x[j]);
                }
            }
        }
        if (tid == 0) { row[0] = (u64)n; row[1] = (u64)W; row[3] = (u64)(n - P); row[4] = row[C_W1 + 1]; row[5] = (u64)k_star; row[6] = (u64)sc; }
        __syncthreads();
        for (int i = tid; i < HM_COLS; i += HM_THREADS) out[(long)piece * HM_COLS + i] = (long long)row[i];
        for (int i = tid; i < W * HM_WORDS; i += HM_THREADS) hist[b_lo * HM_WORDS + i] = 0u;      // only these bars were written
        __syncthreads();
    }
}

}  // namespace

extern "C" int pb_harmony_lags(void) { return HM_LAGS; }
extern "C" int pb_harmony_cols(void) { return HM_COLS; }

extern "C" int pb_piece_harmony(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, const int64_t* table,
                                int64_t* out, int32_t N, int32_t S, void* stream_) {
    Pad8 pad;
    if (int e = check_pieces("pb_piece_harmony", HM_MAX_S, "the per-bar counts are sized for it", ids16, start, pad8, pitch_of, N, S, pad)) return e;
    PB_REQUIRE(table && ((uintptr_t)table % 8 == 0), "pb_piece_harmony: table must be a non-NULL int64 pointer (4097 entries)");
    PB_REQUIRE((N == 0 || out) && ((uintptr_t)out % 8 == 0), "pb_piece_harmony: out must be a non-NULL int64 pointer");
    if (N == 0) return 0;
    const int grid = piece_grid(N, S, HM_ROWS_PER_WG);
    if (S <= HM_NARROW_S)
        hipLaunchKernelGGL(harmony_kernel<HM_NARROW>, dim3(grid), dim3(HM_NARROW), 0, (hipStream_t)stream_, (const uint4*)ids16, start, pad, pitch_of,
                           (const long long*)table, (long long*)out, (int)N, (int)S);
    else
        hipLaunchKernelGGL(harmony_kernel<HM_WIDE>, dim3(grid), dim3(HM_WIDE), 0, (hipStream_t)stream_, (const uint4*)ids16, start, pad, pitch_of,
                           (const long long*)table, (long long*)out, (int)N, (int)S);
    PB_LAUNCH_CHECK();
    return 0;
}
