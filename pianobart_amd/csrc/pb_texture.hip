// K24: texture of a piece: how many pitches sound at once, in absolute time. A bar's length is that of its time signature,
// a bar's start B(b) the sum of the lengths before it, a pitched note sounds over [t, e) with t = B(bar) + position and e = t + its
// duration in positions. Per piece: the polyphony histogram of the steps of [min t, max e), collisions and duplicates of one pitch, the
// distinct onsets with their chord sizes and the gaps between them, ties over the bar line and notes behind their bar's end.
//   texture_kernel   one workgroup per piece (grid sweep): 16 waves, or 4 where S <= 512 (pb_harmony.hip: a piece is a chain of barriers).
//     bars      every note row: the bar range, and per bar id an LDS atomicMin of (position << 11) | time signature.
//     time      one max-scan over the W bars carries the time signature over empty bars, one add-scan of the lengths gives B; a bar's LDS
//               word becomes (B << 11) | (len - 1).
//     notes     the pitched notes, compacted: a 64-bit key ((k << 21 | t) << 32) | e and a 32-bit key (t << 11) | k, padded to a power
//               of two with all-ones. P, D, tied and off-bar are counted here.
//     onsets    bitonic sort of the 32-bit keys. A new t is an onset (O, the inter-onset gap to the key before), a new key a distinct
//               (t, k); a segmented add-scan that restarts at every onset counts the distinct keys of an onset: its chord size.
//     pitches   bitonic sort of the 64-bit keys: by pitch, then onset, then end. The running maximum of (k << 21) | e is the largest end so far
//               within the pitch (a larger k outweighs every e). A (k, t) head (G) under an earlier end of its pitch is a collision (X);
//               any other head opens a merged interval, which closes at the running maximum of the last note before the next opening.
//     sweep     the openings and closings, at most 2 (G - X), as (time << 1) | opening, sorted; an add-scan of +1 / -1 gives the level
//               behind each event, and every gap of positive length to the next event adds its length to the level's bin, to U1, U2, A.
// Integers only; every sum is an integer add (registers, lane exchange, LDS atomics) and every order comes from a sort of whole keys, so
// equal inputs and permuted rows give equal bytes. Nothing is indexed by a time: every LDS index is a bar id below pad8[0] <= 1082, a slot
// below the piece's note count (<= S <= MAXN), an event slot below twice that, or a column below 64. Table values are clamped (a
// duration to 1 .. 4096, a bar length to 1 .. 1024), so times stay below 2^21 whatever the device tables hold.
#include "pb_common.h"
#include "pb_api_internal.h"
#include "pb_pieces.h"
#include <algorithm>
#include <climits>

namespace {

constexpr int TX_WIDE = 1024, TX_NARROW = 256, TX_NARROW_S = 512, TX_MAX_S = 4096, TX_COLS = 64;
constexpr int TX_ROWS_PER_WG = 256;                               // a workgroup takes at least this many rows' worth of pieces
constexpr int TX_MAX_DUR = 4096, TX_MAX_BAR = 1024;               // clamps of the table values
constexpr uint32_t TX_TIME = (1u << 21) - 1u, TX_NONE = 0xffffffffu;
constexpr int C_T = 3, C_U1 = 4, C_U2 = 5, C_A = 6, C_MAXC = 7, C_D = 8, C_X = 9, C_Y = 10, C_O = 11, C_TIED = 12, C_OFF = 13, C_G = 14;
constexpr int C_POLY = 16, POLY_TOP = 16, C_CHORD = 33, CHORD_TOP = 9, C_IOI = 42, IOI_TOP = 15;

typedef unsigned long long u64;

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct OpAdd { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; } };
struct OpMax { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return max(a, b); } };
// a count that restarts: bit 31 = a restart lies inside, bits 0 .. 30 = the count behind the last restart
struct OpSeg {
    __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const {
        return (b >> 31) ? b : ((a & 0x80000000u) | ((a & 0x7fffffffu) + (b & 0x7fffffffu)));
    }
};

// The exclusive scan over the workgroup's threads, in thread order, of one value each (0 is the identity of all three operators).
// Every thread calls it; s_w holds one word per wave; a barrier lies behind it, so s_w is free again.
template <int THREADS, class Op>
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, Op op, uint32_t* s_w) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)x, o);
        if (lane >= o) x = op(u, x);
    }
    if (lane == 63) s_w[wave] = x;
    uint32_t ex = (uint32_t)__shfl_up((int)x, 1);
    if (lane == 0) ex = 0u;
    __syncthreads();
    uint32_t before = 0u;
    for (int w = 0; w < wave; ++w) before = op(before, s_w[w]);
    __syncthreads();
    return op(before, ex);
}

// Bitonic sort, ascending, of a[0 .. n2) in LDS; n2 is a power of two. Barriers in front and behind.
template <int THREADS, typename T>
__device__ __forceinline__ void block_sort(T* a, int n2) {
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int idx = threadIdx.x; idx < (n2 >> 1); idx += THREADS) {
                const int i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), p = i | j;       // p < n2
                const T x = a[i], y = a[p];
                if ((x > y) == ((i & k) == 0)) { a[i] = y; a[p] = x; }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ int pow2_at_least(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

template <int THREADS, int MAXN>
__global__ __launch_bounds__(THREADS) void texture_kernel(const uint4* __restrict__ ids, const int32_t* __restrict__ start, const Pad8 pad,
                                                          const int16_t* __restrict__ pitch_of, const int32_t* __restrict__ dur_pos,
                                                          const int32_t* __restrict__ bar_pos, int32_t* __restrict__ out, int N, int S) {
    constexpr int PER = MAXN / THREADS;                                                 // sorted notes per thread at most
    static_assert(MAXN % THREADS == 0 && PER >= 1 && PER <= 8, "a thread keeps the events of its notes in registers");
    __shared__ uint32_t bars[PIECE_IDS];                                                // by bar id: the smallest (position, time signature), then (B, len - 1)
    __shared__ __attribute__((aligned(16))) u64 K[MAXN];                                // (k, t, e) of the pitched notes; later the 2 MAXN events
    __shared__ uint32_t R[MAXN];                                                        // (t, k) of the pitched notes; later the running maximum
    __shared__ int row[TX_COLS];                                                        // the output row; the sums are counted in place
    __shared__ uint32_t s_w[TX_WIDE / 64];
    __shared__ int s_L, s_lo, s_hi, s_cnt, s_ev;
    uint32_t* EV = reinterpret_cast<uint32_t*>(K);
    const int tid = threadIdx.x;

    for (int i = tid; i < PIECE_IDS; i += THREADS) bars[i] = TX_NONE;                   // once: a piece clears what it used
    for (int piece = blockIdx.x; piece < N; piece += gridDim.x) {
        const uint4* rows = ids + (long)piece * S;
        if (tid < TX_COLS) row[tid] = 0;
        if (tid == 0) { s_L = S; s_lo = INT_MAX; s_hi = -1; s_cnt = 0; s_ev = 0; }
        __syncthreads();
        const int L = first_special_row<THREADS>(rows, S, pad, s_L);
        const int first = first_row(start, piece);
        const int n = max(L - first, 0);                                                // notes: rows first .. L - 1, n <= S <= MAXN

        // bars
        int lo = INT_MAX, hi = -1;
        for (int i = tid; i < n; i += THREADS) {
            const uint4 r = rows[first + i];
            const int bar = row_id(r, 0);                                               // every id of a note row lies below its pad8 <= 1082
            lo = min(lo, bar); hi = max(hi, bar);
            atomicMin(&bars[bar], ((uint32_t)row_id(r, 1) << 11) | (uint32_t)row_id(r, 6));
        }
        if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
        __syncthreads();
        const int b_lo = s_hi >= 0 ? s_lo : 0, W = s_hi >= 0 ? s_hi - b_lo + 1 : 0;     // b_lo + W <= pad8[0] <= 1082

        // time: a thread owns the bar indices per * tid .. per * tid + per - 1
        {
            const int per = (W + THREADS - 1) / THREADS, b0 = tid * per;
            uint32_t last = 0u;                                                         // ((b + 1) << 11) | ts of my last bar with a note
            for (int c = 0; c < per; ++c) {
                const int b = b0 + c;
                if (b < W) { const uint32_t v = bars[b_lo + b]; if (v != TX_NONE) last = ((uint32_t)(b + 1) << 11) | (v & 2047u); }
            }
            uint32_t ts = block_exscan<THREADS>(last, OpMax(), s_w) & 2047u;            // of the last bar with a note before mine (bar 0 has one)
            uint32_t sum = 0u;
            for (int c = 0; c < per; ++c) {
                const int b = b0 + c;
                if (b < W) {
                    const uint32_t v = bars[b_lo + b];
                    if (v != TX_NONE) ts = v & 2047u;                                   // ts < pad8[6]: the length of bar_pos
                    const uint32_t len = (uint32_t)min(max(bar_pos[ts], 1), TX_MAX_BAR);
                    bars[b_lo + b] = len - 1u;
                    sum += len;
                }
            }
            uint32_t B = block_exscan<THREADS>(sum, OpAdd(), s_w);                      // < 1082 * 1024
            for (int c = 0; c < per; ++c) {
                const int b = b0 + c;
                if (b < W) { const uint32_t l1 = bars[b_lo + b]; bars[b_lo + b] = (B << 11) | l1; B += l1 + 1u; }
            }
        }
        __syncthreads();

        // notes
        {
            int pitched = 0, tied = 0, off = 0, dsum = 0;
            for (int i = tid; i < n; i += THREADS) {
                const uint4 r = rows[first + i];
                const int m = pitch_of[row_id(r, 3)];
                if (m < 0) continue;
                const uint32_t k = (uint32_t)min(m, 2047), bw = bars[row_id(r, 0)], B = bw >> 11, len = (bw & 2047u) + 1u;
                const uint32_t pos = (uint32_t)row_id(r, 1), t = B + pos, d = (uint32_t)min(max(dur_pos[row_id(r, 4)], 1), TX_MAX_DUR), e = t + d;
                const int slot = atomicAdd(&s_cnt, 1);                                  // < n <= MAXN
                K[slot] = ((u64)((k << 21) | t) << 32) | (u64)e;                         // t, e < 2^21: 1082 bars of 1024, a position, 4096
                R[slot] = (t << 11) | k;
                ++pitched; tied += e > B + len; off += pos >= len; dsum += (int)d;
            }
            pitched = wave_sum(pitched); tied = wave_sum(tied); off = wave_sum(off); dsum = wave_sum(dsum);
            if ((tid & 63) == 0 && pitched) { atomicAdd(&row[C_D], dsum); atomicAdd(&row[C_TIED], tied); atomicAdd(&row[C_OFF], off); }
        }
        __syncthreads();
        const int P = s_cnt;
        if (P > 0) {                                                                    // the same for every thread: the barriers inside are met by all
            const int n2 = pow2_at_least(P);
            for (int i = P + tid; i < n2; i += THREADS) { K[i] = ~0ull; R[i] = TX_NONE; }
            const int per = (P + THREADS - 1) / THREADS, i0 = tid * per;                // <= PER; a thread owns the sorted slots i0 .. i0 + per - 1

            // onsets
            block_sort<THREADS>(R, n2);
            {
                int onsets = 0;
                uint32_t agg = 0u;
                for (int c = 0; c < per; ++c) {
                    const int i = i0 + c;
                    if (i < P) {
                        const uint32_t key = R[i], prev = i > 0 ? R[i - 1] : TX_NONE;
                        const bool onset = i == 0 || (key >> 11) != (prev >> 11);
                        if (onset) {
                            ++onsets;
                            if (i > 0) atomicAdd(&row[C_IOI + min(31 - __clz((int)((key >> 11) - (prev >> 11))), IOI_TOP)], 1);
                        }
                        agg = OpSeg()(agg, (onset ? 0x80000000u : 0u) | (uint32_t)(i == 0 || key != prev));
                    }
                }
                uint32_t run = block_exscan<THREADS>(agg, OpSeg(), s_w);
                for (int c = 0; c < per; ++c) {
                    const int i = i0 + c;
                    if (i < P) {
                        const uint32_t key = R[i], prev = i > 0 ? R[i - 1] : TX_NONE;
                        const bool onset = i == 0 || (key >> 11) != (prev >> 11);
                        run = OpSeg()(run, (onset ? 0x80000000u : 0u) | (uint32_t)(i == 0 || key != prev));
                        if (i == P - 1 || (R[i + 1] >> 11) != (key >> 11))               // the onset's last note: its distinct keys are counted
                            atomicAdd(&row[C_CHORD + min((int)(run & 0x7fffffffu), CHORD_TOP) - 1], 1);
                    }
                }
                onsets = wave_sum(onsets);
                if ((tid & 63) == 0 && onsets) atomicAdd(&row[C_O], onsets);
            }

            // pitches
            block_sort<THREADS>(K, n2);                                                 // its first barrier: R is free
            {
                uint32_t agg = 0u;
                for (int c = 0; c < per; ++c) {
                    const int i = i0 + c;
                    if (i < P) { const u64 q = K[i]; agg = max(agg, ((uint32_t)(q >> 32) & ~TX_TIME) | (uint32_t)q); }
                }
                uint32_t run = block_exscan<THREADS>(agg, OpMax(), s_w);
                for (int c = 0; c < per; ++c) {
                    const int i = i0 + c;
                    if (i < P) { const u64 q = K[i]; run = max(run, ((uint32_t)(q >> 32) & ~TX_TIME) | (uint32_t)q); R[i] = run; }
                }
            }
            __syncthreads();
            uint32_t ev_open[PER], ev_close[PER];
            {
                int heads = 0, coll = 0;
#pragma unroll
                for (int c = 0; c < PER; ++c) {
                    const int i = i0 + c;
                    ev_open[c] = TX_NONE; ev_close[c] = TX_NONE;
                    if (c < per && i < P) {
                        const uint32_t kt = (uint32_t)(K[i] >> 32), k = kt >> 21, t = kt & TX_TIME, m = R[i];
                        if (i == 0 || kt != (uint32_t)(K[i - 1] >> 32)) {               // the head of a (k, t) group
                            ++heads;
                            const uint32_t mp = i > 0 ? R[i - 1] : 0u;
                            if (i > 0 && (mp >> 21) == k && (mp & TX_TIME) > t) ++coll; else ev_open[c] = (t << 1) | 1u;
                        }
                        bool closes = i == P - 1;
                        if (!closes) {
                            const uint32_t kt2 = (uint32_t)(K[i + 1] >> 32);
                            closes = kt2 != kt && ((kt2 >> 21) != k || (m & TX_TIME) <= (kt2 & TX_TIME));        // the next note opens an interval
                        }
                        if (closes) ev_close[c] = (m & TX_TIME) << 1;
                    }
                }
                heads = wave_sum(heads); coll = wave_sum(coll);
                if ((tid & 63) == 0 && heads) { atomicAdd(&row[C_G], heads); atomicAdd(&row[C_X], coll); }
            }
            __syncthreads();                                                            // K is read: the events take its place

            // sweep
#pragma unroll
            for (int c = 0; c < PER; ++c) {
                if (ev_open[c] != TX_NONE) EV[atomicAdd(&s_ev, 1)] = ev_open[c];        // at most one opening and one closing per note: < 2 MAXN
                if (ev_close[c] != TX_NONE) EV[atomicAdd(&s_ev, 1)] = ev_close[c];
            }
            __syncthreads();
            const int E = s_ev, e2 = pow2_at_least(E);                                  // E >= 2 and even
            for (int i = E + tid; i < e2; i += THREADS) EV[i] = TX_NONE;
            block_sort<THREADS>(EV, e2);
            {
                const int pere = (E + THREADS - 1) / THREADS, j0 = tid * pere;
                uint32_t agg = 0u;
                for (int c = 0; c < pere; ++c) {
                    const int j = j0 + c;
                    if (j < E) agg += (EV[j] & 1u) ? 1u : 0xffffffffu;
                }
                int level = (int)block_exscan<THREADS>(agg, OpAdd(), s_w);
                int u1 = 0, u2 = 0, area = 0, top = 0;
                for (int c = 0; c < pere; ++c) {
                    const int j = j0 + c;
                    if (j < E) {
                        const uint32_t ev = EV[j];
                        level += (ev & 1u) ? 1 : -1;
                        const int gap = j + 1 < E ? (int)((EV[j + 1] >> 1) - (ev >> 1)) : 0;
                        if (gap > 0) {
                            atomicAdd(&row[C_POLY + min(level, POLY_TOP)], gap);
                            u1 += level >= 1 ? gap : 0; u2 += level >= 2 ? gap : 0; area += level * gap; top = max(top, level);
                        }
                    }
                }
                u1 = wave_sum(u1); u2 = wave_sum(u2); area = wave_sum(area);
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) top = max(top, __shfl_xor(top, o));
                if ((tid & 63) == 0 && top) { atomicAdd(&row[C_U1], u1); atomicAdd(&row[C_U2], u2); atomicAdd(&row[C_A], area); atomicMax(&row[C_MAXC], top); }
                if (tid == 0) row[C_T] = (int)((EV[E - 1] >> 1) - (EV[0] >> 1));
            }
            __syncthreads();
        }
        if (tid == 0) { row[0] = n; row[1] = P; row[2] = W; row[C_Y] = P - row[C_G]; }
        __syncthreads();
        if (tid < TX_COLS) out[(long)piece * TX_COLS + tid] = row[tid];
        for (int i = tid; i < W; i += THREADS) bars[b_lo + i] = TX_NONE;                // only these bars were written
        __syncthreads();
    }
}

}  // namespace

extern "C" int pb_texture_cols(void) { return TX_COLS; }

extern "C" int pb_piece_texture(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, const int32_t* dur_pos,
                                const int32_t* bar_pos, int32_t* out, int32_t N, int32_t S, void* stream_) {
    Pad8 pad;
    if (int e = check_pieces("pb_piece_texture", TX_MAX_S, "a time signature and a pitch take 11 bits of a key", ids16, start, pad8, pitch_of, N, S, pad))
        return e;
    PB_REQUIRE(dur_pos && ((uintptr_t)dur_pos % 4 == 0), "pb_piece_texture: dur_pos must be a non-NULL int32 pointer (pad8[4] entries)");
    PB_REQUIRE(bar_pos && ((uintptr_t)bar_pos % 4 == 0), "pb_piece_texture: bar_pos must be a non-NULL int32 pointer (pad8[6] entries)");
    PB_REQUIRE((N == 0 || out) && ((uintptr_t)out % 4 == 0), "pb_piece_texture: out must be a non-NULL int32 pointer");
    if (N == 0) return 0;
    const int grid = piece_grid(N, S, TX_ROWS_PER_WG);
    if (S <= TX_NARROW_S)
        hipLaunchKernelGGL((texture_kernel<TX_NARROW, TX_NARROW_S>), dim3(grid), dim3(TX_NARROW), 0, (hipStream_t)stream_, (const uint4*)ids16, start, pad,
                           pitch_of, dur_pos, bar_pos, out, (int)N, (int)S);
    else
        hipLaunchKernelGGL((texture_kernel<TX_WIDE, TX_MAX_S>), dim3(grid), dim3(TX_WIDE), 0, (hipStream_t)stream_, (const uint4*)ids16, start, pad,
                           pitch_of, dur_pos, bar_pos, out, (int)N, (int)S);
    PB_LAUNCH_CHECK();
    return 0;
}
