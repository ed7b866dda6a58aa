// The front end of the kernels that read pieces as (N, S, 8) int16 id rows (pb_piece_features, pb_piece_keys, pb_piece_structure,
// pb_piece_harmony, pb_piece_texture): which rows of a piece are its notes, and the entry checks and launch grid that go with them.
//   A row is one 16-byte word of eight unsigned 16-bit ids. A piece ends at L, its first row with a special id (>= pad8[h]) in any
//   head (S if none); its notes are the rows first .. L - 1 with first = max(start[piece], 0), or 0 without start.
#pragma once
#include "pb_common.h"
#include <algorithm>

constexpr int PIECE_IDS = 1088;                // ids of a head stay below HEAD_MAX = 1088 (ops.py)
constexpr int PIECE_MAX_S = 1 << 20;           // the S limit of an entry that has none of its own
constexpr int PIECE_GRID = 1024;               // workgroups of a grid sweep at most

struct Pad8 { int v[8]; };

__device__ __forceinline__ int row_id(const uint4& r, int h) {
    const uint32_t w = h < 2 ? r.x : h < 4 ? r.y : h < 6 ? r.z : r.w;
    return (int)((w >> (16 * (h & 1))) & 0xffffu);
}
__device__ __forceinline__ bool row_is_special(const uint4& r, const Pad8& pad) {
    bool sp = false;
#pragma unroll
    for (int h = 0; h < 8; ++h) sp |= row_id(r, h) >= pad.v[h];      // unsigned 16 bits: a negative id ends the piece too
    return sp;
}

// L of the piece whose rows these are, for a workgroup of THREADS threads. s_L is the workgroup's LDS word: it holds S, and a barrier lies
// between that store and this call. A barrier lies behind the search as well: every thread returns the same L.
template <int THREADS>
__device__ __forceinline__ int first_special_row(const uint4* rows, int S, const Pad8& pad, int& s_L) {
    int mine = S;
    for (int r = threadIdx.x; r < S && mine == S; r += THREADS) if (row_is_special(rows[r], pad)) mine = r;
    if (mine < S) atomicMin(&s_L, mine);
    __syncthreads();
    return s_L;
}

__device__ __forceinline__ int first_row(const int32_t* start, int piece) { return start ? max(start[piece], 0) : 0; }

// The checks of the arguments every pb_piece_* entry takes, `who`; fills pad. max_S: the largest S of the entry; pad_why: why none of its
// pad8 may pass PIECE_IDS - 6. Returns the entry's error code (0: fine). With N = 0 there are no rows: ids16 may be NULL.
inline int check_pieces(const char* who, int max_S, const char* pad_why, const int16_t* ids16, const int32_t* start, const int32_t* pad8,
                        const int16_t* pitch_of, int32_t N, int32_t S, Pad8& pad) {
    PB_REQUIRE((N == 0 || ids16) && ((uintptr_t)ids16 % 16 == 0), "%s: ids16 must be a non-NULL 16-byte aligned pointer (rows of 8 int16)", who);
    PB_REQUIRE((uintptr_t)start % 4 == 0, "%s: start must be NULL or an int32 pointer", who);
    PB_REQUIRE(pad8, "%s: pad8 (8 host int32) is required", who);
    PB_REQUIRE(pitch_of && ((uintptr_t)pitch_of % 2 == 0), "%s: pitch_of must be a non-NULL int16 pointer", who);
    PB_REQUIRE(N >= 0 && N <= (1 << 24), "%s: N = %d out of range (0 .. 2^24)", who, (int)N);
    PB_REQUIRE(S >= 1 && S <= max_S, "%s: S = %d out of range (1 .. %d)", who, (int)S, max_S);
    for (int h = 0; h < 8; ++h) {
        PB_REQUIRE(pad8[h] >= 1 && pad8[h] <= PIECE_IDS - 6, "%s: pad8[%d] = %d out of range (1 .. %d: %s)", who, h, (int)pad8[h], PIECE_IDS - 6, pad_why);
        pad.v[h] = pad8[h];
    }
    return 0;
}

// the grid of a sweep over N pieces in which a workgroup takes at least rows_per_wg rows' worth of pieces
inline int piece_grid(int N, int S, int rows_per_wg) {
    const int per_wg = std::max(1, rows_per_wg / S);
    return std::min(PIECE_GRID, (N + per_wg - 1) / per_wg);
}
