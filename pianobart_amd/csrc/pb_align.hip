// K21: copy detection that survives edits: Smith-Waterman local alignment, linear gap penalty, of a generated piece's
// keys with every corpus piece's keys. A cell holds P = H << 12 | (4095 - start): the score of the best alignment that ends there and
// the A index of its first matched key; among alignments of equal score the integer maximum keeps the smallest start.
//   s       = A[p] == B[q] ? +match : -mismatch                    (a value with bit 31 set matches nothing)
//   d       = max(P(p - 1, q - 1), 4095 - p) + (s << 12)
//   r       = max(d, P(p - 1, q) - (gap << 12), P(p, q - 1) - (gap << 12))
//   P(p, q) = r >= 4096 ? r : 0
// align_kernel: one workgroup per (generated piece, tile of AL_TILE corpus pieces), as runs_kernel; each of its four waves takes whole
// pairs of the tile. The A row lies in LDS once per workgroup, with AL_PAD = 63 "no key" entries in front and 64 behind. A wave runs the
// table as an anti-diagonal wavefront over blocks of AL_BLOCK = 64 AL_C columns of B: lane l keeps AL_C consecutive columns in
// registers and computes row p = t - l of them at step t, so every lane makes the same Ka + 63 steps per block and a lane outside the
// rectangle reads a key that matches nothing: no bounds test, no data-dependent trip count. The right-most value of lane l is the left
// neighbour of lane l + 1 one step later (__shfl_up) and its diagonal neighbour the step after. Lane 63 writes the block's last column
// to LDS (Ka ints per wave), lane 0 reads it back as the left neighbour of the next block: row t is read at step t - 1 (a step ahead,
// as the A key is) and rewritten at step t + 63, so the column is updated in place. Cells outside the rectangle never match: they are
// never recorded, and they feed only cells further right or further down, which are outside too.
// Only match cells are recorded. Every output is an integer maximum (LDS and global atomic max, vector atomics): it depends on no order
// of lanes, waves, workgroups or chunks, and equal inputs give equal bytes.
#include "pb_common.h"
#include "pb_api_internal.h"
#include <algorithm>

namespace {

constexpr uint32_t NO_KEY = 0xFFFFFFFFu;        // in the LDS image of A: matches nothing
constexpr uint32_t STOP = 0xFFFFFFFEu;          // in the registers that hold B: matches nothing, NO_KEY included

constexpr int AL_THREADS = 256, AL_WAVES = AL_THREADS / 64, AL_TILE = 32, AL_MAX_S = 4096;
constexpr int AL_C = 4, AL_BLOCK = 64 * AL_C, AL_PAD = 63;
constexpr int AL_ONE = 4096;                    // H = 1 in a packed cell

// entries of the padded image of the A row (one more behind than a step reads: the next step's key is fetched ahead), a multiple of 2
__host__ __device__ constexpr int al_image(int Sa) { return (Sa + 2 * AL_PAD + 2) & ~1; }

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// dynamic LDS: ax[al_image(Sa)] (the padded A row), ae[Sa] (the align_end row of this workgroup), then, where Sb > AL_BLOCK, edge[AL_WAVES][Sa]
// (the last column of a wave's previous block)
__global__ __launch_bounds__(AL_THREADS) void align_kernel(const uint32_t* __restrict__ A, const int32_t* __restrict__ alen, int Sa,
                                                           const uint32_t* __restrict__ B, const int32_t* __restrict__ blen, int M, int Sb, int tiles,
                                                           int match12, int mismatch12, int gap12, int thr, int exclude_self, int j_base,
                                                           int32_t* __restrict__ score, int32_t* __restrict__ align_end,
                                                           unsigned long long* __restrict__ best) {
    extern __shared__ __attribute__((aligned(16))) int lds[];
    __shared__ int s_h[AL_TILE];
    uint32_t* ax = reinterpret_cast<uint32_t*>(lds);
    int* ae = lds + al_image(Sa);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* edge = ae + Sa + wave * Sa;                                // touched only where Sb > AL_BLOCK: the host sized the LDS for it
    const int i = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * AL_TILE;
    const int nj = min(AL_TILE, M - j0);
    const int Ka = min(max(alen[i], 0), Sa);
    const uint32_t* __restrict__ a_row = A + (long)i * Sa;

    for (int x = tid; x < Ka + 2 * AL_PAD + 1; x += AL_THREADS) {   // Ka + 127 <= al_image(Sa)
        const int p = x - AL_PAD;
        uint32_t v = NO_KEY;
        if (p >= 0 && p < Ka) { v = a_row[p]; if (v >> 31) v = NO_KEY; }
        ax[x] = v;
    }
    for (int p = tid; p < Ka; p += AL_THREADS) ae[p] = 0;
    if (tid < AL_TILE) s_h[tid] = 0;
    __syncthreads();

    for (int jl = wave; jl < nj; jl += AL_WAVES) {                  // a wave owns its pairs: no barrier in here
        const int j = j0 + jl;
        const int Kb = min(max(blen[j], 0), Sb);
        if (Ka == 0 || Kb == 0 || (exclude_self && j + j_base == i)) continue;      // wave-uniform
        const uint32_t* __restrict__ b_row = B + (long)j * Sb;
        const int steps = Ka + 63;
        int smax = 0;
        for (int qb = 0; qb < Kb; qb += AL_BLOCK) {
            uint32_t b[AL_C];
#pragma unroll
            for (int c = 0; c < AL_C; ++c) {
                const int q = qb + lane * AL_C + c;
                uint32_t v = STOP;
                if (q < Kb) { v = b_row[q]; if (v >> 31) v = STOP; }
                b[c] = v;
            }
            const bool first = qb == 0, more = qb + AL_BLOCK < Kb;
            int hg[AL_C], h[AL_C];                                  // row p - 1 of my columns: P - gap, and P
#pragma unroll
            for (int c = 0; c < AL_C; ++c) { hg[c] = -gap12; h[c] = 0; }
            int left = 0, diag = 0;                                 // P(p, q0 - 1) and P(p - 1, q0 - 1), q0 my first column
            const uint32_t* ap = ax + AL_PAD - lane;                // ap[t] = A[t - lane]; entries 0 .. Ka + 126 are read
            uint32_t a_next = ap[0];
            int e_next = (!first && lane == 0) ? edge[0] : 0;       // Ka >= 1
            for (int t = 0; t < steps; ++t) {
                const uint32_t a = a_next;
                const int p = t - lane;
                if (lane == 0) left = e_next;                       // lanes 1 .. 63 got theirs from the shuffle of the step before
                a_next = ap[t + 1];                                 // t + 1 - lane + 63 <= Ka + 126
                if (!first && lane == 0 && t + 1 < Ka) e_next = edge[t + 1]; else e_next = 0;
                const int base = 4095 - p;
                int e[AL_C], r[AL_C];
                bool eq[AL_C];
#pragma unroll
                for (int c = 0; c < AL_C; ++c) {                    // what does not wait for the left neighbour
                    eq[c] = a == b[c];
                    const int dg = c == 0 ? diag : h[c - 1];
                    e[c] = max(max(dg, base) + (eq[c] ? match12 : -mismatch12), hg[c]);
                }
                int lg = left - gap12, rowmax = 0;
#pragma unroll
                for (int c = 0; c < AL_C; ++c) {
                    const int v = max(e[c], lg);
                    r[c] = v >= AL_ONE ? v : 0;
                    lg = r[c] - gap12;
                    rowmax = max(rowmax, eq[c] ? r[c] : 0);
                }
#pragma unroll
                for (int c = 0; c < AL_C; ++c) { h[c] = r[c]; hg[c] = r[c] - gap12; }
                diag = left;
                smax = max(smax, rowmax);
                if (__any(rowmax >= thr)) {                         // few steps hold an alignment that counts
                    if (rowmax >= thr) atomicMax(&ae[p], rowmax);   // a match cell: 0 <= p < Ka
                }
                if (more && lane == 63 && p >= 0 && p < Ka) edge[p] = r[AL_C - 1];
                left = __shfl_up(r[AL_C - 1], 1);                   // lane 0 keeps its own value and overwrites it from the edge column
            }
        }
        smax = wave_max(smax);
        if (lane == 0) s_h[jl] = smax >> 12;
    }
    __syncthreads();

    if (tid < 64) {                                                 // AL_TILE <= 64: one wave writes the tile's scores and joins its best
        unsigned long long bv = 0ull;
        if (tid < nj) {
            const int r = s_h[tid];
            if (score) score[(long)i * M + j0 + tid] = r;
            if (r > 0) bv = ((unsigned long long)(uint32_t)r << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(j0 + tid + j_base));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(bv, o);
            bv = other > bv ? other : bv;
        }
        if (tid == 0 && bv) atomicMax(&best[i], bv);
    }
    for (int p = tid; p < Ka; p += AL_THREADS) {
        const int v = ae[p];
        if (v > 0) atomicMax(&align_end[(long)i * Sa + p], v);
    }
}

}  // namespace

extern "C" int pb_align_block(void) { return AL_BLOCK; }

extern "C" int pb_local_align(const uint32_t* A, const int32_t* alen, int32_t N, int32_t Sa, const uint32_t* B, const int32_t* blen, int32_t M, int32_t Sb,
                              int32_t match, int32_t mismatch, int32_t gap, int32_t min_score, int32_t exclude_self, int32_t j_base,
                              int32_t* score, int32_t* align_end, int64_t* best, int32_t accumulate, void* stream_) {
    PB_REQUIRE(N >= 0 && N <= (1 << 20), "pb_local_align: N = %d out of range (0 .. 2^20)", (int)N);
    PB_REQUIRE(M >= 0 && M <= (1 << 20), "pb_local_align: M = %d out of range (0 .. 2^20)", (int)M);
    PB_REQUIRE(Sa >= 1 && Sa <= AL_MAX_S, "pb_local_align: Sa = %d out of range (1 .. %d)", (int)Sa, AL_MAX_S);
    PB_REQUIRE(Sb >= 1 && Sb <= AL_MAX_S, "pb_local_align: Sb = %d out of range (1 .. %d)", (int)Sb, AL_MAX_S);
    PB_REQUIRE(match >= 1 && match <= 8, "pb_local_align: match = %d out of range (1 .. 8)", (int)match);
    PB_REQUIRE(mismatch >= 1 && mismatch <= 16, "pb_local_align: mismatch = %d out of range (1 .. 16)", (int)mismatch);
    PB_REQUIRE(gap >= 1 && gap <= 16, "pb_local_align: gap = %d out of range (1 .. 16)", (int)gap);
    PB_REQUIRE(min_score >= 1, "pb_local_align: min_score = %d must be >= 1", (int)min_score);
    PB_REQUIRE(exclude_self == 0 || exclude_self == 1, "pb_local_align: exclude_self = %d (0 or 1)", (int)exclude_self);
    PB_REQUIRE(accumulate == 0 || accumulate == 1, "pb_local_align: accumulate = %d (0 or 1)", (int)accumulate);
    PB_REQUIRE(j_base >= 0 && (int64_t)j_base + M <= (int64_t)1 << 31, "pb_local_align: j_base = %d out of range (0 .. 2^31 - M)", (int)j_base);
    PB_REQUIRE(!exclude_self || N == M, "pb_local_align: exclude_self needs N == M (got N = %d, M = %d)", (int)N, (int)M);
    // an empty side has no storage: its pointers may be NULL
    PB_REQUIRE((N == 0 || (A && alen)) && ((uintptr_t)A % 4 == 0) && ((uintptr_t)alen % 4 == 0), "pb_local_align: A and alen must be non-NULL 4-byte aligned pointers");
    PB_REQUIRE((M == 0 || (B && blen)) && ((uintptr_t)B % 4 == 0) && ((uintptr_t)blen % 4 == 0), "pb_local_align: B and blen must be non-NULL 4-byte aligned pointers");
    PB_REQUIRE((uintptr_t)score % 4 == 0, "pb_local_align: score must be NULL or an int32 pointer");
    PB_REQUIRE((N == 0 || align_end) && ((uintptr_t)align_end % 4 == 0), "pb_local_align: align_end must be a non-NULL int32 pointer");
    PB_REQUIRE((N == 0 || best) && ((uintptr_t)best % 8 == 0), "pb_local_align: best must be a non-NULL 8-byte aligned int64 pointer");
    const int tiles = (M + AL_TILE - 1) / AL_TILE;
    PB_REQUIRE((int64_t)N * tiles < ((int64_t)1 << 31), "pb_local_align: N = %d times %d tiles of M = %d passes the grid limit 2^31; feed the corpus in chunks",
               (int)N, tiles, (int)M);
    if (N == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    if (!accumulate) {
        PB_CHECK_HIP(hipMemsetAsync(align_end, 0, sizeof(int32_t) * (size_t)N * Sa, stream));
        PB_CHECK_HIP(hipMemsetAsync(best, 0, sizeof(int64_t) * (size_t)N, stream));
    }
    if (M == 0) return 0;
    // the A image and the align_end row, and one edge column per wave where a corpus row spans more than one block:
    // 98 816 bytes at Sa = Sb = 4096 (one workgroup per CU), 2 560 at Sa = Sb = 256
    const size_t lds = sizeof(int32_t) * ((size_t)al_image(Sa) + Sa + (Sb > AL_BLOCK ? (size_t)AL_WAVES * Sa : 0));
    if (lds > 65536) PB_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int thr = std::min<int>(min_score, 32768) << 12;          // H <= 8 * 4095 = 32 760: a larger min_score lets nothing count
    hipLaunchKernelGGL(align_kernel, dim3((unsigned)(N * tiles)), dim3(AL_THREADS), lds, stream, A, alen, (int)Sa, B, blen, (int)M, (int)Sb, tiles,
                       (int)match << 12, (int)mismatch << 12, (int)gap << 12, thr, (int)exclude_self, (int)j_base, score, align_end,
                       reinterpret_cast<unsigned long long*>(best));
    PB_LAUNCH_CHECK();
    return 0;
}
