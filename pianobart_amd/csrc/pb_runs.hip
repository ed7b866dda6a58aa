// K20: copy detection: the longest run of consecutive notes that a generated piece shares with a corpus piece.
//   keys_kernel   one workgroup per piece (grid sweep): one 32-bit key per note after the first, from the (S, 8) id rows
//   runs_kernel   one workgroup per (generated piece, tile of RN_TILE corpus pieces): run(p, q) = A[p] == B[q] ? run(p - 1, q - 1) + 1 : 0
// run(p, q) depends only on its own diagonal q - p. The workgroup lays a corpus row out in LDS as the cyclic string B[0 .. Kb - 1], STOP,
// B[0], ... of Ka + Kb + 2 entries; a cyclic diagonal c reads entry p + c at p = 0 .. Ka - 1. STOP matches nothing, so a run ends where
// the diagonal wraps from the row's last key to its first: the Kb + 1 cyclic diagonals of Ka cells each are the Ka + Kb - 1 real ones,
// every thread makes the same number of steps, and no cell is out of range. Thread t takes the PAIRS of diagonals c, c + 1 with
// c = 2 t, 2 t + 512, ... < Kb + 1: eight steps of both read ten consecutive entries as five aligned 8-byte words (ds_read_b64, lanes
// contiguous: full LDS width, no bank conflict), 5 LDS reads per 16 cells. With Kb + 1 odd the last pair's second diagonal is c = Kb + 1,
// which is diagonal 0 again: it finds nothing new and changes no maximum. Windows of at most 256 keys have too few diagonals for four
// waves of pairs: there a thread takes one diagonal and reads 4-byte words. A[p] is the same for the whole workgroup: a uniform (scalar)
// load from global memory, no LDS read. Every output is an integer maximum (LDS and global atomic max, vector atomics), so it depends
// on no order of threads, workgroups or chunks: equal inputs give equal bytes.
#include "pb_common.h"
#include "pb_api_internal.h"
#include "pb_pieces.h"
#include <algorithm>

namespace {

constexpr uint32_t NO_KEY = 0xFFFFFFFFu;        // in A: matches nothing
constexpr uint32_t STOP = 0xFFFFFFFEu;          // in the LDS image of B: matches nothing (a value with bit 31 set is "no key" on either side)

// ---- keys ------------------------------------------------------------------------------------------------------------------------------
constexpr int KY_THREADS = 256, KY_ROWS_PER_WG = 2048, KY_IDS = PIECE_IDS;

__global__ __launch_bounds__(KY_THREADS) void keys_kernel(const uint4* __restrict__ ids, const int32_t* __restrict__ start, const Pad8 pad,
                                                          const int16_t* __restrict__ pitch_of, uint32_t* __restrict__ keys, int32_t* __restrict__ klen,
                                                          int N, int S, int mode) {
    __shared__ int s_L;
    const int tid = threadIdx.x;
    for (int piece = blockIdx.x; piece < N; piece += gridDim.x) {
        const uint4* rows = ids + (long)piece * S;
        if (tid == 0) s_L = S;
        __syncthreads();
        const int L = first_special_row<KY_THREADS>(rows, S, pad, s_L);
        const int first = first_row(start, piece);
        const int K = max(L - first - 1, 0);                        // first < L <= S whenever K > 0
        uint32_t* out = keys + (long)piece * S;
        for (int t = tid; t < S; t += KY_THREADS) {
            uint32_t key = NO_KEY;
            if (t < K) {
                const uint4 prev = rows[first + t], row = rows[first + t + 1];
                const int pit = row_id(row, 3);
                int field = pit;
                if (mode == 1) {
                    const int k = pitch_of[pit], kp = pitch_of[row_id(prev, 3)];
                    field = (k >= 0 && kp >= 0) ? KY_IDS + k - kp : KY_IDS + 1216 + pit;
                }
                const int step = row_id(row, 0) - row_id(prev, 0);
                key = (uint32_t)field | ((uint32_t)row_id(row, 1) << 12) | ((uint32_t)((step >= 0 && step <= 2) ? step : 3) << 23);
            }
            out[t] = key;
        }
        if (tid == 0) klen[piece] = K;
        __syncthreads();                                            // s_L is rewritten by the next piece
    }
}

// ---- shared runs -------------------------------------------------------------------------------------------------------------------------
constexpr int RN_THREADS = 256, RN_TILE = 32, RN_MAX_S = 4096, RN_UNROLL = 8;

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// entries of the cyclic image of one corpus row, a multiple of 2 (the run_end row behind it stays 8-byte aligned)
__host__ __device__ constexpr int rn_image(int Sa, int Sb) { return (Sa + Sb + 3) & ~1; }

// dynamic LDS: bx[rn_image(Sa, Sb)] (the cyclic image of one corpus row), then re[Sa] (the run_end row of this workgroup).
// D = the diagonals of a thread: 2, or 1 where the window is so short (Sb <= 256) that pairs would leave under four waves with work
template <int D>
__global__ __launch_bounds__(RN_THREADS) void runs_kernel(const uint32_t* __restrict__ A, const int32_t* __restrict__ alen, int Sa,
                                                          const uint32_t* __restrict__ B, const int32_t* __restrict__ blen, int M, int Sb, int tiles,
                                                          int min_run, int exclude_self, int j_base, int32_t* __restrict__ R,
                                                          int32_t* __restrict__ run_end, unsigned long long* __restrict__ best) {
    extern __shared__ __attribute__((aligned(16))) int lds[];
    __shared__ int s_r[RN_TILE];
    uint32_t* bx = reinterpret_cast<uint32_t*>(lds);
    int* re = lds + rn_image(Sa, Sb);
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x;      // 1 to 4 waves: the host sizes the workgroup for Sb
    const int i = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * RN_TILE;
    const int nj = min(RN_TILE, M - j0);
    const int Ka = min(max(alen[i], 0), Sa);
    const uint32_t* __restrict__ a_row = A + (long)i * Sa;

    for (int p = tid; p < Ka; p += nthr) re[p] = 0;
    if (tid < RN_TILE) s_r[tid] = 0;
    __syncthreads();

    for (int jl = 0; jl < nj; ++jl) {
        const int j = j0 + jl;
        const int Kb = min(max(blen[j], 0), Sb);
        if (Ka == 0 || Kb == 0 || (exclude_self && j + j_base == i)) continue;      // workgroup-uniform
        const uint32_t* b_row = B + (long)j * Sb;
        const int period = Kb + 1, span = Ka + Kb + 2;              // entries 0 .. Ka + Kb + 1 are read; span <= rn_image(Sa, Sb)
        for (int x = tid; x < span; x += nthr) {
            const int q = x % period;
            uint32_t v = STOP;
            if (q < Kb) { v = b_row[q]; if (v >> 31) v = STOP; }
            bx[x] = v;
        }
        __syncthreads();
        int mx = 0;
        for (int c = D * tid; c < period; c += D * nthr) {          // the diagonals c .. c + D - 1
            const uint32_t* bd = bx + c;                            // D = 2: c and p are even in the block loop, 8-byte aligned reads
            int run[D], p = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) run[d] = 0;
            for (; p + RN_UNROLL <= Ka; p += RN_UNROLL) {           // the last read is entry c + p + 9 <= Kb + Ka + 1
                uint32_t a[RN_UNROLL], b[RN_UNROLL + 2];
                int r[D][RN_UNROLL], m = 0;
#pragma unroll
                for (int u = 0; u < RN_UNROLL; ++u) a[u] = a_row[p + u];
                if constexpr (D == 2) {
#pragma unroll
                    for (int u = 0; u < RN_UNROLL + 2; u += 2) {
                        const unsigned long long w = *reinterpret_cast<const unsigned long long*>(bd + p + u);      // one 8-byte LDS read
                        b[u] = (uint32_t)w;
                        b[u + 1] = (uint32_t)(w >> 32);
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < RN_UNROLL; ++u) b[u] = bd[p + u];
                }
#pragma unroll
                for (int u = 0; u < RN_UNROLL; ++u) {
                    const uint32_t av = (a[u] >> 31) ? NO_KEY : a[u];          // uniform: scalar work
#pragma unroll
                    for (int d = 0; d < D; ++d) {
                        run[d] = (av == b[u + d]) ? run[d] + 1 : 0;
                        r[d][u] = run[d];
                        m = max(m, run[d]);
                    }
                }
                mx = max(mx, m);
                if (m >= min_run) {                                 // one test per 8 D cells: few blocks hold a run that counts
#pragma unroll
                    for (int u = 0; u < RN_UNROLL; ++u) {
                        const int v = max(r[0][u], r[D - 1][u]);
                        if (v >= min_run) atomicMax(&re[p + u], v);
                    }
                }
            }
            for (; p < Ka; ++p) {                                   // the last read is entry c + D - 1 + Ka - 1 <= Kb + Ka
                const uint32_t a0 = a_row[p];
                const uint32_t av = (a0 >> 31) ? NO_KEY : a0;
                int v = 0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    run[d] = (av == bd[p + d]) ? run[d] + 1 : 0;
                    v = max(v, run[d]);
                }
                mx = max(mx, v);
                if (v >= min_run) atomicMax(&re[p], v);
            }
        }
        mx = wave_max(mx);
        if (lane == 0 && mx > 0) atomicMax(&s_r[jl], mx);
        __syncthreads();                                            // bx is rewritten by the next corpus piece
    }
    __syncthreads();

    if (tid < 64) {                                                 // RN_TILE <= 64: one wave writes the tile's R and joins its best
        unsigned long long bv = 0ull;
        if (tid < nj) {
            const int r = s_r[tid];
            if (R) R[(long)i * M + j0 + tid] = r;
            if (r > 0) bv = ((unsigned long long)(uint32_t)r << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(j0 + tid + j_base));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(bv, o);
            bv = other > bv ? other : bv;
        }
        if (tid == 0 && bv) atomicMax(&best[i], bv);
    }
    for (int p = tid; p < Ka; p += nthr) {
        const int v = re[p];
        if (v > 0) atomicMax(&run_end[(long)i * Sa + p], v);
    }
}

}  // namespace

extern "C" int pb_runs_tile(void) { return RN_TILE; }

extern "C" int pb_piece_keys(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, uint32_t* keys, int32_t* klen,
                             int32_t N, int32_t S, int32_t mode, void* stream_) {
    Pad8 pad;
    if (int e = check_pieces("pb_piece_keys", RN_MAX_S, "the key's fields are sized for it", ids16, start, pad8, pitch_of, N, S, pad)) return e;
    PB_REQUIRE((N == 0 || keys) && ((uintptr_t)keys % 4 == 0), "pb_piece_keys: keys must be a non-NULL uint32 pointer");
    PB_REQUIRE((N == 0 || klen) && ((uintptr_t)klen % 4 == 0), "pb_piece_keys: klen must be a non-NULL int32 pointer");
    PB_REQUIRE(mode == 0 || mode == 1, "pb_piece_keys: mode = %d (0 = exact, 1 = interval)", (int)mode);
    if (N == 0) return 0;
    hipLaunchKernelGGL(keys_kernel, dim3(piece_grid(N, S, KY_ROWS_PER_WG)), dim3(KY_THREADS), 0, (hipStream_t)stream_, (const uint4*)ids16, start, pad, pitch_of, keys, klen, (int)N,
                       (int)S, (int)mode);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_shared_runs(const uint32_t* A, const int32_t* alen, int32_t N, int32_t Sa, const uint32_t* B, const int32_t* blen, int32_t M, int32_t Sb,
                              int32_t min_run, int32_t exclude_self, int32_t j_base, int32_t* R, int32_t* run_end, int64_t* best, int32_t accumulate,
                              void* stream_) {
    PB_REQUIRE(N >= 0 && N <= (1 << 20), "pb_shared_runs: N = %d out of range (0 .. 2^20)", (int)N);
    PB_REQUIRE(M >= 0 && M <= (1 << 20), "pb_shared_runs: M = %d out of range (0 .. 2^20)", (int)M);
    PB_REQUIRE(Sa >= 1 && Sa <= RN_MAX_S, "pb_shared_runs: Sa = %d out of range (1 .. %d)", (int)Sa, RN_MAX_S);
    PB_REQUIRE(Sb >= 1 && Sb <= RN_MAX_S, "pb_shared_runs: Sb = %d out of range (1 .. %d)", (int)Sb, RN_MAX_S);
    PB_REQUIRE(min_run >= 1, "pb_shared_runs: min_run = %d must be >= 1", (int)min_run);
    PB_REQUIRE(exclude_self == 0 || exclude_self == 1, "pb_shared_runs: exclude_self = %d (0 or 1)", (int)exclude_self);
    PB_REQUIRE(accumulate == 0 || accumulate == 1, "pb_shared_runs: accumulate = %d (0 or 1)", (int)accumulate);
    PB_REQUIRE(j_base >= 0 && (int64_t)j_base + M <= (int64_t)1 << 31, "pb_shared_runs: j_base = %d out of range (0 .. 2^31 - M)", (int)j_base);
    PB_REQUIRE(!exclude_self || N == M, "pb_shared_runs: exclude_self needs N == M (got N = %d, M = %d)", (int)N, (int)M);
    // an empty side has no storage: its pointers may be NULL
    PB_REQUIRE((N == 0 || (A && alen)) && ((uintptr_t)A % 4 == 0) && ((uintptr_t)alen % 4 == 0), "pb_shared_runs: A and alen must be non-NULL 4-byte aligned pointers");
    PB_REQUIRE((M == 0 || (B && blen)) && ((uintptr_t)B % 4 == 0) && ((uintptr_t)blen % 4 == 0), "pb_shared_runs: B and blen must be non-NULL 4-byte aligned pointers");
    PB_REQUIRE((uintptr_t)R % 4 == 0, "pb_shared_runs: R must be NULL or an int32 pointer");
    PB_REQUIRE((N == 0 || run_end) && ((uintptr_t)run_end % 4 == 0), "pb_shared_runs: run_end must be a non-NULL int32 pointer");
    PB_REQUIRE((N == 0 || best) && ((uintptr_t)best % 8 == 0), "pb_shared_runs: best must be a non-NULL 8-byte aligned int64 pointer");
    const int tiles = (M + RN_TILE - 1) / RN_TILE;
    PB_REQUIRE((int64_t)N * tiles < ((int64_t)1 << 31), "pb_shared_runs: N = %d times %d tiles of M = %d passes the grid limit 2^31; feed the corpus in chunks",
               (int)N, tiles, (int)M);
    if (N == 0) return 0;
    hipStream_t stream = (hipStream_t)stream_;
    if (!accumulate) {
        PB_CHECK_HIP(hipMemsetAsync(run_end, 0, sizeof(int32_t) * (size_t)N * Sa, stream));
        PB_CHECK_HIP(hipMemsetAsync(best, 0, sizeof(int64_t) * (size_t)N, stream));
    }
    if (M == 0) return 0;
    const size_t lds = sizeof(int32_t) * ((size_t)rn_image(Sa, Sb) + Sa);      // 49 160 bytes at Sa = Sb = 4096
    // a thread takes one (Sb <= 256: the keys of pieces of up to 256 rows) or two diagonals of the Sb + 1 at most; whole waves, so that
    // no wave only waits at the barriers
    const int D = Sb <= RN_THREADS ? 1 : 2;
    const int threads = std::min(RN_THREADS, ((Sb + D) / D + 63) / 64 * 64);
    hipLaunchKernelGGL(D == 1 ? runs_kernel<1> : runs_kernel<2>, dim3((unsigned)(N * tiles)), dim3(threads), lds, stream, A, alen, (int)Sa, B, blen, (int)M, (int)Sb, tiles,
                       (int)min_run, (int)exclude_self, (int)j_base, R, run_end, reinterpret_cast<unsigned long long*>(best));
    PB_LAUNCH_CHECK();
    return 0;
}
