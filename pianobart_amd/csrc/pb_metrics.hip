// K19: set metrics for generated pieces (the protocol of Yang & Lerch, "On the evaluation of generative models in music"): per-piece
// integer features, pairwise feature distances, their moments and a Gaussian kernel density estimate. Four kernel families:
//   feat_kernel                         one workgroup per piece (grid sweep): 288 exact integer columns from the (S, 8) id rows
//   l2_kernel                           D[i, j] = |A_i - B_j|, difference form, 64 x 64 tile per workgroup, 4 x 4 per thread
//   moments_kernel / moments_sum_kernel n, sum, sum of squares, min, max of a distance matrix (or its strict upper triangle), f64
//   kde_kernel / kde_sum_kernel         lanes hold grid points, the samples are wave-uniform; one f64 partial row per sample slab
// Integer LDS atomics only (their sums do not depend on the order); every floating-point sum has a fixed order: per-thread strides,
// an LDS tree, and per-slab / per-workgroup partial rows summed front to back by a second kernel. Equal inputs give equal bytes.
#include "pb_common.h"
#include "pb_api_internal.h"
#include "pb_pieces.h"
#include <algorithm>
#include <climits>

namespace {

// ---- piece features ----------------------------------------------------------------------------------------------------------------
constexpr int FT_THREADS = 256, FT_COLS = 288, FT_IDS = PIECE_IDS;
constexpr int FT_ROWS_PER_WG = 2048;                               // a workgroup takes at least this many rows' worth of pieces
constexpr int C_PCH = 16, C_PCTM = 28, C_BEAT = 172, C_DUR = 188, C_VEL = 220, C_BARD = 252;

__global__ __launch_bounds__(FT_THREADS) void feat_kernel(const uint4* __restrict__ ids, const int32_t* __restrict__ start, const Pad8 pad,
                                                          const int16_t* __restrict__ pitch_of, const int32_t* __restrict__ dur_pos,
                                                          int32_t* __restrict__ feat, int N, int S) {
    __shared__ int f[FT_COLS];                     // the output row; the histograms are counted in place
    __shared__ int bar_cnt[FT_IDS];                // notes per bar id
    __shared__ uint32_t k_map[FT_IDS / 32], ins_map[FT_IDS / 32];
    __shared__ int wave_last[FT_THREADS / 64];     // the last pitched k of each wave of the chunk (-1: none)
    __shared__ int s_L, s_carry, s_bar_lo, s_bar_hi;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    for (int piece = blockIdx.x; piece < N; piece += gridDim.x) {
        const uint4* rows = ids + (long)piece * S;
        for (int i = tid; i < FT_COLS; i += FT_THREADS) f[i] = i == 5 ? INT_MAX : i == 6 ? -1 : 0;      // min k, max k start at their identities
        for (int i = tid; i < FT_IDS; i += FT_THREADS) bar_cnt[i] = 0;
        if (tid < FT_IDS / 32) { k_map[tid] = 0u; ins_map[tid] = 0u; }
        if (tid == 0) { s_L = S; s_carry = -1; s_bar_lo = INT_MAX; s_bar_hi = -1; }
        __syncthreads();
        const int L = first_special_row<FT_THREADS>(rows, S, pad, s_L);
        const int first = first_row(start, piece);

        int n_notes = 0, n_pitched = 0, iv_sum = 0, iv_cnt = 0, onsets = 0, back = 0, dur_sum = 0, vel_sum = 0;
        for (int base = first; base < L; base += FT_THREADS) {          // chunks of 256 rows, in row order
            const int r = base + tid;
            const bool live = r < L;
            int k = -1;
            if (live) {
                const uint4 row = rows[r];
                const int bar = row_id(row, 0), pos = row_id(row, 1), ins = row_id(row, 2), pit = row_id(row, 3), dur = row_id(row, 4), vel = row_id(row, 5);
                k = pitch_of[pit];
                ++n_notes;
                if (r > first) {
                    const uint4 prev = rows[r - 1];
                    const int t = bar * 1024 + pos, tp = row_id(prev, 0) * 1024 + row_id(prev, 1);
                    onsets += t != tp;
                    back += t < tp;
                } else {
                    onsets += 1;
                }
                dur_sum += dur_pos[dur];
                vel_sum += vel;
                atomicAdd(&bar_cnt[bar], 1);
                atomicMin(&s_bar_lo, bar);
                atomicMax(&s_bar_hi, bar);
                atomicOr(&ins_map[ins >> 5], 1u << (ins & 31));
                atomicAdd(&f[C_BEAT + (pos & 15)], 1);
                atomicAdd(&f[C_DUR + min(dur >> 2, 31)], 1);
                atomicAdd(&f[C_VEL + min(vel, 31)], 1);
            }
            // the previous pitched note: in this wave, else in an earlier wave of the chunk, else the carry of the earlier chunks
            const bool pitched = live && k >= 0;
            const unsigned long long pm = __ballot(pitched);
            const unsigned long long below = pm & ((1ull << lane) - 1ull);
            const int src = below ? 63 - __clzll((long long)below) : 0;
            const int k_wave = __shfl(k, src);
            const int top = pm ? 63 - __clzll((long long)pm) : 0;
            const int k_top = __shfl(k, top);
            if (lane == 0) wave_last[wave] = pm ? k_top : -1;
            __syncthreads();
            if (pitched) {
                int kp = below ? k_wave : -1;
                for (int w = wave - 1; w >= 0 && kp < 0; --w) kp = wave_last[w];
                if (kp < 0) kp = s_carry;
                ++n_pitched;
                if (k < FT_IDS) atomicOr(&k_map[k >> 5], 1u << (k & 31));
                atomicMin(&f[5], k);
                atomicMax(&f[6], k);
                atomicAdd(&f[C_PCH + k % 12], 1);
                if (kp >= 0) {
                    iv_sum += abs(k - kp);
                    ++iv_cnt;
                    atomicAdd(&f[C_PCTM + 12 * (kp % 12) + k % 12], 1);
                }
            }
            __syncthreads();
            if (tid == 0) {
                int c = -1;
                for (int w = FT_THREADS / 64 - 1; w >= 0 && c < 0; --w) c = wave_last[w];
                if (c >= 0) s_carry = c;
            }
            __syncthreads();
        }
        atomicAdd(&f[0], n_notes);
        atomicAdd(&f[1], n_pitched);
        atomicAdd(&f[7], iv_sum);
        atomicAdd(&f[8], iv_cnt);
        atomicAdd(&f[9], onsets);
        atomicAdd(&f[10], back);
        atomicAdd(&f[11], dur_sum);
        atomicAdd(&f[12], vel_sum);
        // distinct bars and their density histogram, distinct pitches and instruments
        int bars = 0, kinds = 0, inss = 0;
        for (int i = tid; i < FT_IDS; i += FT_THREADS) {
            const int c = bar_cnt[i];
            if (c > 0) { ++bars; atomicAdd(&f[C_BARD + min(c, 32) - 1], 1); }
        }
        if (tid < FT_IDS / 32) { kinds = __popc(k_map[tid]); inss = __popc(ins_map[tid]); }
        atomicAdd(&f[2], bars);
        atomicAdd(&f[4], kinds);
        atomicAdd(&f[13], inss);
        __syncthreads();
        if (tid == 0) {
            f[3] = s_bar_hi >= 0 ? s_bar_hi - s_bar_lo + 1 : 0;
            if (f[6] < 0) f[5] = -1;
        }
        __syncthreads();
        for (int i = tid; i < FT_COLS; i += FT_THREADS) feat[(long)piece * FT_COLS + i] = f[i];
        __syncthreads();
    }
}

// ---- pairwise distances --------------------------------------------------------------------------------------------------------------
constexpr int L2_TILE = 64, L2_FK = 16, L2_THREADS = 256, L2_MAX_F = 144;

__global__ __launch_bounds__(L2_THREADS) void l2_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ D, int N, int M, int F) {
    __shared__ __attribute__((aligned(16))) float As[L2_FK][L2_TILE + 4], Bs[L2_FK][L2_TILE + 4];      // feature-major: a thread reads its 4 rows as one 16-byte word
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i0 = blockIdx.y * L2_TILE, j0 = blockIdx.x * L2_TILE;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int f0 = 0; f0 < F; f0 += L2_FK) {
        // 64 rows x 16 features of each operand: thread t stages row t / 4, features (t % 4) * 4 .. + 3; rows and features past the end are
        // zeros in BOTH tiles, so they add (0 - 0)^2 = +0 and change no sum
        const int lr = tid >> 2, lf = (tid & 3) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int fcol = f0 + lf + q;
            As[lf + q][lr] = (i0 + lr < N && fcol < F) ? A[(long)(i0 + lr) * F + fcol] : 0.f;
            Bs[lf + q][lr] = (j0 + lr < M && fcol < F) ? B[(long)(j0 + lr) * F + fcol] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ff = 0; ff < L2_FK; ++ff) {          // features in order: every D[i, j] is one f32 chain over f = 0 .. F - 1
            const f32x4 av = *reinterpret_cast<const f32x4*>(&As[ff][ti * 4]);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[ff][tj * 4]);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float d = av[a] - bv[b];
                    acc[a][b] += d * d;
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + ti * 4 + a;
        if (i >= N) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + tj * 4 + b;
            if (j < M) D[(long)i * M + j] = sqrtf(acc[a][b]);
        }
    }
}

// ---- moments -----------------------------------------------------------------------------------------------------------------------------
constexpr int MO_THREADS = 256, MO_BLOCKS = 1024, MO_VALS = 5;      // partial row: n, sum, sum of squares, min, max

struct Mom { double n, s, q, lo, hi; };
__device__ __forceinline__ void mom_join(Mom& a, const Mom& b) {
    a.n += b.n; a.s += b.s; a.q += b.q; a.lo = fmin(a.lo, b.lo); a.hi = fmax(a.hi, b.hi);
}
// the fixed-order tree over the 256 threads' values; thread 0 holds the result
__device__ __forceinline__ Mom mom_block_reduce(Mom m, Mom* sh) {
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int o = MO_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { Mom a = sh[threadIdx.x]; mom_join(a, sh[threadIdx.x + o]); sh[threadIdx.x] = a; }
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(MO_THREADS) void moments_kernel(const float* __restrict__ D, long total, int M, int upper, double* __restrict__ part) {
    __shared__ Mom sh[MO_THREADS];
    Mom m = {0.0, 0.0, 0.0, HUGE_VAL, -HUGE_VAL};
    const long stride = (long)gridDim.x * MO_THREADS;
    for (long e = (long)blockIdx.x * MO_THREADS + threadIdx.x; e < total; e += stride) {
        if (upper && (e % M) <= (e / M)) continue;
        const double v = (double)D[e];
        m.n += 1.0; m.s += v; m.q += v * v; m.lo = fmin(m.lo, v); m.hi = fmax(m.hi, v);
    }
    m = mom_block_reduce(m, sh);
    if (threadIdx.x == 0) {
        double* p = part + (long)blockIdx.x * MO_VALS;
        p[0] = m.n; p[1] = m.s; p[2] = m.q; p[3] = m.lo; p[4] = m.hi;
    }
}

__global__ __launch_bounds__(MO_THREADS) void moments_sum_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out) {
    __shared__ Mom sh[MO_THREADS];
    Mom m = {0.0, 0.0, 0.0, HUGE_VAL, -HUGE_VAL};
    for (int b = threadIdx.x; b < nblk; b += MO_THREADS) {
        const double* p = part + (long)b * MO_VALS;
        const Mom o = {p[0], p[1], p[2], p[3], p[4]};
        mom_join(m, o);
    }
    m = mom_block_reduce(m, sh);
    if (threadIdx.x == 0) { out[0] = m.n; out[1] = m.s; out[2] = m.q; out[3] = 0.0; out[4] = m.lo; out[5] = m.hi; }
}

// ---- kernel density estimate ---------------------------------------------------------------------------------------------------------
constexpr int KD_THREADS = 256, KD_PER = 4, KD_TILE = KD_THREADS * KD_PER;      // 1024 grid points per workgroup, 4 per lane
constexpr int KD_WGS = 1024, KD_SLAB_MIN = 1024, KD_MAX_G = 4096;               // 4 workgroups on each of 256 CUs; a slab holds >= 1024 matrix entries

int kde_slabs(long total, int G) {
    const int tiles = (G + KD_TILE - 1) / KD_TILE;
    return (int)std::max(1L, std::min((long)(KD_WGS / tiles), (total + KD_SLAB_MIN - 1) / KD_SLAB_MIN));
}

constexpr int KD_UNROLL = 8;
__device__ __forceinline__ void kde_add(const float (&x)[KD_PER], double (&acc)[KD_PER], int np, float s, float c2) {
#pragma unroll
    for (int p = 0; p < KD_PER; ++p) {
        if (p < np) {
            const float d = x[p] - s;
            acc[p] += (double)__builtin_amdgcn_exp2f(d * d * c2);
        }
    }
}

// part[slab][g] = sum over the slab's samples s of exp2(c2 (grid[g] - s)^2), c2 = -log2(e) / (2 h^2): f32 terms, f64 sum in sample order
__global__ __launch_bounds__(KD_THREADS) void kde_kernel(const float* __restrict__ D, long total, int M, int upper, const float* __restrict__ grid, int G,
                                                         float c2, long per_slab, double* __restrict__ part) {
    const int g0 = blockIdx.y * KD_TILE + threadIdx.x;
    if (blockIdx.y * KD_TILE + (int)(threadIdx.x & ~63u) >= G) return;          // a wave with no grid point (no barrier below)
    float x[KD_PER];
    double acc[KD_PER];
#pragma unroll
    for (int p = 0; p < KD_PER; ++p) { const int g = g0 + p * KD_THREADS; x[p] = g < G ? grid[g] : 0.f; acc[p] = 0.0; }
    const int np = min(KD_PER, (G - blockIdx.y * KD_TILE + KD_THREADS - 1) / KD_THREADS);      // the lane's live points (workgroup-uniform)
    const long e0 = (long)blockIdx.x * per_slab, e1 = min(total, e0 + per_slab);
    for (long i = e0 / M; i * M < e1; ++i) {                                     // matrix rows of the slab; everything here is wave-uniform
        long lo = max(e0, i * M), hi = min(e1, (i + 1) * M);
        if (upper) lo = max(lo, i * M + i + 1);
        long e = lo;
        for (; e + KD_UNROLL <= hi; e += KD_UNROLL) {                            // the loads of 8 samples in flight, their terms added in sample order
            float s[KD_UNROLL];
#pragma unroll
            for (int u = 0; u < KD_UNROLL; ++u) s[u] = D[e + u];
#pragma unroll
            for (int u = 0; u < KD_UNROLL; ++u) kde_add(x, acc, np, s[u], c2);
        }
        for (; e < hi; ++e) kde_add(x, acc, np, D[e], c2);
    }
#pragma unroll
    for (int p = 0; p < KD_PER; ++p) { const int g = g0 + p * KD_THREADS; if (g < G) part[(long)blockIdx.x * G + g] = acc[p]; }
}

__global__ __launch_bounds__(KD_THREADS) void kde_sum_kernel(const double* __restrict__ part, int slabs, int G, double norm, double* __restrict__ dens) {
    const int g = blockIdx.x * KD_THREADS + threadIdx.x;
    if (g >= G) return;
    double s = 0.0;
    for (int b = 0; b < slabs; ++b) s += part[(long)b * G + g];
    dens[g] = norm * s;
}

// the shared checks of the two entries that read a distance matrix as samples; n_out = the number of samples
int check_samples(const char* who, const float* D, int64_t N, int64_t M, int32_t upper, const void* ws, int64_t& n_out) {
    PB_REQUIRE(D && ((uintptr_t)D % 4 == 0), "%s: D must be a non-NULL f32 pointer", who);
    PB_REQUIRE(N >= 1 && M >= 1 && N <= 65536 && M <= 65536, "%s: N = %lld, M = %lld out of range (1 .. 65536)", who, (long long)N, (long long)M);
    PB_REQUIRE(upper == 0 || upper == 1, "%s: upper = %d (0 or 1)", who, (int)upper);
    PB_REQUIRE(!upper || N == M, "%s: upper needs N == M (got N = %lld, M = %lld)", who, (long long)N, (long long)M);
    PB_REQUIRE(ws && ((uintptr_t)ws % 8 == 0), "%s: ws must be a non-NULL 8-byte aligned pointer (pb_metrics_ws_bytes)", who);
    n_out = upper ? N * (N - 1) / 2 : N * M;
    return 0;
}

}  // namespace

extern "C" int64_t pb_metrics_ws_bytes(int64_t N, int64_t M, int32_t G) {
    if (N < 1 || M < 1 || G < 1) return 0;
    const int64_t mom = (int64_t)MO_BLOCKS * MO_VALS * 8;
    const int64_t kde = (int64_t)kde_slabs((long)(N * M), (int)std::min<int32_t>(G, KD_MAX_G)) * G * 8;
    return std::max(mom, kde);
}

extern "C" int pb_piece_features(const int16_t* ids16, const int32_t* start, const int32_t* pad8, const int16_t* pitch_of, const int32_t* dur_pos,
                                 int32_t* feat, int32_t N, int32_t S, void* stream_) {
    Pad8 pad;
    if (int e = check_pieces("pb_piece_features", PIECE_MAX_S, "the per-id counters live in LDS", ids16, start, pad8, pitch_of, N, S, pad)) return e;
    PB_REQUIRE(dur_pos && ((uintptr_t)dur_pos % 4 == 0), "pb_piece_features: dur_pos must be a non-NULL int32 pointer");
    PB_REQUIRE(feat && ((uintptr_t)feat % 4 == 0), "pb_piece_features: feat must be a non-NULL int32 pointer");
    if (N == 0) return 0;
    hipLaunchKernelGGL(feat_kernel, dim3(piece_grid(N, S, FT_ROWS_PER_WG)), dim3(FT_THREADS), 0, (hipStream_t)stream_, (const uint4*)ids16, start, pad, pitch_of, dur_pos, feat, (int)N, (int)S);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_pairwise_l2(const float* A, const float* B, float* D, int32_t N, int32_t M, int32_t F, void* stream_) {
    PB_REQUIRE(A && B && D && ((uintptr_t)A % 4 == 0) && ((uintptr_t)B % 4 == 0) && ((uintptr_t)D % 4 == 0), "pb_pairwise_l2: A, B and D must be non-NULL f32 pointers");
    PB_REQUIRE(N >= 1 && M >= 1 && N <= 65536 && M <= 65536, "pb_pairwise_l2: N = %d, M = %d out of range (1 .. 65536)", (int)N, (int)M);
    PB_REQUIRE(F >= 1 && F <= L2_MAX_F, "pb_pairwise_l2: F = %d out of range (1 .. %d)", (int)F, L2_MAX_F);
    PB_REQUIRE(D != A && D != B, "pb_pairwise_l2: D aliases an input");
    const dim3 grid((M + L2_TILE - 1) / L2_TILE, (N + L2_TILE - 1) / L2_TILE);
    hipLaunchKernelGGL(l2_kernel, grid, dim3(L2_THREADS), 0, (hipStream_t)stream_, A, B, D, (int)N, (int)M, (int)F);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_sample_moments(const float* D, int64_t N, int64_t M, int32_t upper, double* out, void* ws, void* stream_) {
    int64_t n;
    if (int rc = check_samples("pb_sample_moments", D, N, M, upper, ws, n)) return rc;
    PB_REQUIRE(out && ((uintptr_t)out % 8 == 0), "pb_sample_moments: out must be a non-NULL device double[6]");
    const long total = (long)(N * M);
    const int grid = (int)std::min((long)MO_BLOCKS, (total + MO_THREADS - 1) / MO_THREADS);
    hipLaunchKernelGGL(moments_kernel, dim3(grid), dim3(MO_THREADS), 0, (hipStream_t)stream_, D, total, (int)M, (int)upper, (double*)ws);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(moments_sum_kernel, dim3(1), dim3(MO_THREADS), 0, (hipStream_t)stream_, (const double*)ws, grid, out);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_kde_eval(const float* D, int64_t N, int64_t M, int32_t upper, const float* grid, int32_t G, double h, double* dens, void* ws, void* stream_) {
    int64_t n;
    if (int rc = check_samples("pb_kde_eval", D, N, M, upper, ws, n)) return rc;
    PB_REQUIRE(n >= 1, "pb_kde_eval: no samples (upper with N = 1)");
    PB_REQUIRE(grid && ((uintptr_t)grid % 4 == 0), "pb_kde_eval: grid must be a non-NULL f32 pointer");
    PB_REQUIRE(G >= 1 && G <= KD_MAX_G, "pb_kde_eval: G = %d out of range (1 .. %d)", (int)G, KD_MAX_G);
    PB_REQUIRE(h > 0.0 && h < HUGE_VAL, "pb_kde_eval: h = %g must be positive and finite", h);
    PB_REQUIRE(dens && ((uintptr_t)dens % 8 == 0), "pb_kde_eval: dens must be a non-NULL device double pointer");
    const double c2d = -1.4426950408889634 / (2.0 * h * h);
    const float c2 = (float)c2d;
    PB_REQUIRE(c2 < 0.f && c2 > -HUGE_VALF, "pb_kde_eval: h = %g leaves 1 / (2 h^2) outside float32", h);
    const long total = (long)(N * M);
    const int slabs = kde_slabs(total, G);
    const long per_slab = (total + slabs - 1) / slabs;
    const int tiles = (G + KD_TILE - 1) / KD_TILE;
    hipLaunchKernelGGL(kde_kernel, dim3(slabs, tiles), dim3(KD_THREADS), 0, (hipStream_t)stream_, D, total, (int)M, (int)upper, grid, (int)G, c2, per_slab, (double*)ws);
    PB_LAUNCH_CHECK();
    const double norm = 1.0 / ((double)n * h * 2.5066282746310002);
    hipLaunchKernelGGL(kde_sum_kernel, dim3((G + KD_THREADS - 1) / KD_THREADS), dim3(KD_THREADS), 0, (hipStream_t)stream_, (const double*)ws, slabs, (int)G, norm, dens);
    PB_LAUNCH_CHECK();
    return 0;
}
