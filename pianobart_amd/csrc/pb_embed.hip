// K27: embedding-space set metrics. One vector per piece (mean of the encoder's hidden rows), the float64 moments of a set of such vectors,
// squared distances between rows up to 4096 wide, and the neighbourhood counts of precision / recall / density / coverage. Five families:
//   pool_kernel                          (B, S, d) bf16 / f32 -> (B, d) f32 masked row means, f64 sums in a fixed order, and the row counts
//   colsum_kernel / mean_kernel          column sums of X per row chunk, folded in chunk order into the f64 mean
//   scatter_kernel / scatter_fold_kernel 64 x 64 tiles of sum (x - mean)(x - mean)^T per row chunk, lower triangle, folded and mirrored
//   sqdist_kernel                        D2[i, j] = |A_i - B_j|^2, difference form, 64 x 64 tile per workgroup, 4 x 4 per thread
//   knn_kernel / ball_kernel             k-th smallest of a row by radix selection on the bits; strict < counts by row and by column
// No float atomics; every floating-point sum has a fixed order. Integer atomics where the result is an integer sum. Equal inputs give equal bytes.
#include "pb_common.h"
#include "pb_api_internal.h"
#include <algorithm>

namespace {

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---- masked row mean ----------------------------------------------------------------------------------------------------------------------
constexpr int PL_THREADS = 256, PL_GROUPS = 16, PL_SLICES = PL_THREADS / PL_GROUPS;      // 16 column groups x 16 slices of S: enough workgroups at B = 16, d = 768

template <typename T, int VEC> struct PoolLoad;
template <> struct PoolLoad<float, 1> { static __device__ __forceinline__ void get(const float* p, double (&v)[1]) { v[0] = (double)p[0]; } };
template <> struct PoolLoad<bf16_t, 1> { static __device__ __forceinline__ void get(const bf16_t* p, double (&v)[1]) { v[0] = (double)(float)p[0]; } };
template <> struct PoolLoad<float, 4> {
    static __device__ __forceinline__ void get(const float* p, double (&v)[4]) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = (double)x[q];
    }
};
template <> struct PoolLoad<bf16_t, 8> {
    static __device__ __forceinline__ void get(const bf16_t* p, double (&v)[8]) {
        const bf16x8 x = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = (double)(float)x[q];
    }
};

// thread (slice, group): columns c0 .. c0 + VEC - 1 of the rows of its slice, front to back. With VEC > 1 the host has made sure that d is a
// multiple of VEC and every row start 16-byte aligned.
template <typename T, int VEC>
__global__ __launch_bounds__(PL_THREADS) void pool_kernel(const T* __restrict__ H, long ldh, const float* __restrict__ mask, float* __restrict__ out,
                                                          long ldo, int32_t* __restrict__ count, int S, int d) {
    __shared__ double part[PL_SLICES][PL_GROUPS * VEC];
    __shared__ int cnt[PL_SLICES];
    const int b = blockIdx.y, g = threadIdx.x % PL_GROUPS, sl = threadIdx.x / PL_GROUPS;
    const int c0 = (blockIdx.x * PL_GROUPS + g) * VEC;
    const int per = (S + PL_SLICES - 1) / PL_SLICES, s0 = sl * per, s1 = min(S, s0 + per);
    const float* m = mask ? mask + (long)b * S : nullptr;
    double acc[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) acc[q] = 0.0;
    int n = 0;
    const bool live = c0 < d;
    for (int s = s0; s < s1; ++s) {
        if (m && m[s] == 0.f) continue;
        ++n;
        if (live) {
            double v[VEC];
            PoolLoad<T, VEC>::get(H + ((long)b * S + s) * ldh + c0, v);
#pragma unroll
            for (int q = 0; q < VEC; ++q) acc[q] += v[q];
        }
    }
#pragma unroll
    for (int q = 0; q < VEC; ++q) part[sl][g * VEC + q] = acc[q];
    if (g == 0) cnt[sl] = n;
    __syncthreads();
    if (sl != 0) return;
    int total = 0;
#pragma unroll
    for (int q = 0; q < PL_SLICES; ++q) total += cnt[q];
    if (live) {
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            double sum = part[0][g * VEC + q];
#pragma unroll
            for (int r = 1; r < PL_SLICES; ++r) sum += part[r][g * VEC + q];
            out[(long)b * ldo + c0 + q] = total > 0 ? (float)(sum / (double)total) : 0.f;
        }
    }
    if (blockIdx.x == 0 && g == 0) count[b] = total;
}

// ---- set moments ----------------------------------------------------------------------------------------------------------------------------
constexpr int MM_THREADS = 256, MM_TILE = 64, MM_NK = 16, MM_MAX_CHUNKS = 16, MM_MAX_D = 4096;
constexpr long MM_MAX_N = 1L << 24;

// rows per chunk (a multiple of MM_NK) and the number of chunks: a function of N alone
inline void mm_chunks(long N, long& rows, int& chunks) {
    rows = (N + MM_MAX_CHUNKS - 1) / MM_MAX_CHUNKS;
    rows = std::max<long>(256, (rows + MM_NK - 1) / MM_NK * MM_NK);
    chunks = (int)((N + rows - 1) / rows);
}
inline long mm_tiles(int d) { const long t = (d + MM_TILE - 1) / MM_TILE; return t * (t + 1) / 2; }

// part[chunk][c] = sum of X[n][c] over the chunk's rows, front to back
__global__ __launch_bounds__(MM_THREADS) void colsum_kernel(const float* __restrict__ X, long ldx, long N, int d, long rows, double* __restrict__ part) {
    const int c = blockIdx.x * MM_THREADS + threadIdx.x;
    if (c >= d) return;
    const long n0 = (long)blockIdx.y * rows, n1 = min(N, n0 + rows);
    double s = 0.0;
    for (long n = n0; n < n1; ++n) s += (double)X[n * ldx + c];
    part[(long)blockIdx.y * d + c] = s;
}

__global__ __launch_bounds__(MM_THREADS) void mean_kernel(const double* __restrict__ part, int chunks, int d, long N, double* __restrict__ mean) {
    const int c = blockIdx.x * MM_THREADS + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += part[(long)k * d + c];
    mean[c] = s / (double)N;
}

// tile t of the lower triangle -> (ti, tj), tj <= ti
__device__ __forceinline__ void tri_tile(int t, int& ti, int& tj) {
    int i = (int)((sqrtf(8.f * (float)t + 1.f) - 1.f) * 0.5f);
    while ((long)(i + 1) * (i + 2) / 2 <= t) ++i;
    while ((long)i * (i + 1) / 2 > t) --i;
    ti = i; tj = t - i * (i + 1) / 2;
}

// slot[chunk][tile][64][64] = sum over the chunk's rows of (x_i - mean_i)(x_j - mean_j), rows front to back; columns past d hold zeros
__global__ __launch_bounds__(MM_THREADS) void scatter_kernel(const float* __restrict__ X, long ldx, long N, int d, long rows,
                                                             const double* __restrict__ mean, double* __restrict__ slots) {
    __shared__ double Ai[MM_NK][MM_TILE + 2], Aj[MM_NK][MM_TILE + 2];
    int ti, tj;
    tri_tile(blockIdx.x, ti, tj);
    const int i0 = ti * MM_TILE, j0 = tj * MM_TILE;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const long n0 = (long)blockIdx.y * rows, n1 = min(N, n0 + rows);
    // staging: thread -> row tid / 16 of the slab, columns (tid % 16) + 16 q: a wave reads 16 consecutive floats of 4 rows
    const int lr = tid >> 4, lc = tid & 15;
    double mi[4], mj[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        mi[q] = i0 + lc + 16 * q < d ? mean[i0 + lc + 16 * q] : 0.0;
        mj[q] = j0 + lc + 16 * q < d ? mean[j0 + lc + 16 * q] : 0.0;
    }
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    for (long nb = n0; nb < n1; nb += MM_NK) {
        const long n = nb + lr;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ci = i0 + lc + 16 * q, cj = j0 + lc + 16 * q;
            Ai[lr][lc + 16 * q] = (n < n1 && ci < d) ? (double)X[n * ldx + ci] - mi[q] : 0.0;
            Aj[lr][lc + 16 * q] = (n < n1 && cj < d) ? (double)X[n * ldx + cj] - mj[q] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < MM_NK; ++r) {
            double av[4], bv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { av[a] = Ai[r][ty + 16 * a]; bv[a] = Aj[r][tx + 16 * a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
        }
        __syncthreads();
    }
    double* slot = slots + ((long)blockIdx.y * gridDim.x + blockIdx.x) * (MM_TILE * MM_TILE);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) slot[(ty + 16 * a) * MM_TILE + tx + 16 * b] = acc[a][b];
}

// C[i][j] = C[j][i] = the tile slots of (i, j), j <= i, added in chunk order
__global__ __launch_bounds__(MM_THREADS) void scatter_fold_kernel(const double* __restrict__ slots, int chunks, int tiles, int d, double* __restrict__ C, long ldc) {
    int ti, tj;
    tri_tile(blockIdx.x, ti, tj);
    for (int e = threadIdx.x; e < MM_TILE * MM_TILE; e += MM_THREADS) {
        const int i = ti * MM_TILE + e / MM_TILE, j = tj * MM_TILE + e % MM_TILE;
        if (i >= d || j > i) continue;
        double s = 0.0;
        for (int k = 0; k < chunks; ++k) s += slots[((long)k * tiles + blockIdx.x) * (MM_TILE * MM_TILE) + e];
        C[(long)i * ldc + j] = s;
        C[(long)j * ldc + i] = s;
    }
}

// ---- squared distances ------------------------------------------------------------------------------------------------------------------
constexpr int SQ_TILE = 64, SQ_FK = 32, SQ_THREADS = 256, SQ_MAX_D = 4096, SQ_MAX_ROWS = 1 << 20;

// 64 rows x 32 features of one operand, feature-major in LDS. Thread t stages row t / 4, features (t % 4) * 4 .. + 3 and the same + 16: the 64 lanes
// of a store hit 64 banks. Rows and features past the end are zeros in BOTH tiles: they add (0 - 0)^2 = +0 and change no sum.
template <bool VEC>
__device__ __forceinline__ void sq_stage(float (*T)[SQ_TILE + 4], const float* __restrict__ P, long ld, int r0, int nrows, int f0, int d, int tid) {
    const int lr = tid >> 2, lf = (tid & 3) * 4;
    const bool row_ok = r0 + lr < nrows;
    const float* p = P + (long)(r0 + lr) * ld;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int fl = lf + 16 * h, f = f0 + fl;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row_ok) {
            if (VEC && f + 3 < d) {
                v = *reinterpret_cast<const f32x4*>(p + f);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) if (f + q < d) v[q] = p[f + q];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) T[fl + q][lr] = v[q];
    }
}

template <bool VEC>
__global__ __launch_bounds__(SQ_THREADS) void sqdist_kernel(const float* __restrict__ A, long lda, const float* __restrict__ B, long ldb, float* __restrict__ D2,
                                                            long ldd, int N, int M, int d) {
    __shared__ __attribute__((aligned(16))) float As[SQ_FK][SQ_TILE + 4], Bs[SQ_FK][SQ_TILE + 4];      // a thread reads its 4 rows as one 16-byte word
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int i0 = blockIdx.y * SQ_TILE, j0 = blockIdx.x * SQ_TILE;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (int f0 = 0; f0 < d; f0 += SQ_FK) {
        sq_stage<VEC>(As, A, lda, i0, N, f0, d, tid);
        sq_stage<VEC>(Bs, B, ldb, j0, M, f0, d, tid);
        __syncthreads();
#pragma unroll
        for (int ff = 0; ff < SQ_FK; ++ff) {          // features in order: every D2[i, j] is one f32 chain over f = 0 .. d - 1
            const f32x4 av = *reinterpret_cast<const f32x4*>(&As[ff][ti * 4]);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[ff][tj * 4]);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float x = av[a] - bv[b];
                    acc[a][b] = fmaf(x, x, acc[a][b]);
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
            if (j < M) D2[(long)i * ldd + j] = acc[a][b];
        }
    }
}

// ---- k-th nearest neighbour ---------------------------------------------------------------------------------------------------------------
constexpr int KN_THREADS = 256, KN_MAX_K = 64;

// the order of floats as unsigned integers (negative values reversed below the positive ones) and back
__device__ __forceinline__ uint32_t f_key(float x) { const uint32_t u = __float_as_uint(x); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float key_f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// one workgroup per row: four passes of 8 bits, most significant first; each pass counts the digits of the entries that share the prefix found so
// far and walks the counts to the digit that holds the k-th entry
__global__ __launch_bounds__(KN_THREADS) void knn_kernel(const float* __restrict__ D2, long ldd, int N, int r0, int k, float* __restrict__ rad) {
    __shared__ int hist[KN_THREADS], scan[KN_THREADS];
    __shared__ uint32_t s_prefix;
    __shared__ int s_k;
    const int tid = threadIdx.x, row = blockIdx.x, self = r0 + row;
    const float* p = D2 + (long)row * ldd;
    if (tid == 0) { s_prefix = 0u; s_k = k; }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix, pmask = pass == 0 ? 0u : ~0u << (shift + 8);
        const int want = s_k;
        for (int j = tid; j < N; j += KN_THREADS) {
            if (j == self) continue;
            const uint32_t key = f_key(p[j]);
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        // inclusive scan of the 256 counts
        int v = hist[tid];
        scan[tid] = v;
        __syncthreads();
        for (int o = 1; o < KN_THREADS; o <<= 1) {
            const int add = tid >= o ? scan[tid - o] : 0;
            __syncthreads();
            v += add;
            scan[tid] = v;
            __syncthreads();
        }
        const int before = v - hist[tid];
        if (before < want && want <= v) {                      // exactly one digit
            s_prefix = prefix | ((uint32_t)tid << shift);
            s_k = want - before;
        }
        __syncthreads();
    }
    if (tid == 0) rad[row] = key_f(s_prefix);
}

// ---- ball counts ----------------------------------------------------------------------------------------------------------------------------
constexpr int BC_THREADS = 256, BC_ROWS = 32;

// a workgroup takes 32 rows x 256 columns; a thread owns a column, its column counts stay in registers, the row counts meet in LDS
__global__ __launch_bounds__(BC_THREADS) void ball_kernel(const float* __restrict__ D2, long ldd, int n, int M, const float* __restrict__ rad_ref,
                                                          const float* __restrict__ rad_gen, int32_t* __restrict__ row_hits, int32_t* __restrict__ col_hits,
                                                          int32_t* __restrict__ col_hits_gen) {
    __shared__ int rows[BC_ROWS];
    const int tid = threadIdx.x, j = blockIdx.x * BC_THREADS + tid, i0 = blockIdx.y * BC_ROWS;
    if (tid < BC_ROWS) rows[tid] = 0;
    __syncthreads();
    const bool live = j < M;
    const float rr = live ? rad_ref[j] : 0.f;
    int c_ref = 0, c_gen = 0;
    const int i1 = min(n, i0 + BC_ROWS);
    for (int i = i0; i < i1; ++i) {
        const float v = live ? D2[(long)i * ldd + j] : 0.f;
        const bool in_ref = live && v < rr, in_gen = live && v < rad_gen[i];
        c_ref += in_ref;
        c_gen += in_gen;
        const unsigned long long hit = __ballot(in_ref);
        if ((tid & 63) == 0 && hit) atomicAdd(&rows[i - i0], __popcll(hit));
    }
    if (c_ref) atomicAdd(&col_hits[j], c_ref);
    if (c_gen) atomicAdd(&col_hits_gen[j], c_gen);
    __syncthreads();
    if (tid < i1 - i0 && rows[tid]) atomicAdd(&row_hits[i0 + tid], rows[tid]);
}

bool f32_ptr(const void* p) { return p && ((uintptr_t)p % 4 == 0); }

}  // namespace

extern "C" int64_t pb_embed_ws_bytes(int64_t N, int32_t d) {
    if (N < 2 || N > MM_MAX_N || d < 1 || d > MM_MAX_D) return 0;
    long rows; int chunks;
    mm_chunks((long)N, rows, chunks);
    return (int64_t)chunks * ((int64_t)d + mm_tiles(d) * MM_TILE * MM_TILE) * 8;
}

extern "C" int pb_pool_rows(const void* H, int64_t ldh, int32_t dtype, const float* mask, float* out, int64_t ldo, int32_t* count, int32_t B, int32_t S,
                            int32_t d, void* stream_) {
    PB_REQUIRE(dtype == PB_F32 || dtype == PB_BF16, "pb_pool_rows: dtype = %d (PB_F32 or PB_BF16)", (int)dtype);
    const int esz = dtype == PB_F32 ? 4 : 2;
    PB_REQUIRE(H && ((uintptr_t)H % esz == 0), "pb_pool_rows: H must be a non-NULL pointer aligned to its element");
    PB_REQUIRE(B >= 1 && B <= 65535, "pb_pool_rows: B = %d out of range (1 .. 65535)", (int)B);
    PB_REQUIRE(S >= 1 && S <= 65536, "pb_pool_rows: S = %d out of range (1 .. 65536)", (int)S);
    PB_REQUIRE(d >= 1, "pb_pool_rows: d = %d must be >= 1", (int)d);
    PB_REQUIRE(ldh >= d, "pb_pool_rows: ldh = %lld is smaller than d = %d", (long long)ldh, (int)d);
    PB_REQUIRE(ldo >= d, "pb_pool_rows: ldo = %lld is smaller than d = %d", (long long)ldo, (int)d);
    PB_REQUIRE(mask == nullptr || f32_ptr(mask), "pb_pool_rows: mask must be NULL or an f32 pointer");
    PB_REQUIRE(f32_ptr(out), "pb_pool_rows: out must be a non-NULL f32 pointer");
    PB_REQUIRE(count && ((uintptr_t)count % 4 == 0), "pb_pool_rows: count must be a non-NULL int32 pointer");
    hipStream_t stream = (hipStream_t)stream_;
    const int vec = 16 / esz;
    const bool wide = aligned16(H) && (ldh * esz) % 16 == 0 && d % vec == 0;
    const int cols = PL_GROUPS * (wide ? vec : 1);
    const dim3 grid((d + cols - 1) / cols, B);
    if (dtype == PB_F32) {
        if (wide) hipLaunchKernelGGL((pool_kernel<float, 4>), grid, dim3(PL_THREADS), 0, stream, (const float*)H, (long)ldh, mask, out, (long)ldo, count, (int)S, (int)d);
        else hipLaunchKernelGGL((pool_kernel<float, 1>), grid, dim3(PL_THREADS), 0, stream, (const float*)H, (long)ldh, mask, out, (long)ldo, count, (int)S, (int)d);
    } else {
        if (wide) hipLaunchKernelGGL((pool_kernel<bf16_t, 8>), grid, dim3(PL_THREADS), 0, stream, (const bf16_t*)H, (long)ldh, mask, out, (long)ldo, count, (int)S, (int)d);
        else hipLaunchKernelGGL((pool_kernel<bf16_t, 1>), grid, dim3(PL_THREADS), 0, stream, (const bf16_t*)H, (long)ldh, mask, out, (long)ldo, count, (int)S, (int)d);
    }
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_embed_moments(const float* X, int64_t ldx, int64_t N, int32_t d, double* mean, double* C, int64_t ldc, void* ws, void* stream_) {
    PB_REQUIRE(f32_ptr(X), "pb_embed_moments: X must be a non-NULL f32 pointer");
    PB_REQUIRE(N >= 2 && N <= MM_MAX_N, "pb_embed_moments: N = %lld out of range (2 .. %ld)", (long long)N, MM_MAX_N);
    PB_REQUIRE(d >= 1 && d <= MM_MAX_D, "pb_embed_moments: d = %d out of range (1 .. %d)", (int)d, MM_MAX_D);
    PB_REQUIRE(ldx >= d, "pb_embed_moments: ldx = %lld is smaller than d = %d", (long long)ldx, (int)d);
    PB_REQUIRE(ldc >= d, "pb_embed_moments: ldc = %lld is smaller than d = %d", (long long)ldc, (int)d);
    PB_REQUIRE(mean && ((uintptr_t)mean % 8 == 0), "pb_embed_moments: mean must be a non-NULL f64 pointer");
    PB_REQUIRE(C && ((uintptr_t)C % 8 == 0), "pb_embed_moments: C must be a non-NULL f64 pointer");
    PB_REQUIRE(ws && ((uintptr_t)ws % 8 == 0), "pb_embed_moments: ws must be a non-NULL 8-byte aligned pointer (pb_embed_ws_bytes)");
    hipStream_t stream = (hipStream_t)stream_;
    long rows; int chunks;
    mm_chunks((long)N, rows, chunks);
    const int tiles = (int)mm_tiles(d);
    double* part = (double*)ws;
    double* slots = part + (long)chunks * d;
    const int cblocks = (d + MM_THREADS - 1) / MM_THREADS;
    hipLaunchKernelGGL(colsum_kernel, dim3(cblocks, chunks), dim3(MM_THREADS), 0, stream, X, (long)ldx, (long)N, (int)d, rows, part);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(mean_kernel, dim3(cblocks), dim3(MM_THREADS), 0, stream, (const double*)part, chunks, (int)d, (long)N, mean);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(scatter_kernel, dim3(tiles, chunks), dim3(MM_THREADS), 0, stream, X, (long)ldx, (long)N, (int)d, rows, (const double*)mean, slots);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(scatter_fold_kernel, dim3(tiles), dim3(MM_THREADS), 0, stream, (const double*)slots, chunks, tiles, (int)d, C, (long)ldc);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_sqdist(const float* A, int64_t lda, const float* B, int64_t ldb, float* D2, int64_t ldd, int32_t N, int32_t M, int32_t d, void* stream_) {
    PB_REQUIRE(f32_ptr(A) && f32_ptr(B) && f32_ptr(D2), "pb_sqdist: A, B and D2 must be non-NULL f32 pointers");
    PB_REQUIRE(N >= 1 && N <= SQ_MAX_ROWS && M >= 1 && M <= SQ_MAX_ROWS, "pb_sqdist: N = %d, M = %d out of range (1 .. %d)", (int)N, (int)M, SQ_MAX_ROWS);
    PB_REQUIRE(d >= 1 && d <= SQ_MAX_D, "pb_sqdist: d = %d out of range (1 .. %d)", (int)d, SQ_MAX_D);
    PB_REQUIRE(lda >= d && ldb >= d, "pb_sqdist: lda = %lld, ldb = %lld must be >= d = %d", (long long)lda, (long long)ldb, (int)d);
    PB_REQUIRE(ldd >= M, "pb_sqdist: ldd = %lld is smaller than M = %d", (long long)ldd, (int)M);
    PB_REQUIRE(D2 != A && D2 != B, "pb_sqdist: D2 aliases an input");
    const dim3 grid((M + SQ_TILE - 1) / SQ_TILE, (N + SQ_TILE - 1) / SQ_TILE);
    const bool wide = aligned16(A) && aligned16(B) && lda % 4 == 0 && ldb % 4 == 0;
    if (wide) hipLaunchKernelGGL(sqdist_kernel<true>, grid, dim3(SQ_THREADS), 0, (hipStream_t)stream_, A, (long)lda, B, (long)ldb, D2, (long)ldd, (int)N, (int)M, (int)d);
    else hipLaunchKernelGGL(sqdist_kernel<false>, grid, dim3(SQ_THREADS), 0, (hipStream_t)stream_, A, (long)lda, B, (long)ldb, D2, (long)ldd, (int)N, (int)M, (int)d);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_knn_radius(const float* D2, int64_t ldd, int32_t n, int32_t N, int32_t r0, int32_t k, float* rad, void* stream_) {
    PB_REQUIRE(f32_ptr(D2) && f32_ptr(rad), "pb_knn_radius: D2 and rad must be non-NULL f32 pointers");
    PB_REQUIRE(N >= 2 && N <= (1 << 24), "pb_knn_radius: N = %d out of range (2 .. 2^24)", (int)N);
    PB_REQUIRE(n >= 1 && r0 >= 0 && (int64_t)r0 + n <= N, "pb_knn_radius: rows r0 = %d .. r0 + n = %lld leave 0 .. N = %d", (int)r0, (long long)r0 + n, (int)N);
    PB_REQUIRE(k >= 1 && k <= std::min(N - 1, KN_MAX_K), "pb_knn_radius: k = %d out of range (1 .. min(N - 1, %d) = %d)", (int)k, KN_MAX_K, std::min(N - 1, KN_MAX_K));
    PB_REQUIRE(ldd >= N, "pb_knn_radius: ldd = %lld is smaller than N = %d", (long long)ldd, (int)N);
    hipLaunchKernelGGL(knn_kernel, dim3(n), dim3(KN_THREADS), 0, (hipStream_t)stream_, D2, (long)ldd, (int)N, (int)r0, (int)k, rad);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_ball_counts(const float* D2, int64_t ldd, int32_t n, int32_t M, const float* rad_ref, const float* rad_gen, int32_t* row_hits,
                              int32_t* col_hits, int32_t* col_hits_gen, void* stream_) {
    PB_REQUIRE(f32_ptr(D2) && f32_ptr(rad_ref) && f32_ptr(rad_gen), "pb_ball_counts: D2, rad_ref and rad_gen must be non-NULL f32 pointers");
    PB_REQUIRE(n >= 1 && n <= (1 << 20), "pb_ball_counts: n = %d out of range (1 .. 2^20)", (int)n);
    PB_REQUIRE(M >= 1 && M <= (1 << 24), "pb_ball_counts: M = %d out of range (1 .. 2^24)", (int)M);
    PB_REQUIRE(ldd >= M, "pb_ball_counts: ldd = %lld is smaller than M = %d", (long long)ldd, (int)M);
    PB_REQUIRE(row_hits && col_hits && col_hits_gen && ((uintptr_t)row_hits % 4 == 0) && ((uintptr_t)col_hits % 4 == 0) && ((uintptr_t)col_hits_gen % 4 == 0),
               "pb_ball_counts: row_hits, col_hits and col_hits_gen must be non-NULL int32 pointers");
    const dim3 grid((M + BC_THREADS - 1) / BC_THREADS, (n + BC_ROWS - 1) / BC_ROWS);
    hipLaunchKernelGGL(ball_kernel, grid, dim3(BC_THREADS), 0, (hipStream_t)stream_, D2, (long)ldd, (int)n, (int)M, rad_ref, rad_gen, row_hits, col_hits, col_hits_gen);
    PB_LAUNCH_CHECK();
    return 0;
}
