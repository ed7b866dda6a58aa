// K26: RegMean merging (the reference's model_merging_methods/merging_methods.py:266-416): W^T = (sum_m G_m)^-1 sum_m G_m W_m^T per linear layer,
// G_m the Gram matrix of the layer's inputs under model m. Entries:
//   pb_gram_accum      G (K, K) f32 += X^T X for X (T, K) bf16 or f32: only the 128x128 tiles on and below the diagonal are computed, the T
//                      dimension is cut into chunks over blockIdx.y, every (tile, chunk) writes its partial tile to ITS slot of a workspace and
//                      a second kernel folds the slots in chunk order, adds G and writes the result to (i, j) and (j, i): no atomics, the order
//                      of every addition a function of (T, K) alone, G symmetric bit for bit.
//   pb_regmean_scale   out = G * (diag on the diagonal, off elsewhere): reduce_non_diagonal_elements
//   pb_chol_factor     in-place lower Cholesky factor, blocks of 64 columns: diagonal block in LDS by one workgroup, the panel below it by
//                      forward substitution against that block, the trailing matrix by pb_gemm (f32, alpha = -1, accumulate)
//   pb_chol_solve      L L^T Z = R in place, blocked the same way: forward, then backward substitution
//   pb_transpose_f32   dst (cols, rows) = src (rows, cols)^T, the (out, in) layout of a Linear.weight from the solve's (in, out)
// X is (T, K) with the reduction over T, so BOTH operands of the Gram product are non-contiguous in the reduction dimension (pb_gemm's
// "TN" form). bf16: a thread loads a 4 (t) x 8 (column) block as four 16-byte vectors and writes it transposed, so LDS holds [column][t]
// rows whose 16-byte pieces are the MFMA's 8-element fragments. f32: the 16x16x4 MFMA takes ONE value per lane, A[lane & 15][lane >> 4],
// so the natural [t][column] image serves as it is. Rows are padded (144 B / 144 floats) instead of swizzled.
#include "pb_common.h"
#include "pb_api_internal.h"
#include <algorithm>

namespace {

// ---- G += X^T X ------------------------------------------------------------------------------------------------------------------------
constexpr int GT = 128, G_THREADS = 256;
constexpr int G_STAGE = 18432;                              // bytes of one staged operand: bf16 128 columns x 144 B, f32 32 rows x 576 B
constexpr int G_SLOT = GT * GT;                             // floats of one workspace slot
constexpr int G_WANT = 512;                                 // workgroups the T split aims at
constexpr long G_MIN_CHUNK = 256;                           // rows of X below which a chunk is not cut further

template <typename T> struct GElem;
template <> struct GElem<bf16_t> { static constexpr int EPV = 8, BKT = 64; };
template <> struct GElem<float>  { static constexpr int EPV = 4, BKT = 32; };

struct GVec { uint32_t w[4]; };
struct GStage { GVec v[4]; };

// one 16-byte vector of EPV elements starting at X[off]; `nvalid` of them are inside the matrix, the rest become 0
template <typename T>
__device__ __forceinline__ GVec gram_load(const T* __restrict__ X, long off, int nvalid, bool aligned) {
    constexpr int EPV = GElem<T>::EPV;
    GVec v = {{0u, 0u, 0u, 0u}};
    if (nvalid <= 0) return v;
    if (aligned && nvalid >= EPV) {
        const uint4 q = *reinterpret_cast<const uint4*>(X + off);
        v.w[0] = q.x; v.w[1] = q.y; v.w[2] = q.z; v.w[3] = q.w;
        return v;
    }
    if constexpr (sizeof(T) == 2) {
        const unsigned short* p = reinterpret_cast<const unsigned short*>(X) + off;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (j < nvalid) v.w[j >> 1] |= (uint32_t)p[j] << (16 * (j & 1));
    } else {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(X) + off;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (j < nvalid) v.w[j] = p[j];
    }
    return v;
}

// columns c0 .. c0 + 127, rows t0 .. t0 + BKT - 1 of X (rows >= t_end and columns >= K read as 0)
template <typename T>
__device__ __forceinline__ void gram_gload(GStage& s, const T* __restrict__ X, long ldx, int c0, long t0, long t_end, int K, bool aligned, int tid) {
    constexpr int EPV = GElem<T>::EPV;
    if constexpr (sizeof(T) == 2) {
        const int col = c0 + 8 * (tid & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long t = t0 + 4 * (tid >> 4) + i;
            s.v[i] = gram_load<T>(X, t * ldx + col, t < t_end ? K - col : 0, aligned);
        }
    } else {
        const int col = c0 + EPV * (tid & 31);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long t = t0 + (tid >> 5) + 8 * i;
            s.v[i] = gram_load<T>(X, t * ldx + col, t < t_end ? K - col : 0, aligned);
        }
    }
}

template <typename T>
__device__ __forceinline__ void gram_lstore(const GStage& s, char* lds, int tid) {
    if constexpr (sizeof(T) == 2) {
        const int cc = tid & 15, tg = tid >> 4;                 // [column][t]: column 8 cc + j gets t = 4 tg .. 4 tg + 3 as 8 bytes
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int w = j >> 1, sh = 16 * (j & 1);
            const uint32_t e0 = (s.v[0].w[w] >> sh) & 0xffffu, e1 = (s.v[1].w[w] >> sh) & 0xffffu;
            const uint32_t e2 = (s.v[2].w[w] >> sh) & 0xffffu, e3 = (s.v[3].w[w] >> sh) & 0xffffu;
            *reinterpret_cast<uint2*>(lds + (8 * cc + j) * 144 + 8 * tg) = make_uint2(e0 | (e1 << 16), e2 | (e3 << 16));
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)                             // [t][column]
            *reinterpret_cast<uint4*>(lds + ((tid >> 5) + 8 * i) * 576 + 16 * (tid & 31)) = make_uint4(s.v[i].w[0], s.v[i].w[1], s.v[i].w[2], s.v[i].w[3]);
    }
}

// A and B fragments are read the same way from images staged the same way, so element j of lane group g is the same t in both
template <typename T>
__device__ __forceinline__ void gram_mma(const char* ldsA, const char* ldsB, int wm, int wn, int lane, f32x4 (&acc)[4][4]) {
    const int lr = lane & 15, lg = lane >> 4;
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = *reinterpret_cast<const bf16x8*>(ldsA + (wm * 64 + i * 16 + lr) * 144 + ks * 64 + lg * 16);
                b[i] = *reinterpret_cast<const bf16x8*>(ldsB + (wn * 64 + i * 16 + lr) * 144 + ks * 64 + lg * 16);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = *reinterpret_cast<const float*>(ldsA + (ks * 4 + lg) * 576 + (wm * 64 + i * 16 + lr) * 4);
                b[i] = *reinterpret_cast<const float*>(ldsB + (ks * 4 + lg) * 576 + (wn * 64 + i * 16 + lr) * 4);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
}

// lower tile x -> (ti, tj), ti >= tj: x = ti (ti + 1) / 2 + tj
__device__ __forceinline__ void gram_tile(int x, int& ti, int& tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= x) ++ti;
    tj = x - ti * (ti + 1) / 2;
}

// grid (lower tiles, chunks): slot (tile, chunk) of ws = X[chunk rows, tile ti columns]^T X[chunk rows, tile tj columns]
template <typename T>
__global__ __launch_bounds__(G_THREADS) void gram_partial_kernel(const T* __restrict__ X, long ldx, long Tn, int K, long chunk, int aligned, float* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) char smem[2 * G_STAGE];
    constexpr int BKT = GElem<T>::BKT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    int ti, tj;
    gram_tile(blockIdx.x, ti, tj);
    const bool diag = ti == tj;                                  // both operands are the same columns: staged once
    const long t_begin = (long)blockIdx.y * chunk, t_end = t_begin + chunk < Tn ? t_begin + chunk : Tn;
    char* ldsA = smem;
    char* ldsB = diag ? smem : smem + G_STAGE;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    GStage sa, sb;
    gram_gload<T>(sa, X, ldx, ti * GT, t_begin, t_end, K, aligned, tid);
    if (!diag) gram_gload<T>(sb, X, ldx, tj * GT, t_begin, t_end, K, aligned, tid);
    for (long t0 = t_begin; t0 < t_end; t0 += BKT) {
        gram_lstore<T>(sa, ldsA, tid);
        if (!diag) gram_lstore<T>(sb, ldsB, tid);
        __syncthreads();
        if (t0 + BKT < t_end) {                                  // the next stage's loads fly over this stage's MFMAs
            gram_gload<T>(sa, X, ldx, ti * GT, t0 + BKT, t_end, K, aligned, tid);
            if (!diag) gram_gload<T>(sb, X, ldx, tj * GT, t0 + BKT, t_end, K, aligned, tid);
        }
        gram_mma<T>(ldsA, ldsB, wm, wn, lane, acc);
        __syncthreads();
    }

    // C/D map of the 16x16 MFMA: col = lane & 15, row = 4 (lane >> 4) + reg. The whole slot is written (zeros beyond K included).
    float* slot = ws + ((long)blockIdx.x * gridDim.y + blockIdx.y) * G_SLOT;
    const int lr = lane & 15, lg = lane >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) slot[(wm * 64 + i * 16 + lg * 4 + r) * GT + wn * 64 + j * 16 + lr] = acc[i][j][r];
}

// grid (lower tiles, 16): a thread owns 4 adjacent columns of one row of the tile. v = G[i][j] + ((p_0 + p_1) + ..) for j <= i goes to
// (i, j) and (j, i); of a diagonal tile only the lower half is used, so nothing rests on the MFMA being symmetric in its operands.
__global__ __launch_bounds__(G_THREADS) void gram_fold_kernel(const float* __restrict__ ws, int nsplit, float* __restrict__ G, long ldg, int K) {
    int ti, tj;
    gram_tile(blockIdx.x, ti, tj);
    const int e = blockIdx.y * G_THREADS + threadIdx.x, m = e >> 5, n4 = e & 31;
    const int gi = ti * GT + m, gj0 = tj * GT + 4 * n4;
    if (gi >= K || gj0 >= K || gj0 > gi) return;
    const float* slot = ws + (long)blockIdx.x * nsplit * G_SLOT + m * GT + 4 * n4;
    f32x4 sum = *reinterpret_cast<const f32x4*>(slot);
    for (int s = 1; s < nsplit; ++s) sum = sum + *reinterpret_cast<const f32x4*>(slot + (long)s * G_SLOT);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int gj = gj0 + q;
        if (gj < K && gj <= gi) {
            const float v = G[(long)gi * ldg + gj] + sum[q];
            G[(long)gi * ldg + gj] = v;
            if (gj != gi) G[(long)gj * ldg + gi] = v;
        }
    }
}

struct GramSplit { int ntiles, nsplit; long chunk; };
GramSplit gram_split(long T, int K) {
    const int nt = (K + GT - 1) / GT;
    GramSplit g;
    g.ntiles = nt * (nt + 1) / 2;
    const long want = std::max(1L, std::min((long)((G_WANT + g.ntiles - 1) / g.ntiles), (T + G_MIN_CHUNK - 1) / G_MIN_CHUNK));
    g.chunk = ((T + want - 1) / want + 63) / 64 * 64;           // whole stages of either dtype
    g.nsplit = (int)((T + g.chunk - 1) / g.chunk);
    return g;
}

// ---- out = G * F ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void regmean_scale_kernel(const float* G, long ldg, float* out, long ldo, int K, float off, float diag) {
    const long n = (long)K * K, stride = (long)gridDim.x * 256;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const long i = e / K, j = e - i * K;
        out[i * ldo + j] = G[i * ldg + j] * (i == j ? diag : off);
    }
}

// ---- Cholesky ---------------------------------------------------------------------------------------------------------------------------
constexpr int NB = 64;

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// one workgroup: the lower Cholesky factor of the n x n block at A (n <= 64), right-looking in LDS. A pivot <= 0 or not finite sets
// *info = 1 + col0 + j if *info is still 0 (kernels of one stream run in order, so the first such column of the first such matrix stays).
__global__ __launch_bounds__(256) void chol_diag_kernel(float* __restrict__ A, long ld, int n, int col0, int32_t* __restrict__ info) {
    __shared__ float s[NB][NB + 1];
    const int tid = threadIdx.x;
    for (int idx = tid; idx < NB * NB; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        s[r][c] = (r < n && c <= r) ? A[(long)r * ld + c] : 0.f;
    }
    for (int j = 0; j < n; ++j) {
        __syncthreads();
        const float d = s[j][j];
        const float l = sqrtf(d);
        __syncthreads();
        if (tid == 0) {
            s[j][j] = l;
            if ((!(d > 0.f) || !finite_f(d)) && *info == 0) *info = 1 + col0 + j;
        }
        if (tid > j && tid < n) s[tid][j] = s[tid][j] / l;
        __syncthreads();
        for (int idx = tid; idx < NB * NB; idx += 256) {
            const int i = idx >> 6, k = idx & 63;
            if (k > j && k <= i && i < n) s[i][k] = s[i][k] - s[i][j] * s[k][j];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < NB * NB; idx += 256) {
        const int r = idx >> 6, c = idx & 63;
        if (r < n && c <= r) A[(long)r * ld + c] = s[r][c];
    }
}

// 64 right-hand sides per workgroup, one per thread, against the n x n lower block L (n <= 64):
//   LT = false: L x = r (forward)      LT = true: L^T x = r (backward)
//   RHS_T = false: value (k, c) of the right-hand sides at R[k * ldr + c]      RHS_T = true: at R[c * ldr + k] (the factor's panel: x L^T = r by rows)
template <bool LT, bool RHS_T>
__global__ __launch_bounds__(64) void tri_solve_kernel(const float* __restrict__ L, long ldl, int n, float* __restrict__ R, long ldr, int nrhs) {
    __shared__ float Ls[NB][NB + 1], Rs[NB][NB + 1];
    const int tid = threadIdx.x, c0 = blockIdx.x * NB, cn = min(NB, nrhs - c0);
    for (int idx = tid; idx < NB * NB; idx += 64) {
        const int a = idx >> 6, b = idx & 63;
        Ls[a][b] = (a < n && b <= a) ? L[(long)a * ldl + b] : 0.f;
        if (RHS_T) Rs[b][a] = (a < cn && b < n) ? R[(long)(c0 + a) * ldr + b] : 0.f;
        else Rs[a][b] = (a < n && b < cn) ? R[(long)a * ldr + c0 + b] : 0.f;
    }
    __syncthreads();
    const int c = tid;
    if (!LT) {
        for (int j = 0; j < n; ++j) {
            float acc = Rs[j][c];
            for (int k = 0; k < j; ++k) acc = acc - Ls[j][k] * Rs[k][c];
            Rs[j][c] = acc / Ls[j][j];
        }
    } else {
        for (int j = n - 1; j >= 0; --j) {
            float acc = Rs[j][c];
            for (int k = j + 1; k < n; ++k) acc = acc - Ls[k][j] * Rs[k][c];
            Rs[j][c] = acc / Ls[j][j];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < NB * NB; idx += 64) {
        const int a = idx >> 6, b = idx & 63;
        if (RHS_T) { if (a < cn && b < n) R[(long)(c0 + a) * ldr + b] = Rs[b][a]; }
        else { if (a < n && b < cn) R[(long)a * ldr + c0 + b] = Rs[a][b]; }
    }
}

__global__ __launch_bounds__(256) void zero_upper_kernel(float* __restrict__ A, long ld, int K) {
    const long n = (long)K * K, stride = (long)gridDim.x * 256;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += stride) {
        const long i = e / K, j = e - i * K;
        if (j > i) A[i * ld + j] = 0.f;
    }
}

// dst[c][r] = src[r][c]: 32 x 32 tiles through LDS, 256 threads as 32 x 8
__global__ __launch_bounds__(256) void transpose_f32_kernel(const float* __restrict__ src, long lds_, float* __restrict__ dst, long ldd, int rows, int cols) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        if (r < rows && c < cols) tile[ty + 8 * i][tx] = src[(long)r * lds_ + c];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (r < rows && c < cols) dst[(long)c * ldd + r] = tile[tx][ty + 8 * i];
    }
}

bool f32_ptr(const void* p) { return p && ((uintptr_t)p % 4 == 0); }
int grid_for(long items) { return (int)std::max(1L, std::min(2048L, (items + 255) / 256)); }

// C (M, N) -= sum_k A(m, k) B(n, k) in f32 (the 16x16x4 f32-input MFMA kernel of pb_gemm.hip takes any M, N, K and leading dimension)
int gemm_sub(const float* A, int a_kc, long lda, const float* B, int b_kc, long ldb, float* C, long ldc, int M, int N, int K, void* stream) {
    pb_gemm_desc d = {};
    d.A = A; d.B = B; d.C = C;
    d.dtype = PB_F32; d.a_kcontig = a_kc; d.b_kcontig = b_kc; d.flags = PB_GEMM_ACCUM;
    d.M = M; d.N = N; d.K = K; d.nb1 = 1; d.nb2 = 1;
    d.lda = lda; d.ldb = ldb; d.ldc = ldc; d.ldaux = ldc;
    d.alpha = -1.0f; d.splitk = 1;
    return pb_gemm(&d, stream);
}

constexpr int CHOL_MAX_K = 32768, UPDATE_COLS = 512;

}  // namespace

extern "C" int64_t pb_gram_ws_bytes(int64_t T, int32_t K) {
    if (T < 1 || T > (1ll << 30) || K < 1 || K > CHOL_MAX_K) return 0;
    const GramSplit g = gram_split((long)T, K);
    return (int64_t)g.ntiles * g.nsplit * G_SLOT * (int64_t)sizeof(float);
}

extern "C" int pb_gram_accum(const void* X, int64_t ldx, int32_t dtype, int64_t T, int32_t K, float* G, int64_t ldg, void* ws, void* stream_) {
    PB_REQUIRE(dtype == PB_BF16 || dtype == PB_F32, "pb_gram_accum: dtype = %d (PB_F32 or PB_BF16)", (int)dtype);
    PB_REQUIRE(T >= 1 && T <= (1ll << 30), "pb_gram_accum: T = %lld (1 .. 2^30 rows)", (long long)T);
    PB_REQUIRE(K >= 1 && K <= CHOL_MAX_K, "pb_gram_accum: K = %d (1 .. %d columns)", (int)K, CHOL_MAX_K);
    PB_REQUIRE(ldx >= K && ldg >= K, "pb_gram_accum: ldx = %lld, ldg = %lld are below K = %d", (long long)ldx, (long long)ldg, (int)K);
    const int esz = dtype == PB_BF16 ? 2 : 4;
    PB_REQUIRE(X && ((uintptr_t)X % esz == 0), "pb_gram_accum: X must be a non-NULL pointer aligned to its element");
    PB_REQUIRE(f32_ptr(G), "pb_gram_accum: G must be a non-NULL f32 pointer");
    PB_REQUIRE(ws && ((uintptr_t)ws % 16 == 0), "pb_gram_accum: ws must be pb_gram_ws_bytes(T, K) bytes, 16-byte aligned");
    PB_REQUIRE((const void*)G != X && (const void*)G != ws && X != ws, "pb_gram_accum: X, G and ws must be distinct buffers");
    const GramSplit g = gram_split((long)T, K);
    const int aligned = ((uintptr_t)X % 16 == 0) && (ldx % (16 / esz) == 0);
    const dim3 grid(g.ntiles, g.nsplit);
    hipStream_t stream = (hipStream_t)stream_;
    if (dtype == PB_BF16) hipLaunchKernelGGL(gram_partial_kernel<bf16_t>, grid, dim3(G_THREADS), 0, stream, (const bf16_t*)X, (long)ldx, (long)T, (int)K, g.chunk, aligned, (float*)ws);
    else hipLaunchKernelGGL(gram_partial_kernel<float>, grid, dim3(G_THREADS), 0, stream, (const float*)X, (long)ldx, (long)T, (int)K, g.chunk, aligned, (float*)ws);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(gram_fold_kernel, dim3(g.ntiles, G_SLOT / (4 * G_THREADS)), dim3(G_THREADS), 0, stream, (const float*)ws, g.nsplit, G, (long)ldg, (int)K);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_regmean_scale(const float* G, int64_t ldg, float* out, int64_t ldo, int32_t K, float off, float diag, void* stream_) {
    PB_REQUIRE(K >= 1 && K <= CHOL_MAX_K, "pb_regmean_scale: K = %d (1 .. %d)", (int)K, CHOL_MAX_K);
    PB_REQUIRE(ldg >= K && ldo >= K, "pb_regmean_scale: ldg = %lld, ldo = %lld are below K = %d", (long long)ldg, (long long)ldo, (int)K);
    PB_REQUIRE(f32_ptr(G) && f32_ptr(out), "pb_regmean_scale: G and out must be non-NULL f32 pointers");
    PB_REQUIRE(out != G || ldo == ldg, "pb_regmean_scale: out aliases G with another leading dimension");
    hipLaunchKernelGGL(regmean_scale_kernel, dim3(grid_for((long)K * K)), dim3(256), 0, (hipStream_t)stream_, G, (long)ldg, out, (long)ldo, (int)K, off, diag);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_chol_factor(float* A, int64_t ld, int32_t K, int32_t* info, void* stream_) {
    PB_REQUIRE(K >= 1 && K <= CHOL_MAX_K, "pb_chol_factor: K = %d (1 .. %d)", (int)K, CHOL_MAX_K);
    PB_REQUIRE(ld >= K, "pb_chol_factor: ld = %lld is below K = %d", (long long)ld, (int)K);
    PB_REQUIRE(f32_ptr(A), "pb_chol_factor: A must be a non-NULL f32 pointer");
    PB_REQUIRE(info && ((uintptr_t)info % 4 == 0), "pb_chol_factor: info must be a device int32");
    hipStream_t stream = (hipStream_t)stream_;
    for (int k0 = 0; k0 < K; k0 += NB) {
        const int n = std::min(NB, K - k0), rem = K - k0 - n;
        float* Akk = A + (long)k0 * ld + k0;
        hipLaunchKernelGGL(chol_diag_kernel, dim3(1), dim3(256), 0, stream, Akk, (long)ld, n, k0, info);
        PB_LAUNCH_CHECK();
        if (rem == 0) break;
        float* panel = A + (long)(k0 + n) * ld + k0;             // (rem, n): L21 = A21 L11^-T, row by row
        hipLaunchKernelGGL((tri_solve_kernel<false, true>), dim3((rem + NB - 1) / NB), dim3(64), 0, stream, (const float*)Akk, (long)ld, n, panel, (long)ld, rem);
        PB_LAUNCH_CHECK();
        for (int c = 0; c < rem; c += UPDATE_COLS) {             // A22 -= L21 L21^T, the column blocks from their diagonal down
            const float* Lc = panel + (long)c * ld;
            const int rc = gemm_sub(Lc, 1, ld, Lc, 1, ld, A + (long)(k0 + n + c) * ld + (k0 + n + c), ld, rem - c, std::min(UPDATE_COLS, rem - c), n, stream_);
            if (rc) return rc;
        }
    }
    if (K > 1) {
        hipLaunchKernelGGL(zero_upper_kernel, dim3(grid_for((long)K * K)), dim3(256), 0, stream, A, (long)ld, (int)K);
        PB_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int pb_chol_solve(const float* L, int64_t ldl, int32_t K, float* R, int64_t ldr, int32_t nrhs, void* stream_) {
    PB_REQUIRE(K >= 1 && K <= CHOL_MAX_K, "pb_chol_solve: K = %d (1 .. %d)", (int)K, CHOL_MAX_K);
    PB_REQUIRE(nrhs >= 1, "pb_chol_solve: nrhs = %d (need nrhs >= 1)", (int)nrhs);
    PB_REQUIRE(ldl >= K && ldr >= nrhs, "pb_chol_solve: ldl = %lld is below K = %d or ldr = %lld below nrhs = %d", (long long)ldl, (int)K, (long long)ldr, (int)nrhs);
    PB_REQUIRE(f32_ptr(L) && f32_ptr(R), "pb_chol_solve: L and R must be non-NULL f32 pointers");
    PB_REQUIRE((const float*)R != L, "pb_chol_solve: R aliases L");
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((nrhs + NB - 1) / NB);
    const int last = (K - 1) / NB * NB;
    for (int k0 = 0; k0 < K; k0 += NB) {                         // L Y = R
        const int n = std::min(NB, K - k0), rem = K - k0 - n;
        hipLaunchKernelGGL((tri_solve_kernel<false, false>), grid, dim3(64), 0, stream, L + (long)k0 * ldl + k0, (long)ldl, n, R + (long)k0 * ldr, (long)ldr, (int)nrhs);
        PB_LAUNCH_CHECK();
        if (rem > 0) {                                           // R[k0 + n ..] -= L[k0 + n .., k0 .. k0 + n) Y_b
            const int rc = gemm_sub(L + (long)(k0 + n) * ldl + k0, 1, ldl, R + (long)k0 * ldr, 0, ldr, R + (long)(k0 + n) * ldr, ldr, rem, nrhs, n, stream_);
            if (rc) return rc;
        }
    }
    for (int k0 = last; k0 >= 0; k0 -= NB) {                     // L^T Z = Y
        const int n = std::min(NB, K - k0);
        hipLaunchKernelGGL((tri_solve_kernel<true, false>), grid, dim3(64), 0, stream, L + (long)k0 * ldl + k0, (long)ldl, n, R + (long)k0 * ldr, (long)ldr, (int)nrhs);
        PB_LAUNCH_CHECK();
        if (k0 > 0) {                                            // R[0 .. k0) -= L[k0 .. k0 + n, 0 .. k0)^T Z_b
            const int rc = gemm_sub(L + (long)k0 * ldl, 0, ldl, R + (long)k0 * ldr, 0, ldr, R, ldr, k0, nrhs, n, stream_);
            if (rc) return rc;
        }
    }
    return 0;
}

extern "C" int pb_transpose_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int32_t rows, int32_t cols, void* stream_) {
    PB_REQUIRE(rows >= 1 && cols >= 1, "pb_transpose_f32: rows = %d, cols = %d (need both >= 1)", (int)rows, (int)cols);
    PB_REQUIRE(lds >= cols && ldd >= rows, "pb_transpose_f32: lds = %lld is below cols = %d or ldd = %lld below rows = %d", (long long)lds, (int)cols, (long long)ldd, (int)rows);
    PB_REQUIRE(f32_ptr(src) && f32_ptr(dst), "pb_transpose_f32: src and dst must be non-NULL f32 pointers");
    PB_REQUIRE(src != dst, "pb_transpose_f32: dst aliases src");
    PB_REQUIRE((rows + 31) / 32 <= 65535, "pb_transpose_f32: rows = %d exceeds the grid", (int)rows);
    hipLaunchKernelGGL(transpose_f32_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, (hipStream_t)stream_, src, (long)lds, dst, (long)ldd, (int)rows, (int)cols);
    PB_LAUNCH_CHECK();
    return 0;
}
