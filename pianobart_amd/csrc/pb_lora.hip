// K27: LoRA (low-rank adapters on the attention projections): y = x W^T + b + s (x A^T) B^T with A (r, K), B (N, r), s = alpha / r. The products have
// an inner or an outer dimension of 4 .. 64, far below the 128 / 256 tiles of pb_gemm*.hip, so they get kernels of their own. Entries:
//   pb_lora_down    T (M, r) f32 = alpha * X (M, K; ld, offset) * W^T, W (r, K) or (K, r)          forward t = x A^T, backward dT = s dY B
//   pb_lora_up      Y (M, N; ld, offset) += alpha * T (M, r) * W, W (r, N) or (N, r)               forward y += s t B^T, backward dx += dT A
//   pb_lora_wgrad   G = alpha * T (M, r)^T * X (M, C; ld, offset), G (r, C) or (C, r) f32          dA = dT^T x, dB = s dY^T t
//   pb_lora_merge   W (N, K) += alpha * B (N, r) A (r, K), all f32                                 folding an adapter into its master weight
// X / Y are activations in the storage dtype (bf16 or f32), read or written ONCE with 16-byte vectors; the adapter matrices, the rank-r
// intermediates and every sum are f32. The first three run on the f32-input MFMA 16x16x4 (A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col =
// lane & 15], C[row = 4 (lane >> 4) + reg][col = lane & 15]): bit for bit an f32 fma chain, at the f32 vector rate, with one VGPR per operand.
// A lane's 16-byte vector holds EPV = 4 (f32) or 8 (bf16) neighbouring elements of one row; they feed EPV MFMAs:
//   down   the vector runs along the reduction (k): MFMA s sums k = k0 + EPV (lane >> 4) + s, the W fragment is read at the same k
//   up, wgrad   the vector runs along the output columns: MFMA b owns the columns n0 + EPV (lane & 15) + b, so that a lane ends up with EPV
//          neighbouring columns of 4 rows of the result: 16-byte read-modify-write of Y (up), 16-byte stores of the slot (wgrad)
// No atomics anywhere: down sums its four waves' shares of K through LDS in wave order, wgrad cuts M into chunks, one per wave, each wave writes
// its partial G to ITS slot of a workspace and a second kernel adds the slots in slot order (as pb_gram_accum does): equal inputs give equal bytes.
#include "pb_common.h"
#include "pb_api_internal.h"
#include <algorithm>

namespace {

constexpr int L_THREADS = 256;
constexpr int DOWN_ROWS = 32;                                // rows of X per workgroup of the down kernel (2 MFMA row tiles; its 4 waves split K)
constexpr int UP_ROWS = 256;                                 // rows of Y per workgroup of the up kernel (4 waves x 4 row tiles)
constexpr long L_MAX_M = 1l << 24;
constexpr int L_MAX_DIM = 1 << 20;

template <typename T> struct LElem;
template <> struct LElem<bf16_t> { static constexpr int EPV = 8; };
template <> struct LElem<float>  { static constexpr int EPV = 4; };

__device__ __forceinline__ float mfma4(float a, float b, f32x4& c) { c = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); return 0.f; }

// EPV elements starting at p as floats; the first `nvalid` lie inside the row, the others read as 0 (no address beyond them is touched)
template <typename T>
__device__ __forceinline__ void l_load(const T* __restrict__ p, int nvalid, bool aligned, float (&f)[LElem<T>::EPV]) {
    constexpr int EPV = LElem<T>::EPV;
#pragma unroll
    for (int j = 0; j < EPV; ++j) f[j] = 0.f;
    if (nvalid <= 0) return;
    if (aligned && nvalid >= EPV) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        if constexpr (sizeof(T) == 2) {
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) { f[2 * j] = __uint_as_float(w[j] << 16); f[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u); }
        } else {
            f[0] = __uint_as_float(q.x); f[1] = __uint_as_float(q.y); f[2] = __uint_as_float(q.z); f[3] = __uint_as_float(q.w);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < EPV; ++j) if (j < nvalid) f[j] = to_f(p[j]);
}

template <typename T>
__device__ __forceinline__ void l_store(T* __restrict__ p, int nvalid, bool aligned, const float (&f)[LElem<T>::EPV]) {
    constexpr int EPV = LElem<T>::EPV;
    if (nvalid <= 0) return;
    if (aligned && nvalid >= EPV) {
        uint4 q;
        if constexpr (sizeof(T) == 2) {
            uint32_t w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bf16_t lo = (bf16_t)f[2 * j], hi = (bf16_t)f[2 * j + 1];
                w[j] = (uint32_t)__builtin_bit_cast(unsigned short, lo) | ((uint32_t)__builtin_bit_cast(unsigned short, hi) << 16);
            }
            q = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            q = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
        }
        *reinterpret_cast<uint4*>(p) = q;
        return;
    }
#pragma unroll
    for (int j = 0; j < EPV; ++j) if (j < nvalid) p[j] = from_f<T>(f[j]);
}

// ---- T = alpha X W^T --------------------------------------------------------------------------------------------------------------------
// grid (row blocks of 32). Wave w takes the k steps w, w + 4, ... (a step = 4 EPV columns of X); the four partial tiles meet in LDS.
template <typename T, int NB4>
__global__ __launch_bounds__(L_THREADS) void lora_down_kernel(const T* __restrict__ X, long ldx, const float* __restrict__ W, int w_kr, float* __restrict__ Tout,
                                                              long M, int K, int r, float alpha, int aligned) {
    constexpr int EPV = LElem<T>::EPV, KSTEP = 4 * EPV, RT = DOWN_ROWS / 16;
    __shared__ float red[4][RT * NB4 * 4][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const long row0 = (long)blockIdx.x * DOWN_ROWS;
    f32x4 acc[RT][NB4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nb = 0; nb < NB4; ++nb) acc[rt][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = wave * KSTEP; k0 < K; k0 += 4 * KSTEP) {
        const int kk = k0 + EPV * lg;
        float xa[RT][EPV];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const long m = row0 + 16 * rt + lr;
            l_load<T>(X + m * ldx + kk, m < M ? K - kk : 0, aligned, xa[rt]);
        }
#pragma unroll
        for (int nb = 0; nb < NB4; ++nb) {
            if (16 * nb < r) {                                       // wave-uniform
                const int j = 16 * nb + lr;
                float wb[EPV];
#pragma unroll
                for (int s = 0; s < EPV; ++s) {
                    const int k = kk + s;
                    wb[s] = (j < r && k < K) ? (w_kr ? W[(long)k * r + j] : W[(long)j * K + k]) : 0.f;
                }
#pragma unroll
                for (int s = 0; s < EPV; ++s)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) mfma4(xa[rt][s], wb[s], acc[rt][nb]);
            }
        }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int nb = 0; nb < NB4; ++nb)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) red[wave][(rt * NB4 + nb) * 4 + reg][lane] = acc[rt][nb][reg];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RT * NB4; ++i) {
        const int idx = tid + L_THREADS * i, q = idx >> 6, ln = idx & 63;
        const float v = ((red[0][q][ln] + red[1][q][ln]) + red[2][q][ln]) + red[3][q][ln];
        const int reg = q & 3, nb = (q >> 2) % NB4, rt = (q >> 2) / NB4;
        const long m = row0 + 16 * rt + 4 * (ln >> 4) + reg;
        const int j = 16 * nb + (ln & 15);
        if (m < M && j < r) Tout[m * r + j] = alpha * v;
    }
}

// ---- Y += alpha T W -----------------------------------------------------------------------------------------------------------------------
// grid (row blocks of 256, column blocks of 16 EPV). A wave keeps the W fragments of its column block in registers and walks over row tiles.
template <typename T, int NB4>
__global__ __launch_bounds__(L_THREADS) void lora_up_kernel(T* __restrict__ Y, long ldy, const float* __restrict__ Tin, const float* __restrict__ W, int w_nr,
                                                            long M, int N, int r, float alpha, int aligned) {
    constexpr int EPV = LElem<T>::EPV, KS = 4 * NB4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int nn = blockIdx.y * 16 * EPV + lr * EPV, nks = r >> 2;
    float wb[KS][EPV];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int k = 4 * ks + lg;
#pragma unroll
        for (int b = 0; b < EPV; ++b) {
            const int n = nn + b;
            wb[ks][b] = (ks < nks && n < N) ? (w_nr ? W[(long)n * r + k] : W[(long)k * N + n]) : 0.f;
        }
    }
    const long rowb = (long)blockIdx.x * UP_ROWS;
    for (int rt = wave; rt < UP_ROWS / 16; rt += 4) {
        const long row0 = rowb + 16 * rt;
        if (row0 >= M) break;
        float y[4][EPV];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const long m = row0 + 4 * lg + reg;
            l_load<T>(Y + m * ldy + nn, m < M ? N - nn : 0, aligned, y[reg]);
        }
        float ta[KS];
        const long ma = row0 + lr;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ta[ks] = (ks < nks && ma < M) ? Tin[ma * r + 4 * ks + lg] : 0.f;
        f32x4 acc[EPV];
#pragma unroll
        for (int b = 0; b < EPV; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            if (ks < nks) {
#pragma unroll
                for (int b = 0; b < EPV; ++b) mfma4(ta[ks], wb[ks][b], acc[b]);
            }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const long m = row0 + 4 * lg + reg;
#pragma unroll
            for (int b = 0; b < EPV; ++b) y[reg][b] = fmaf(alpha, acc[b][reg], y[reg][b]);
            l_store<T>(Y + m * ldy + nn, m < M ? N - nn : 0, aligned, y[reg]);
        }
    }
}

// ---- G = alpha T^T X ----------------------------------------------------------------------------------------------------------------------
// grid (slot groups of 4, column blocks of 16 EPV). Wave = one slot: rows slot * chunk .. of X and T, its (r, C block) partial into ws[slot].
template <typename T, int NB4>
__global__ __launch_bounds__(L_THREADS) void lora_wgrad_kernel(const float* __restrict__ Tin, const T* __restrict__ X, long ldx, long M, int C, int r, long chunk, int nsplit,
                                                               int aligned, float* __restrict__ ws) {
    constexpr int EPV = LElem<T>::EPV;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lg = lane >> 4;
    const int slot = blockIdx.x * 4 + wave;
    if (slot >= nsplit) return;
    const long m_begin = (long)slot * chunk, m_end = m_begin + chunk < M ? m_begin + chunk : M;
    const int nn = blockIdx.y * 16 * EPV + lr * EPV;
    f32x4 acc[NB4][EPV];
#pragma unroll
    for (int jb = 0; jb < NB4; ++jb)
#pragma unroll
        for (int b = 0; b < EPV; ++b) acc[jb][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (long m0 = m_begin; m0 < m_end; m0 += 4) {
        const long m = m0 + lg;
        const bool valid = m < m_end;
        float x[EPV];
        l_load<T>(X + m * ldx + nn, valid ? C - nn : 0, aligned, x);
#pragma unroll
        for (int jb = 0; jb < NB4; ++jb)
            if (16 * jb < r) {
                const int j = 16 * jb + lr;
                const float ta = (valid && j < r) ? Tin[m * r + j] : 0.f;
#pragma unroll
                for (int b = 0; b < EPV; ++b) mfma4(ta, x[b], acc[jb][b]);
            }
    }
    float* out = ws + (long)slot * r * C;
    const bool vec = (C & 3) == 0 && nn + EPV <= C;
#pragma unroll
    for (int jb = 0; jb < NB4; ++jb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int j = 16 * jb + 4 * lg + reg;
            if (j < r) {
                float* p = out + (long)j * C + nn;
                if (vec) {
#pragma unroll
                    for (int b = 0; b < EPV; b += 4) *reinterpret_cast<f32x4*>(p + b) = f32x4{acc[jb][b][reg], acc[jb][b + 1][reg], acc[jb][b + 2][reg], acc[jb][b + 3][reg]};
                } else {
#pragma unroll
                    for (int b = 0; b < EPV; ++b) if (nn + b < C) p[b] = acc[jb][b][reg];
                }
            }
        }
}

// G[j][n] (or G[n][j]) = alpha * (((slot 0 + slot 1) + slot 2) + ...): one thread per element
__global__ __launch_bounds__(L_THREADS) void lora_wgrad_fold_kernel(const float* __restrict__ ws, int nsplit, float* __restrict__ G, int g_cr, int C, int r, float alpha) {
    const long n_el = (long)r * C, stride = (long)gridDim.x * L_THREADS;
    for (long e = (long)blockIdx.x * L_THREADS + threadIdx.x; e < n_el; e += stride) {
        float sum = ws[e];
        for (int s = 1; s < nsplit; ++s) sum += ws[(long)s * n_el + e];
        const long j = e / C, n = e - j * C;
        G[g_cr ? n * r + j : e] = alpha * sum;
    }
}

// ---- W += alpha B A -----------------------------------------------------------------------------------------------------------------------
// a thread owns 4 neighbouring k of one row n: one fma chain over j = 0 .. r - 1 per element, then one fma onto W
__global__ __launch_bounds__(L_THREADS) void lora_merge_kernel(float* __restrict__ W, const float* __restrict__ B, const float* __restrict__ A, long N, int K, int r, float alpha,
                                                               int aligned) {
    const int K4 = (K + 3) >> 2;
    const long n_el = N * K4, stride = (long)gridDim.x * L_THREADS;
    for (long e = (long)blockIdx.x * L_THREADS + threadIdx.x; e < n_el; e += stride) {
        const long n = e / K4;
        const int k = 4 * (int)(e - n * K4), nv = K - k;
        float acc[4] = {0.f, 0.f, 0.f, 0.f}, a[4], w[4];
        for (int j = 0; j < r; ++j) {
            const float b = B[n * r + j];
            l_load<float>(A + (long)j * K + k, nv, aligned, a);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = fmaf(b, a[q], acc[q]);
        }
        l_load<float>(W + n * K + k, nv, aligned, w);
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = fmaf(alpha, acc[q], w[q]);
        l_store<float>(W + n * K + k, nv, aligned, w);
    }
}

struct WgradSplit { long chunk; int nsplit; };
WgradSplit wgrad_split(long M, int r) {
    const long target = r <= 16 ? 128 : 64;
    WgradSplit s;
    s.chunk = std::max(64L, ((M + target - 1) / target + 3) / 4 * 4);
    s.nsplit = (int)std::max(1L, (M + s.chunk - 1) / s.chunk);
    return s;
}

bool elem_ptr(const void* p, int esz) { return p && ((uintptr_t)p % esz == 0); }
bool f32_ok(const void* p) { return elem_ptr(p, 4); }
bool rank_ok(int r) { return r >= 4 && r <= 64 && (r & 3) == 0; }
bool vec_ok(const void* p, long ld, int esz) { return ((uintptr_t)p % 16 == 0) && (ld % (16 / esz) == 0); }

#define LORA_BY_RANK(KERNEL, TYPE, r, ...)                                                                             \
    do {                                                                                                               \
        if ((r) <= 16) hipLaunchKernelGGL((KERNEL<TYPE, 1>), __VA_ARGS__);                                            \
        else if ((r) <= 32) hipLaunchKernelGGL((KERNEL<TYPE, 2>), __VA_ARGS__);                                       \
        else if ((r) <= 48) hipLaunchKernelGGL((KERNEL<TYPE, 3>), __VA_ARGS__);                                       \
        else hipLaunchKernelGGL((KERNEL<TYPE, 4>), __VA_ARGS__);                                                      \
    } while (0)

}  // namespace

extern "C" int pb_lora_down_rows(void) { return DOWN_ROWS; }
extern "C" int pb_lora_up_rows(void) { return UP_ROWS; }

extern "C" int64_t pb_lora_wgrad_chunk(int64_t M, int32_t r) {
    if (M < 1 || M > L_MAX_M || !rank_ok(r)) return 0;
    return wgrad_split((long)M, r).chunk;
}

extern "C" int64_t pb_lora_wgrad_ws_floats(int64_t M, int32_t r, int32_t C) {
    if (M < 1 || M > L_MAX_M || !rank_ok(r) || C < 1 || C > L_MAX_DIM) return 0;
    return (int64_t)wgrad_split((long)M, r).nsplit * r * C;
}

extern "C" int pb_lora_down(const void* X, int64_t ldx, int64_t x_off, int32_t dtype, const float* W, int32_t w_kr, float* T, int64_t M, int32_t K, int32_t r,
                            float alpha, void* stream_) {
    PB_REQUIRE(dtype == PB_BF16 || dtype == PB_F32, "pb_lora_down: dtype = %d (PB_F32 or PB_BF16)", (int)dtype);
    PB_REQUIRE(rank_ok(r), "pb_lora_down: r = %d (a multiple of 4 in 4 .. 64)", (int)r);
    PB_REQUIRE(M >= 0 && M <= L_MAX_M, "pb_lora_down: M = %lld (0 .. 2^24 rows)", (long long)M);
    PB_REQUIRE(K >= 1 && K <= L_MAX_DIM, "pb_lora_down: K = %d (1 .. 2^20 columns)", (int)K);
    PB_REQUIRE(x_off >= 0 && ldx >= x_off + K, "pb_lora_down: ldx = %lld is below x_off + K = %lld + %d", (long long)ldx, (long long)x_off, (int)K);
    PB_REQUIRE(w_kr == 0 || w_kr == 1, "pb_lora_down: w_kr = %d (0: W is (r, K), 1: W is (K, r))", (int)w_kr);
    const int esz = dtype == PB_BF16 ? 2 : 4;
    PB_REQUIRE(elem_ptr(X, esz), "pb_lora_down: X must be a non-NULL pointer aligned to its element");
    PB_REQUIRE(f32_ok(W), "pb_lora_down: W must be a non-NULL f32 pointer");
    PB_REQUIRE(f32_ok(T), "pb_lora_down: T must be a non-NULL f32 pointer");
    PB_REQUIRE((const void*)T != X && (const void*)T != (const void*)W, "pb_lora_down: T must not alias X or W");
    if (M == 0) return 0;
    const char* x = (const char*)X + x_off * esz;
    const int aligned = vec_ok(x, ldx, esz);
    const dim3 grid((unsigned)((M + DOWN_ROWS - 1) / DOWN_ROWS)), block(L_THREADS);
    hipStream_t stream = (hipStream_t)stream_;
    if (dtype == PB_BF16) LORA_BY_RANK(lora_down_kernel, bf16_t, r, grid, block, 0, stream, (const bf16_t*)x, (long)ldx, W, (int)w_kr, T, (long)M, (int)K, (int)r, alpha, aligned);
    else LORA_BY_RANK(lora_down_kernel, float, r, grid, block, 0, stream, (const float*)x, (long)ldx, W, (int)w_kr, T, (long)M, (int)K, (int)r, alpha, aligned);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_lora_up(void* Y, int64_t ldy, int64_t y_off, int32_t dtype, const float* T, const float* W, int32_t w_nr, int64_t M, int32_t N, int32_t r,
                          float alpha, void* stream_) {
    PB_REQUIRE(dtype == PB_BF16 || dtype == PB_F32, "pb_lora_up: dtype = %d (PB_F32 or PB_BF16)", (int)dtype);
    PB_REQUIRE(rank_ok(r), "pb_lora_up: r = %d (a multiple of 4 in 4 .. 64)", (int)r);
    PB_REQUIRE(M >= 0 && M <= L_MAX_M, "pb_lora_up: M = %lld (0 .. 2^24 rows)", (long long)M);
    PB_REQUIRE(N >= 1 && N <= L_MAX_DIM, "pb_lora_up: N = %d (1 .. 2^20 columns)", (int)N);
    PB_REQUIRE(y_off >= 0 && ldy >= y_off + N, "pb_lora_up: ldy = %lld is below y_off + N = %lld + %d", (long long)ldy, (long long)y_off, (int)N);
    PB_REQUIRE(w_nr == 0 || w_nr == 1, "pb_lora_up: w_nr = %d (0: W is (r, N), 1: W is (N, r))", (int)w_nr);
    const int esz = dtype == PB_BF16 ? 2 : 4;
    PB_REQUIRE(elem_ptr(Y, esz), "pb_lora_up: Y must be a non-NULL pointer aligned to its element");
    PB_REQUIRE(f32_ok(T), "pb_lora_up: T must be a non-NULL f32 pointer");
    PB_REQUIRE(f32_ok(W), "pb_lora_up: W must be a non-NULL f32 pointer");
    PB_REQUIRE((const void*)T != Y && (const void*)W != Y, "pb_lora_up: Y must not alias T or W");
    if (M == 0) return 0;
    char* y = (char*)Y + y_off * esz;
    const int aligned = vec_ok(y, ldy, esz);
    const int cols = 16 * (16 / esz);
    const dim3 grid((unsigned)((M + UP_ROWS - 1) / UP_ROWS), (unsigned)((N + cols - 1) / cols)), block(L_THREADS);
    hipStream_t stream = (hipStream_t)stream_;
    if (dtype == PB_BF16) LORA_BY_RANK(lora_up_kernel, bf16_t, r, grid, block, 0, stream, (bf16_t*)y, (long)ldy, T, W, (int)w_nr, (long)M, (int)N, (int)r, alpha, aligned);
    else LORA_BY_RANK(lora_up_kernel, float, r, grid, block, 0, stream, (float*)y, (long)ldy, T, W, (int)w_nr, (long)M, (int)N, (int)r, alpha, aligned);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_lora_wgrad(const float* T, const void* X, int64_t ldx, int64_t x_off, int32_t dtype, float* G, int32_t g_cr, int64_t M, int32_t C, int32_t r,
                             float alpha, float* ws, void* stream_) {
    PB_REQUIRE(dtype == PB_BF16 || dtype == PB_F32, "pb_lora_wgrad: dtype = %d (PB_F32 or PB_BF16)", (int)dtype);
    PB_REQUIRE(rank_ok(r), "pb_lora_wgrad: r = %d (a multiple of 4 in 4 .. 64)", (int)r);
    PB_REQUIRE(M >= 0 && M <= L_MAX_M, "pb_lora_wgrad: M = %lld (0 .. 2^24 rows)", (long long)M);
    PB_REQUIRE(C >= 1 && C <= L_MAX_DIM, "pb_lora_wgrad: C = %d (1 .. 2^20 columns)", (int)C);
    PB_REQUIRE(x_off >= 0 && ldx >= x_off + C, "pb_lora_wgrad: ldx = %lld is below x_off + C = %lld + %d", (long long)ldx, (long long)x_off, (int)C);
    PB_REQUIRE(g_cr == 0 || g_cr == 1, "pb_lora_wgrad: g_cr = %d (0: G is (r, C), 1: G is (C, r))", (int)g_cr);
    const int esz = dtype == PB_BF16 ? 2 : 4;
    PB_REQUIRE(elem_ptr(X, esz), "pb_lora_wgrad: X must be a non-NULL pointer aligned to its element");
    PB_REQUIRE(f32_ok(T), "pb_lora_wgrad: T must be a non-NULL f32 pointer");
    PB_REQUIRE(f32_ok(G), "pb_lora_wgrad: G must be a non-NULL f32 pointer");
    PB_REQUIRE(ws && ((uintptr_t)ws % 16 == 0), "pb_lora_wgrad: ws must be pb_lora_wgrad_ws_floats(M, r, C) floats, 16-byte aligned");
    PB_REQUIRE((const void*)G != X && G != T && G != ws && (const void*)ws != X && ws != T, "pb_lora_wgrad: T, X, G and ws must be distinct buffers");
    if (M == 0) return 0;
    const char* x = (const char*)X + x_off * esz;
    const int aligned = vec_ok(x, ldx, esz);
    const WgradSplit sp = wgrad_split((long)M, r);
    const int cols = 16 * (16 / esz);
    const dim3 grid((unsigned)((sp.nsplit + 3) / 4), (unsigned)((C + cols - 1) / cols)), block(L_THREADS);
    hipStream_t stream = (hipStream_t)stream_;
    if (dtype == PB_BF16) LORA_BY_RANK(lora_wgrad_kernel, bf16_t, r, grid, block, 0, stream, T, (const bf16_t*)x, (long)ldx, (long)M, (int)C, (int)r, sp.chunk, sp.nsplit, aligned, ws);
    else LORA_BY_RANK(lora_wgrad_kernel, float, r, grid, block, 0, stream, T, (const float*)x, (long)ldx, (long)M, (int)C, (int)r, sp.chunk, sp.nsplit, aligned, ws);
    PB_LAUNCH_CHECK();
    const long n_el = (long)r * C;
    hipLaunchKernelGGL(lora_wgrad_fold_kernel, dim3((unsigned)std::min(1024L, (n_el + L_THREADS - 1) / L_THREADS)), block, 0, stream, (const float*)ws, sp.nsplit, G, (int)g_cr,
                       (int)C, (int)r, alpha);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_lora_merge(float* W, const float* B, const float* A, int64_t N, int32_t K, int32_t r, float alpha, void* stream_) {
    PB_REQUIRE(rank_ok(r), "pb_lora_merge: r = %d (a multiple of 4 in 4 .. 64)", (int)r);
    PB_REQUIRE(N >= 0 && N <= L_MAX_M, "pb_lora_merge: N = %lld (0 .. 2^24 rows)", (long long)N);
    PB_REQUIRE(K >= 1 && K <= L_MAX_DIM, "pb_lora_merge: K = %d (1 .. 2^20 columns)", (int)K);
    PB_REQUIRE(f32_ok(W), "pb_lora_merge: W must be a non-NULL f32 pointer");
    PB_REQUIRE(f32_ok(B), "pb_lora_merge: B must be a non-NULL f32 pointer");
    PB_REQUIRE(f32_ok(A), "pb_lora_merge: A must be a non-NULL f32 pointer");
    PB_REQUIRE(W != B && W != A, "pb_lora_merge: W must not alias A or B");
    if (N == 0) return 0;
    const int aligned = vec_ok(W, K, 4) && vec_ok(A, K, 4);
    const long n_el = (long)N * ((K + 3) / 4);
    hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)std::min(4096L, (n_el + L_THREADS - 1) / L_THREADS)), dim3(L_THREADS), 0, (hipStream_t)stream_, W, B, A, (long)N, (int)K,
                       (int)r, alpha, aligned);
    PB_LAUNCH_CHECK();
    return 0;
}
