// K25: Fisher merging (the reference's model_merging_methods/merging_methods.py:82-264) on flat f32 vectors. Five entries:
//   fisher_rows_kernel     per logits row: E = sum_c sqrt(p_c) log p_c and dE/dz scaled by a row weight (one wave per row, ce_rows_kernel's form)
//   fisher_accum_kernel    F += g * g over the engine's whole flat gradient buffer, once per batch
//   fisher_finish_kernel   F /= num_computed; flags |= 1 where a result is not finite
//   fisher_norm_*          float32(sqrt(sum F^2)), the sum in float64 in an order that depends on n alone (no float atomics)
//   fisher_merge_kernel    out = sum_m (c_m (F_m + minimal)) W_m / sum_m c_m (F_m + minimal), one fused pass over up to 8 + 8 vectors
// The streaming kernels have pb_merge.hip's shape: f32x4 per lane, grid-stride, <= 2048 workgroups, pointers that are segments of flat
// buffers (scalar head and tail by workgroup 0; pointers offset differently from a 16-byte boundary go scalar throughout).
// Bit parity with the reference's CPU tensors needs every float32 operation rounded once: build.py compiles THIS file with
// -ffp-contract=off (FILE_FLAGS), and tests/test_fisher_cpu.py looks for fused multiply-adds in its code.
#include "pb_common.h"
#include "pb_api_internal.h"
#include <algorithm>

namespace {

constexpr int FS_BLOCKS = 2048, FS_THREADS = 256, FS_MAX = PB_MERGE_MAX_MODELS;

// ---- rows ---------------------------------------------------------------------------------------------------------------------------
// p = softmax(z); E = sum_c sqrt(p_c) log p_c with log p_c = (z_c - max) - log(sum); a class whose p underflows to 0 adds 0 (never 0 * -inf).
// dE/dz_j with sqrt(p) held constant (the reference detaches it): d_j = sqrt(p_j) - p_j S, S = sum_c sqrt(p_c); written times weight[row].
__global__ __launch_bounds__(256) void fisher_rows_kernel(const float* __restrict__ logits, const float* __restrict__ weight, float* __restrict__ e_out,
                                                         float* __restrict__ dlogits, long rows, int C) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* lr = logits + row * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, lr[c]);
    const float wm = wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(lr[c] - wm);
    sum = wave_sum(sum);
    const float lsum = logf(sum), inv = 1.0f / sum;
    float e = 0.f, s = 0.f;
    for (int c = lane; c < C; c += 64) {
        const float t = lr[c] - wm, p = expf(t) * inv;
        if (p > 0.f) { const float r = sqrtf(p); e += r * (t - lsum); s += r; }
    }
    e = wave_sum(e);
    s = wave_sum(s);
    if (lane == 0) e_out[row] = e;
    if (dlogits) {
        const float w = weight ? weight[row] : 1.0f;
        for (int c = lane; c < C; c += 64) {
            const float p = expf(lr[c] - wm) * inv;
            dlogits[row * C + c] = w == 0.f ? 0.f : w * (sqrtf(p) - p * s);
        }
    }
}

// ---- F += g g, F /= divisor ----------------------------------------------------------------------------------------------------------
// [0, head) scalar | [head, head + 4 n4) as n4 vectors (VEC) or scalars | [head + 4 n4, n) scalar
template <bool VEC>
__global__ __launch_bounds__(FS_THREADS) void fisher_accum_kernel(float* __restrict__ F, const float* __restrict__ g, long n, long head, long n4) {
    const long tid = (long)blockIdx.x * FS_THREADS + threadIdx.x, stride = (long)gridDim.x * FS_THREADS;
    float* f = F + head;
    const float* s = g + head;
    if (VEC) {
        for (long i = tid; i < n4; i += stride) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(s + 4 * i);
            *reinterpret_cast<f32x4*>(f + 4 * i) = *reinterpret_cast<const f32x4*>(f + 4 * i) + v * v;
        }
    } else {
        for (long i = tid; i < 4 * n4; i += stride) f[i] = f[i] + s[i] * s[i];
    }
    if (blockIdx.x == 0) {
        const long body_end = head + 4 * n4;
        long i = -1;
        if ((long)threadIdx.x < head) i = threadIdx.x;                                             // head: lanes 0 .. 2
        else if (threadIdx.x >= 64 && body_end + (threadIdx.x - 64) < n) i = body_end + (threadIdx.x - 64);    // tail: lanes 64 .. 66
        if (i >= 0) F[i] = F[i] + g[i] * g[i];
    }
}

__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(FS_THREADS) void fisher_finish_kernel(float* __restrict__ F, long n, long head, long n4, float divisor, int32_t* __restrict__ flags) {
    const long tid = (long)blockIdx.x * FS_THREADS + threadIdx.x, stride = (long)gridDim.x * FS_THREADS;
    float* f = F + head;
    bool bad = false;
    for (long i = tid; i < n4; i += stride) {
        f32x4 v = *reinterpret_cast<const f32x4*>(f + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = v[j] / divisor; bad |= !finite_f(v[j]); }
        *reinterpret_cast<f32x4*>(f + 4 * i) = v;
    }
    if (blockIdx.x == 0) {
        const long body_end = head + 4 * n4;
        long i = -1;
        if ((long)threadIdx.x < head) i = threadIdx.x;
        else if (threadIdx.x >= 64 && body_end + (threadIdx.x - 64) < n) i = body_end + (threadIdx.x - 64);
        if (i >= 0) { const float v = F[i] / divisor; F[i] = v; bad |= !finite_f(v); }
    }
    if (bad) atomicOr(flags, 1);
}

// ---- norm -----------------------------------------------------------------------------------------------------------------------------
// Item i holds elements 4 i .. 4 i + 3 of F (the last item may be short), whatever F's alignment: thread t of the grid sums the squares
// of items t, t + stride, .. in float64, a workgroup folds its 256 sums by a fixed tree into ITS slot of ws, and one workgroup folds the
// slots the same way. The grid is a function of n, so the order of every addition is too.
__device__ __forceinline__ double block_fold(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = FS_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

template <bool VEC>
__global__ __launch_bounds__(FS_THREADS) void fisher_norm_partial_kernel(const float* __restrict__ F, long n, double* __restrict__ ws) {
    __shared__ double red[FS_THREADS];
    const long tid = (long)blockIdx.x * FS_THREADS + threadIdx.x, stride = (long)gridDim.x * FS_THREADS;
    const long items = (n + 3) >> 2;
    double acc = 0.0;
    for (long i = tid; i < items; i += stride) {
        const long e = 4 * i;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (VEC && e + 4 <= n) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(F + e);
            v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (e + j < n) v[j] = F[e + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = acc + (double)v[j] * (double)v[j];
    }
    const double total = block_fold(acc, red);
    if (threadIdx.x == 0) ws[blockIdx.x] = total;
}

__global__ __launch_bounds__(FS_THREADS) void fisher_norm_final_kernel(const double* __restrict__ ws, int nparts, float* __restrict__ norm_out) {
    __shared__ double red[FS_THREADS];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += FS_THREADS) acc = acc + ws[i];
    const double total = block_fold(acc, red);
    if (threadIdx.x == 0) norm_out[0] = (float)sqrt(total);
}

// ---- the fused weighted pass -------------------------------------------------------------------------------------------------------------
struct FisherArgs {
    float* out;
    const float* model[FS_MAX];
    const float* fisher[FS_MAX];
    long n, head, n4;
    float coef[FS_MAX];
    float minimal;
    int n_models;
};

// num = ((0 + (c_0 Fp_0) W_0) + (c_1 Fp_1) W_1) + ..; den = ((0 + c_0 Fp_0) + c_1 Fp_1) + ..; Fp_m = F_m + minimal (torch's sum over the
// model axis starts at +0 and goes left to right)
__device__ __forceinline__ float fisher_one(const FisherArgs& a, const float (&w)[FS_MAX], const float (&f)[FS_MAX]) {
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int m = 0; m < FS_MAX; ++m) {
        if (m < a.n_models) {
            const float cf = a.coef[m] * (f[m] + a.minimal);
            num = num + cf * w[m];
            den = den + cf;
        }
    }
    return num / den;
}

template <bool VEC>
__global__ __launch_bounds__(FS_THREADS) void fisher_merge_kernel(const FisherArgs a) {
    const long tid = (long)blockIdx.x * FS_THREADS + threadIdx.x, stride = (long)gridDim.x * FS_THREADS;
    if (VEC) {
        for (long i = tid; i < a.n4; i += stride) {
            const long e = a.head + 4 * i;
            f32x4 wv[FS_MAX], fv[FS_MAX];
#pragma unroll
            for (int m = 0; m < FS_MAX; ++m) {
                if (m < a.n_models) {
                    wv[m] = *reinterpret_cast<const f32x4*>(a.model[m] + e);
                    fv[m] = *reinterpret_cast<const f32x4*>(a.fisher[m] + e);
                }
            }
            f32x4 ov;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float w[FS_MAX], f[FS_MAX];
#pragma unroll
                for (int m = 0; m < FS_MAX; ++m) { w[m] = m < a.n_models ? wv[m][j] : 0.f; f[m] = m < a.n_models ? fv[m][j] : 0.f; }
                ov[j] = fisher_one(a, w, f);
            }
            *reinterpret_cast<f32x4*>(a.out + e) = ov;
        }
    }
    auto scalar = [&](long e) {
        float w[FS_MAX], f[FS_MAX];
#pragma unroll
        for (int m = 0; m < FS_MAX; ++m) { w[m] = m < a.n_models ? a.model[m][e] : 0.f; f[m] = m < a.n_models ? a.fisher[m][e] : 0.f; }
        a.out[e] = fisher_one(a, w, f);
    };
    if (!VEC) for (long i = tid; i < 4 * a.n4; i += stride) scalar(a.head + i);
    if (blockIdx.x == 0) {
        const long body_end = a.head + 4 * a.n4;
        if ((long)threadIdx.x < a.head) scalar(threadIdx.x);
        else if (threadIdx.x >= 64 && body_end + (threadIdx.x - 64) < a.n) scalar(body_end + (threadIdx.x - 64));
    }
}

void split_range(const void* lead, long n, long& head, long& n4) {
    head = std::min<long>(n, (long)(((16 - ((uintptr_t)lead & 15)) & 15) / 4));
    n4 = (n - head) >> 2;
}
bool aligned_at(const float* p, long head) { return (((uintptr_t)(p + head)) & 15) == 0; }
int grid_for(long items) { return (int)std::max(1L, std::min((long)FS_BLOCKS, (items + FS_THREADS - 1) / FS_THREADS)); }
bool f32_ptr(const void* p) { return p && ((uintptr_t)p % 4 == 0); }

}  // namespace

extern "C" int64_t pb_fisher_desc_bytes(void) { return (int64_t)sizeof(pb_fisher_desc); }
extern "C" int64_t pb_fisher_norm_ws_bytes(void) { return (int64_t)(FS_BLOCKS * sizeof(double)); }

extern "C" int pb_fisher_rows(const float* logits, const float* weight, float* e_out, float* dlogits, int64_t rows, int32_t C, void* stream_) {
    PB_REQUIRE(rows >= 0 && C >= 1, "pb_fisher_rows: rows = %lld, C = %d (need rows >= 0, C >= 1)", (long long)rows, (int)C);
    PB_REQUIRE(rows <= 4ll * 0x7fffffff, "pb_fisher_rows: rows = %lld exceeds the grid", (long long)rows);
    if (rows == 0) return 0;
    PB_REQUIRE(f32_ptr(logits) && f32_ptr(e_out), "pb_fisher_rows: logits and e_out must be non-NULL f32 pointers");
    PB_REQUIRE(((uintptr_t)weight % 4 == 0) && ((uintptr_t)dlogits % 4 == 0), "pb_fisher_rows: weight / dlogits need 4-byte alignment");
    PB_REQUIRE(dlogits != logits, "pb_fisher_rows: dlogits aliases logits");
    hipLaunchKernelGGL(fisher_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, logits, weight, e_out, dlogits, (long)rows, (int)C);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_fisher_accum(float* F, const float* g, int64_t n, void* stream_) {
    PB_REQUIRE(n >= 0, "pb_fisher_accum: n = %lld", (long long)n);
    if (n == 0) return 0;
    PB_REQUIRE(f32_ptr(F) && f32_ptr(g), "pb_fisher_accum: F and g must be non-NULL f32 pointers");
    PB_REQUIRE(F != g, "pb_fisher_accum: F aliases g");
    long head, n4;
    split_range(F, (long)n, head, n4);
    const bool vec = aligned_at(g, head);
    const int grid = grid_for(vec ? n4 : 4 * n4);
    if (vec) hipLaunchKernelGGL(fisher_accum_kernel<true>, dim3(grid), dim3(FS_THREADS), 0, (hipStream_t)stream_, F, g, (long)n, head, n4);
    else hipLaunchKernelGGL(fisher_accum_kernel<false>, dim3(grid), dim3(FS_THREADS), 0, (hipStream_t)stream_, F, g, (long)n, head, n4);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_fisher_finish(float* F, int64_t n, int64_t divisor, int32_t* flags, void* stream_) {
    PB_REQUIRE(n >= 0, "pb_fisher_finish: n = %lld", (long long)n);
    PB_REQUIRE(divisor >= 1 && divisor <= (1ll << 24), "pb_fisher_finish: divisor = %lld (the examples computed: 1 .. 2^24, exact in float32)", (long long)divisor);
    PB_REQUIRE(flags && ((uintptr_t)flags % 4 == 0), "pb_fisher_finish: flags must be a device int32");
    if (n == 0) return 0;
    PB_REQUIRE(f32_ptr(F), "pb_fisher_finish: F must be a non-NULL f32 pointer");
    long head, n4;
    split_range(F, (long)n, head, n4);
    hipLaunchKernelGGL(fisher_finish_kernel, dim3(grid_for(n4)), dim3(FS_THREADS), 0, (hipStream_t)stream_, F, (long)n, head, n4, (float)divisor, flags);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_fisher_norm(const float* F, int64_t n, void* ws, float* norm_out, void* stream_) {
    PB_REQUIRE(n >= 1, "pb_fisher_norm: n = %lld (need n >= 1)", (long long)n);
    PB_REQUIRE(f32_ptr(F) && f32_ptr(norm_out), "pb_fisher_norm: F and norm_out must be non-NULL f32 pointers");
    PB_REQUIRE(ws && ((uintptr_t)ws % 8 == 0), "pb_fisher_norm: ws must be pb_fisher_norm_ws_bytes() bytes, 8-byte aligned");
    const int grid = grid_for(((long)n + 3) >> 2);
    if (((uintptr_t)F & 15) == 0) hipLaunchKernelGGL(fisher_norm_partial_kernel<true>, dim3(grid), dim3(FS_THREADS), 0, (hipStream_t)stream_, F, (long)n, (double*)ws);
    else hipLaunchKernelGGL(fisher_norm_partial_kernel<false>, dim3(grid), dim3(FS_THREADS), 0, (hipStream_t)stream_, F, (long)n, (double*)ws);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(fisher_norm_final_kernel, dim3(1), dim3(FS_THREADS), 0, (hipStream_t)stream_, (const double*)ws, grid, norm_out);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_fisher_merge(const pb_fisher_desc* d, void* stream_) {
    PB_REQUIRE(d, "pb_fisher_merge: NULL descriptor");
    PB_REQUIRE(d->n >= 0, "pb_fisher_merge: n = %lld", (long long)d->n);
    PB_REQUIRE(d->n_models >= 2 && d->n_models <= FS_MAX, "pb_fisher_merge: n_models = %d (2 .. %d models)", (int)d->n_models, FS_MAX);
    PB_REQUIRE(f32_ptr(d->out), "pb_fisher_merge: out must be a non-NULL f32 pointer");
    PB_REQUIRE(d->minimal > 0.f && d->minimal < INFINITY, "pb_fisher_merge: minimal = %g must be positive and finite", (double)d->minimal);
    FisherArgs a = {};
    a.out = d->out; a.n = (long)d->n; a.n_models = d->n_models; a.minimal = d->minimal;
    split_range(d->out, a.n, a.head, a.n4);
    bool vec = true;
    for (int m = 0; m < d->n_models; ++m) {
        PB_REQUIRE(f32_ptr(d->model[m]), "pb_fisher_merge: model[%d] must be a non-NULL f32 pointer", m);
        PB_REQUIRE(f32_ptr(d->fisher[m]), "pb_fisher_merge: fisher[%d] must be a non-NULL f32 pointer", m);
        PB_REQUIRE(d->model[m] != d->out && d->fisher[m] != d->out, "pb_fisher_merge: out aliases model[%d] or fisher[%d]", m, m);
        PB_REQUIRE(d->coef[m] > 0.f && d->coef[m] < INFINITY, "pb_fisher_merge: coef[%d] = %g must be positive and finite", m, (double)d->coef[m]);
        a.model[m] = d->model[m]; a.fisher[m] = d->fisher[m]; a.coef[m] = d->coef[m];
        vec = vec && aligned_at(d->model[m], a.head) && aligned_at(d->fisher[m], a.head);
    }
    if (a.n == 0) return 0;
    const int grid = grid_for(vec ? a.n4 : 4 * a.n4);
    if (vec) hipLaunchKernelGGL(fisher_merge_kernel<true>, dim3(grid), dim3(FS_THREADS), 0, (hipStream_t)stream_, a);
    else hipLaunchKernelGGL(fisher_merge_kernel<false>, dim3(grid), dim3(FS_THREADS), 0, (hipStream_t)stream_, a);
    PB_LAUNCH_CHECK();
    return 0;
}
