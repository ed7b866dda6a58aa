// K28: K9 (pb_loss.hip) with soft targets. Per token row and head the fused log-softmax + cross-entropy + argmax + masked accuracy
// of K9, mixed with the KL divergence to a teacher's softened distribution (knowledge distillation) and / or with label smoothing,
// and the gradient w.r.t. the student's logits in the same pass. include/pianobart_hip.h has the formulas.
// One wave64 per student row; lane l holds classes l, l + 64, ... of a head of the student's row AND of the teacher's row (head starts
// are not 16-byte aligned in a logits row, so the coalesced form is one dword per lane: 256 contiguous bytes per wave instruction);
// every max / sum is a VALU-only wave reduction (pb_common.h); lane i < 8 carries head i's scalars and running sums.
// Two forms share one per-head routine (same arithmetic, same summation order, hence the same bits):
//   register-resident   every head <= 64 * DK_REG = 320 classes: both rows are loaded once, 2 x 40 loads per lane in flight together
//   general             heads up to 64 * DK_WIDE = 1088 classes: one head of both rows at a time, 2 x 17 values per lane
#include "pb_common.h"
#include "pb_api_internal.h"
#include <math.h>

namespace {

struct DSeg9 { int off[9]; };
struct DArgs {
    float one_m_alpha;      // 1 - alpha
    float soft_w;           // alpha * tau      (gradient of the soft part)
    float kl_w;             // alpha * tau^2    (loss of the soft part)
    float inv_tau;
    float one_m_eps;        // 1 - eps
    float eps_n[8];         // eps / n_i
};
constexpr int D_MAX_BLOCKS = 2048;
constexpr int D_PLANES = 5;                 // loss, m, correct, hard, kl
constexpr int D_SUMS = D_PLANES * 8;
constexpr int DK_REG = 5, DK_WIDE = 17;

struct HeadOut { float loss, hard, kl; int am; };

// e^x for x <= 0 to about one ulp: the product x log2(e) carries its rounding error and the low half of the constant into a first-order
// correction (__expf rounds the product and loses |x| 2^-24 of relative accuracy; two softmaxes meet in p_tau - q, and their errors add)
__device__ __forceinline__ float exp_acc(float x) {
    const float hi = 1.44269502162933349609375f, lo = 1.925963033500011e-08f;
    const float t = x * hi;
    const float r = fmaf(x, lo, fmaf(x, hi, -t));
    const float e = __builtin_amdgcn_exp2f(t);
    return fmaf(e, r * 0.693147180559945f, e);
}
// e / s from is = 1 / s with one correction step: the correctly rounded quotient but for rare double-rounding cases
__device__ __forceinline__ float quot(float e, float s, float is) {
    const float q = e * is;
    return fmaf(fmaf(-q, s, e), is, q);
}

// wave64 sum of a double, every lane the same bits (xor butterfly). One such sum per head and row: the KL is the small difference of sums
// of magnitude sum_c q_c (|log q_c| + |log p_tau,c|), so its three sums are kept in float64 and its rounding error is the final cast's
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) v += __shfl_xor(v, sft, 64);
    return v;
}

// One head of one row. v / u: the lane's classes lane + 64 k of the student's / teacher's row (-inf past the head's n classes; u is not
// read without a teacher). xt: the target's logit (0 for a target outside the head). kk = coef * m scales the gradient written to g
// (NULL: no gradient).
template <typename T, int K>
__device__ __forceinline__ HeadOut head_step(const float (&v)[K], const float (&u)[K], const bool has_t, const int n, const int lane, const int tgt,
                                             const float xt, const float kk, const DArgs& a, const float eps_n, T* __restrict__ g) {
    HeadOut r;
    float mx = v[0];
#pragma unroll
    for (int k = 1; k < K; ++k) mx = fmaxf(mx, v[k]);
    mx = wave_max(mx);
    // first index attaining the maximum (np.argmax tie rule): class ids < 2^24 are exact in f32
    float neg_first = -16777216.f;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) neg_first = v[k] == mx ? -(float)(lane + 64 * k) : neg_first;
    r.am = (int)(-wave_max(neg_first));
    float e[K], se = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        e[k] = lane + 64 * k < n ? __expf(v[k] - mx) : 0.f;
        se += e[k];                                             // K9's per-lane order
    }
    se = wave_sum(se);
    const float lse = logf(se);
    r.hard = lse + mx - xt;                                     // -log p[y]
    float hard_e = r.hard;
    if (a.one_m_eps != 1.0f) {                                  // label smoothing: -(eps / n) sum_c log p[c] = (eps / n) (sum_c (mx - x_c) + n lse), all terms >= 0
        float sd = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) sd += lane + 64 * k < n ? mx - v[k] : 0.f;
        sd = wave_sum(sd);
        hard_e = a.one_m_eps * r.hard + eps_n * (sd + (float)n * lse);
    }
    float et[K], eq[K], isp = 0.f, isq = 0.f, sp = 1.f, sq = 1.f;
    r.kl = 0.f;
    if (has_t) {
        // p_tau = softmax(z / tau) and q = softmax(u / tau), each on its own maximum: (x - max) / tau <= 0 whatever the quotients reach
        float mu = u[0];
#pragma unroll
        for (int k = 1; k < K; ++k) mu = fmaxf(mu, u[k]);
        mu = wave_max(mu);
        double dsp = 0.0, dsq = 0.0, dot = 0.0;
        const double itau = (double)a.inv_tau;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const bool in = lane + 64 * k < n;
            const double bt = ((double)v[k] - (double)mx) * itau, at = ((double)u[k] - (double)mu) * itau;
            et[k] = in ? exp_acc((float)bt) : 0.f;
            eq[k] = in ? exp_acc((float)at) : 0.f;
            dsp += (double)et[k];
            dsq += (double)eq[k];
            dot += in ? (double)eq[k] * (at - bt) : 0.0;        // q == 0 (underflow): 0 * finite = 0
        }
        dsp = wave_sum_d(dsp); dsq = wave_sum_d(dsq); dot = wave_sum_d(dot);
        // sum_c q_c (log q_c - log p_tau,c), log q_c = at_c - log sq, log p_tau,c = bt_c - log sp, sum_c q_c = 1: exactly the KL of the
        // distributions eq / sq and et / sp that the gradient uses, and exactly 0 when the two rows agree
        sp = (float)dsp; sq = (float)dsq;
        isp = 1.0f / sp; isq = 1.0f / sq;
        r.kl = (float)(dot / dsq + (log(dsp) - log(dsq)));
    }
    r.loss = a.one_m_alpha * hard_e + a.kl_w * r.kl;
    if (g) {
        const float inv = 1.0f / se;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = lane + 64 * k;
            if (c < n) {
                float d = a.one_m_alpha * (e[k] * inv - (c == tgt ? a.one_m_eps : 0.f) - eps_n);
                // p_tau - q: two quotients by the same instructions, so exactly 0 when the two rows agree
                if (has_t) d += a.soft_w * (quot(et[k], sp, isp) - quot(eq[k], sq, isq));
                g[c] = from_f<T>(kk * d);
            }
        }
    }
    return r;
}

// the lane's own head scalars (lane i < 8: head i): offset of head `lane` without indexing the argument struct by a register
__device__ __forceinline__ void lane_head(const DSeg9& so, int lane, int& o, int& n) {
    o = 0; n = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { o = lane == i ? so.off[i] : o; n = lane == i ? so.off[i + 1] - so.off[i] : n; }
}

template <typename T, int K, bool RESIDENT>
__global__ __launch_bounds__(256) void distill_kernel(const float* __restrict__ logits, const float* __restrict__ teacher, const int32_t* __restrict__ t_row,
        const int16_t* __restrict__ target, const float* __restrict__ loss_mask, const DSeg9 so, const DArgs a, float* __restrict__ partials,
        const float* __restrict__ coef, T* __restrict__ dlogits, int16_t* __restrict__ argmax_out, int rows, int rows_t, int V) {
    __shared__ float red[4][D_SUMS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool has_t = teacher != nullptr;
    float acc[D_PLANES] = {0.f, 0.f, 0.f, 0.f, 0.f};            // lane i < 8: running sums of head i
    int my_o, my_n;
    lane_head(so, lane, my_o, my_n);
    const float my_coef = (dlogits && lane < 8) ? coef[lane] : 0.f;
    for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
        const float* x = logits + row * V;
        // the teacher's row: t_row[row], or the same row. A row number outside the teacher's rows_t rows is not read: its logits count
        // as NaN, and so does everything computed from them
        const long tr = t_row ? (long)t_row[row] : row;
        const bool t_ok = has_t && tr >= 0 && tr < rows_t;
        const float* ux = teacher + (t_ok ? tr : 0) * V;
        int my_t = 0; float my_m = 0.f, my_xt = 0.f;
        if (lane < 8) {
            my_t = target[row * 8 + lane];
            my_m = loss_mask[row * 8 + lane];
            if (my_t >= 0 && my_t < my_n) my_xt = x[my_o + my_t];       // a target outside its head scores a logit of 0, as in K9
        }
        float v[RESIDENT ? 8 : 1][K], u[RESIDENT ? 8 : 1][K];
        if constexpr (RESIDENT) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int o = so.off[i], n = so.off[i + 1] - o;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int c = lane + 64 * k;
                    v[i][k] = c < n ? x[o + c] : -INFINITY;
                    u[i][k] = !has_t ? 0.f : c < n ? (t_ok ? ux[o + c] : NAN) : -INFINITY;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = so.off[i], n = so.off[i + 1] - o;
            const int hs = RESIDENT ? i : 0;
            if constexpr (!RESIDENT) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int c = lane + 64 * k;
                    v[0][k] = c < n ? x[o + c] : -INFINITY;
                    u[0][k] = !has_t ? 0.f : c < n ? (t_ok ? ux[o + c] : NAN) : -INFINITY;
                }
            }
            const int tgt = __builtin_amdgcn_readlane(my_t, i);
            const float m = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_m), i));
            const float xt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_xt), i));
            // kk = coef * m multiplies: a head without any loss position has coef = inf, inf * 0 = NaN, exactly where K9 has it
            const float kk = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_coef), i)) * m;
            const HeadOut r = head_step<T, K>(v[hs], u[hs], has_t, n, lane, tgt, xt, kk, a, a.eps_n[i], dlogits ? dlogits + row * V + o : nullptr);
            if (lane == i) {
                acc[0] += r.loss * m; acc[1] += m; acc[2] += (r.am == tgt ? 1.f : 0.f) * m; acc[3] += r.hard * m; acc[4] += r.kl * m;
                if (argmax_out) argmax_out[row * 8 + i] = (int16_t)r.am;
            }
        }
    }
    if (lane < 8) {
#pragma unroll
        for (int p = 0; p < D_PLANES; ++p) red[wave][8 * p + lane] = acc[p];
    }
    __syncthreads();
    if (threadIdx.x < D_SUMS)
        partials[(size_t)blockIdx.x * D_SUMS + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// 40 sums over the block partials in a fixed order: 16 row groups x 64 columns, 4 independent loads in flight per thread, then an LDS tree
__global__ __launch_bounds__(1024) void distill_finalize_kernel(const float* __restrict__ partials, int nblk, float* __restrict__ sums) {
    __shared__ float red[16][64];
    const int k = threadIdx.x & 63, rg = threadIdx.x >> 6;
    float s = 0.f;
    if (k < D_SUMS) {
        int b = rg;
        for (; b + 3 * 16 < nblk; b += 4 * 16) {
            float t[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) t[q] = partials[(size_t)(b + 16 * q) * D_SUMS + k];
            s += (t[0] + t[1]) + (t[2] + t[3]);
        }
        for (; b < nblk; b += 16) s += partials[(size_t)b * D_SUMS + k];
    }
    red[rg][k] = s;
    __syncthreads();
    if (rg < 4) red[rg][k] = (red[rg][k] + red[rg + 4][k]) + (red[rg + 8][k] + red[rg + 12][k]);
    __syncthreads();
    if (rg == 0 && k < D_SUMS) sums[k] += (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
}

template <typename O>
void launch_distill(bool resident, int grid, hipStream_t stream, const float* logits, const float* teacher, const int32_t* t_row, const int16_t* target,
                    const float* loss_mask, const DSeg9& so, const DArgs& a, float* partials, const float* coef, void* dlogits, int16_t* argmax_out, int T,
                    int T_t, int V) {
    if (resident)
        hipLaunchKernelGGL((distill_kernel<O, DK_REG, true>), dim3(grid), dim3(256), 0, stream, logits, teacher, t_row, target, loss_mask, so, a, partials, coef,
                           (O*)dlogits, argmax_out, T, T_t, V);
    else
        hipLaunchKernelGGL((distill_kernel<O, DK_WIDE, false>), dim3(grid), dim3(256), 0, stream, logits, teacher, t_row, target, loss_mask, so, a, partials, coef,
                           (O*)dlogits, argmax_out, T, T_t, V);
}

}  // namespace

extern "C" int64_t pb_distill_partials_floats(void) { return (int64_t)D_MAX_BLOCKS * D_SUMS; }

extern "C" int pb_distill_fwd_bwd(const float* logits, const float* teacher, const int32_t* t_row, const int16_t* target, const float* loss_mask,
                                  const int32_t* seg_off, float* sums, float* partials, const float* coef, void* dlogits, int16_t* argmax_out, int32_t T,
                                  int32_t T_t, int32_t V, int32_t dtype, float alpha, float tau, float eps, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PB_REQUIRE(alpha >= 0.f && alpha <= 1.f, "pb_distill_fwd_bwd: alpha = %g lies outside [0, 1]", (double)alpha);
    PB_REQUIRE(eps >= 0.f && eps < 1.f, "pb_distill_fwd_bwd: eps = %g lies outside [0, 1)", (double)eps);
    PB_REQUIRE(tau > 0.f && std::isfinite(tau), "pb_distill_fwd_bwd: tau = %g must be finite and > 0", (double)tau);
    PB_REQUIRE(alpha == 0.f || teacher != nullptr, "pb_distill_fwd_bwd: alpha = %g > 0 needs teacher logits (teacher is NULL)", (double)alpha);
    PB_REQUIRE(seg_off[8] == V && seg_off[0] == 0, "pb_distill_fwd_bwd: segment offsets (seg_off) do not cover V=%d", V);
    PB_REQUIRE(dlogits == nullptr || coef != nullptr, "pb_distill_fwd_bwd: dlogits needs coef");
    PB_REQUIRE(dtype == PB_F32 || dtype == PB_BF16, "pb_distill_fwd_bwd: dtype %d (dlogits is f32 or bf16)", dtype);
    bool resident = true;
    for (int i = 0; i < 8; ++i) {
        const int n = seg_off[i + 1] - seg_off[i];
        PB_REQUIRE(n >= 1 && n <= 64 * DK_WIDE, "pb_distill_fwd_bwd: seg_off gives head %d %d classes (1 .. %d)", i, n, 64 * DK_WIDE);
        resident = resident && n <= 64 * DK_REG;
    }
    PB_REQUIRE(teacher == nullptr || t_row != nullptr || T_t >= T, "pb_distill_fwd_bwd: T_t = %d teacher rows for T = %d rows without t_row", T_t, T);
    if (T <= 0) return 0;
    DSeg9 so;
    for (int i = 0; i < 9; ++i) so.off[i] = seg_off[i];
    DArgs a;
    a.one_m_alpha = (float)(1.0 - (double)alpha);
    a.soft_w = (float)((double)alpha * (double)tau);
    a.kl_w = (float)((double)alpha * (double)tau * (double)tau);
    a.inv_tau = (float)(1.0 / (double)tau);
    a.one_m_eps = (float)(1.0 - (double)eps);
    for (int i = 0; i < 8; ++i) a.eps_n[i] = (float)((double)eps / (double)(seg_off[i + 1] - seg_off[i]));
    const int grid = std::max(1, std::min(D_MAX_BLOCKS, (T + 3) / 4));
    if (dtype == PB_BF16)
        launch_distill<bf16_t>(resident, grid, stream, logits, teacher, t_row, target, loss_mask, so, a, partials, coef, dlogits, argmax_out, T, T_t, V);
    else
        launch_distill<float>(resident, grid, stream, logits, teacher, t_row, target, loss_mask, so, a, partials, coef, dlogits, argmax_out, T, T_t, V);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(1024), 0, stream, partials, grid, sums);
    PB_LAUNCH_CHECK();
    return 0;
}
