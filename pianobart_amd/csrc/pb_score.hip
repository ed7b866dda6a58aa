// K16: teacher-forced scoring rows. pb_token_scores: per token and head the log-probability of a given target, the entropy of the
// head's softmax and the target's rank, from the (T, V) f32 logits that pb_ce_fwd_bwd reads (the forward-only quantity the
// reference's Ablation.py:126-166 evaluates; K9 keeps only its 24 batch-wide sums). pb_seq_scores: their per-sequence sums.
// One wave64 per token row in the register-resident layout of ce_rows_reg_kernel (pb_loss.hip): the row is loaded once, lane l holds
// classes l, l + 64, ... of every head, the reductions are VALU-only (pb_common.h); lane i < 8 carries head i's results to one
// 32-byte store per output.
#include "pb_common.h"
#include "pb_api_internal.h"

namespace {

struct Seg9 { int off[9]; };
constexpr int SC_K = 5;                     // the register form: heads of at most 64 * SC_K = 320 classes (the default dictionary's: <= 262)
constexpr int SC_KW = 17;                   // the wide form: heads of at most 64 * SC_KW = 1088 classes (ops.Layout's limit)
constexpr int SC_MAX_BLOCKS = 4096;

// FULL = false: logp only (entropy and rank both NULL)
template <bool FULL>
__global__ __launch_bounds__(256) void token_scores_kernel(const float* __restrict__ logits, const int16_t* __restrict__ target,
        const float* __restrict__ mask, const Seg9 so, float* __restrict__ logp, float* __restrict__ entropy,
        int16_t* __restrict__ rank, int rows, int V) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
        if (mask[row] == 0.f) {                                     // wave-uniform; neither the logits nor the target of the row are read
            if (lane < 8) {
                logp[row * 8 + lane] = 0.f;
                if (FULL && entropy) entropy[row * 8 + lane] = 0.f;
                if (FULL && rank) rank[row * 8 + lane] = (int16_t)-1;
            }
            continue;
        }
        const float* x = logits + row * V;
        float v[8][SC_K];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = so.off[i], n = so.off[i + 1] - o;
#pragma unroll
            for (int k = 0; k < SC_K; ++k) {
                const int c = lane + 64 * k;
                v[i][k] = c < n ? x[o + c] : -INFINITY;             // tail lanes: -inf to the maximum, 0 to the sums
            }
        }
        const int my_t = lane < 8 ? (int)target[row * 8 + lane] : 0;
        float r_lp = 0.f, r_en = 0.f;
        int r_rk = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int n = so.off[i + 1] - so.off[i];
            const int tgt = __builtin_amdgcn_readlane(my_t, i);
            float mx = v[i][0];
#pragma unroll
            for (int k = 1; k < SC_K; ++k) mx = fmaxf(mx, v[i][k]);
            mx = wave_max(mx);
            float se = 0.f, sed = 0.f;                              // sum e, sum e * (x - max) with e = exp(x - max)
#pragma unroll
            for (int k = 0; k < SC_K; ++k) {
                const float dlt = v[i][k] - mx;
                const float e = lane + 64 * k < n ? __expf(dlt) : 0.f;
                se += e;                                            // the summation order of the K9 kernels
                if (FULL) sed += e > 0.f ? e * dlt : 0.f;           // p == 0 counts as 0 (never 0 * -inf)
            }
            se = wave_sum(se);
            if (FULL) sed = wave_sum(sed);
            float xt = 0.f;                                         // a target outside its head scores a logit of 0, as in pb_ce_fwd_bwd
            if (tgt >= 0 && tgt < n) {                              // wave-uniform
                const int tk = tgt >> 6, tl = tgt & 63;
                float sel = v[i][0];
#pragma unroll
                for (int k = 1; k < SC_K; ++k) sel = tk == k ? v[i][k] : sel;
                xt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sel), tl));
            }
            const float lg = __logf(se);
            const float lp = (xt - mx) - lg;
            // entropy = lse - sum p x = log(se) - sum e (x - max) / se: no cancellation against a large maximum
            const float en = FULL ? lg - sed / se : 0.f;
            int rk = 0;
            if (FULL) {
                // columns that beat the target: a greater logit, or an equal one at a lower index (tail lanes hold -inf at an index
                // >= n: they beat nothing). Wave-wide counts on the scalar unit.
#pragma unroll
                for (int k = 0; k < SC_K; ++k) {
                    const int c = lane + 64 * k;
                    rk += __popcll(__ballot(v[i][k] > xt || (v[i][k] == xt && c < tgt)));
                }
            }
            if (lane == i) { r_lp = lp; r_en = en; r_rk = rk; }
        }
        if (lane < 8) {
            logp[row * 8 + lane] = r_lp;
            if (FULL && entropy) entropy[row * 8 + lane] = r_en;
            if (FULL && rank) rank[row * 8 + lane] = (int16_t)r_rk;
        }
    }
}

// The wide form, for a dictionary with a head of 321 .. 64 * SC_KW classes: the same per-head arithmetic and summation order (lane l holds
// classes l, l + 64, ...; sums over k in order, then the wave), but one head's SC_KW values in registers at a time instead of the whole
// row's 8 x SC_K -- the register form above keeps its 40 values and is launched for every dictionary it covers.
template <bool FULL>
__global__ __launch_bounds__(256) void token_scores_wide_kernel(const float* __restrict__ logits, const int16_t* __restrict__ target,
        const float* __restrict__ mask, const Seg9 so, float* __restrict__ logp, float* __restrict__ entropy,
        int16_t* __restrict__ rank, int rows, int V) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
        if (mask[row] == 0.f) {                                     // wave-uniform; neither the logits nor the target of the row are read
            if (lane < 8) {
                logp[row * 8 + lane] = 0.f;
                if (FULL && entropy) entropy[row * 8 + lane] = 0.f;
                if (FULL && rank) rank[row * 8 + lane] = (int16_t)-1;
            }
            continue;
        }
        const float* x = logits + row * V;
        const int my_t = lane < 8 ? (int)target[row * 8 + lane] : 0;
        float r_lp = 0.f, r_en = 0.f;
        int r_rk = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int o = so.off[i], n = so.off[i + 1] - o;
            float v[SC_KW];
#pragma unroll
            for (int k = 0; k < SC_KW; ++k) {
                const int c = lane + 64 * k;
                v[k] = c < n ? x[o + c] : -INFINITY;                // tail lanes: -inf to the maximum, 0 to the sums
            }
            const int tgt = __builtin_amdgcn_readlane(my_t, i);
            float mx = v[0];
#pragma unroll
            for (int k = 1; k < SC_KW; ++k) mx = fmaxf(mx, v[k]);
            mx = wave_max(mx);
            float se = 0.f, sed = 0.f;
#pragma unroll
            for (int k = 0; k < SC_KW; ++k) {
                const float dlt = v[k] - mx;
                const float e = lane + 64 * k < n ? __expf(dlt) : 0.f;
                se += e;
                if (FULL) sed += e > 0.f ? e * dlt : 0.f;
            }
            se = wave_sum(se);
            if (FULL) sed = wave_sum(sed);
            const bool in = tgt >= 0 && tgt < n;                    // wave-uniform; a target outside its head scores a logit of 0
            const float xt = in ? x[o + tgt] : 0.f;                 // the value lane tgt & 63 holds in v[tgt >> 6]: the same bits
            const float lg = __logf(se);
            const float lp = (xt - mx) - lg;
            const float en = FULL ? lg - sed / se : 0.f;
            int rk = 0;
            if (FULL) {
#pragma unroll
                for (int k = 0; k < SC_KW; ++k) {
                    const int c = lane + 64 * k;
                    rk += __popcll(__ballot(v[k] > xt || (v[k] == xt && c < tgt)));
                }
            }
            if (lane == i) { r_lp = lp; r_en = en; r_rk = rk; }
        }
        if (lane < 8) {
            logp[row * 8 + lane] = r_lp;
            if (FULL && entropy) entropy[row * 8 + lane] = r_en;
            if (FULL && rank) rank[row * 8 + lane] = (int16_t)r_rk;
        }
    }
}

// One workgroup per sequence: thread t sums head t & 7 over positions (t >> 3) + 32 j in order, then a fixed-order sum over the 32
// position groups. No atomics: two runs give the same bits.
__global__ __launch_bounds__(256) void seq_scores_kernel(const float* __restrict__ logp, const float* __restrict__ entropy,
        const int16_t* __restrict__ rank, const float* __restrict__ mask, float* __restrict__ out, int S) {
    __shared__ float red[4][256];
    const int b = blockIdx.x, c = threadIdx.x & 7, r0 = threadIdx.x >> 3;
    float a_lp = 0.f, a_en = 0.f, a_hit = 0.f, a_m = 0.f;
    for (int s = r0; s < S; s += 32) {
        const long t = (long)b * S + s;
        const float m = mask[t];
        if (m != 0.f) {                                             // a masked position contributes nothing, whatever its row holds
            a_lp += m * logp[t * 8 + c];
            if (entropy) a_en += m * entropy[t * 8 + c];
            if (rank) a_hit += rank[t * 8 + c] == 0 ? m : 0.f;
            a_m += m;
        }
    }
    red[0][threadIdx.x] = a_lp; red[1][threadIdx.x] = a_en; red[2][threadIdx.x] = a_hit; red[3][threadIdx.x] = a_m;
    __syncthreads();
    if (threadIdx.x < 32) {
        const int plane = threadIdx.x >> 3, h = threadIdx.x & 7;
        float t = 0.f;
        for (int k = 0; k < 32; ++k) t += red[plane][k * 8 + h];
        out[(long)b * 32 + plane * 8 + h] = t;
    }
}

}  // namespace

extern "C" int pb_token_scores(const float* logits, const int16_t* target, const float* mask, const int32_t* seg_off, float* logp,
                               float* entropy, int16_t* rank, int32_t T, int32_t V, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (T <= 0) return 0;
    PB_REQUIRE(logits && target && mask && logp, "pb_token_scores: logits, target, mask and logp are required");
    PB_REQUIRE(seg_off[8] == V && seg_off[0] == 0, "pb_token_scores: segment offsets do not cover V=%d", V);
    Seg9 so;
    for (int i = 0; i < 9; ++i) so.off[i] = seg_off[i];
    bool wide = false;
    for (int i = 0; i < 8; ++i) {
        PB_REQUIRE(so.off[i + 1] > so.off[i] && so.off[i + 1] - so.off[i] <= 64 * SC_KW, "pb_token_scores: head %d has %d classes (1 .. %d)", i,
                   so.off[i + 1] - so.off[i], 64 * SC_KW);
        wide = wide || so.off[i + 1] - so.off[i] > 64 * SC_K;
    }
    const int grid = max(1, min(SC_MAX_BLOCKS, (T + 3) / 4));
    if (wide) {
        if (entropy || rank)
            hipLaunchKernelGGL((token_scores_wide_kernel<true>), dim3(grid), dim3(256), 0, stream, logits, target, mask, so, logp, entropy, rank, T, V);
        else
            hipLaunchKernelGGL((token_scores_wide_kernel<false>), dim3(grid), dim3(256), 0, stream, logits, target, mask, so, logp, entropy, rank, T, V);
    } else if (entropy || rank)
        hipLaunchKernelGGL((token_scores_kernel<true>), dim3(grid), dim3(256), 0, stream, logits, target, mask, so, logp, entropy, rank, T, V);
    else
        hipLaunchKernelGGL((token_scores_kernel<false>), dim3(grid), dim3(256), 0, stream, logits, target, mask, so, logp, entropy, rank, T, V);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_seq_scores(const float* logp, const float* entropy, const int16_t* rank, const float* mask, float* out, int32_t B,
                             int32_t S, void* stream_) {
    if (B <= 0) return 0;
    PB_REQUIRE(logp && mask && out, "pb_seq_scores: logp, mask and out are required");
    PB_REQUIRE(S >= 0, "pb_seq_scores: S=%d", S);
    hipLaunchKernelGGL(seq_scores_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream_, logp, entropy, rank, mask, out, S);
    PB_LAUNCH_CHECK();
    return 0;
}
