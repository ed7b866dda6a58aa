// Batched device-sampled decode: up to PB_DECODE_BATCH_MAX prompts through the same launches per step (pb_batch_decoder_*).
// The batch-1 fused decoder (pb_decode.hip, pb_decoder_*) streams all decoder weights for ONE row per token (~203 MB at cfg 3); here a
// step serves B rows with the same 6 n_layers + 3 launches, so the weight bytes of a step are read once for all of them.
//
// Contract: a row's arithmetic is the batch-1 kernels' arithmetic, so the logits a row logs are bit-identical to pb_decoder_*'s for the
// same prompt and fed tokens (tests/test_generate_batch_gpu.py). Each kernel below is its batch-1 counterpart with the row taken from the
// grid (embedding, attention, sampler) or from a loop over the rows (GEMV); only the loads of shared operands (weights, biases, LayerNorm
// parameters) are shared across rows:
//   * bgemv_kernel     gemv_kernel's workgroup (2 output rows, K split over 4 waves, 16-byte weight loads straight to VGPRs) keeps its
//                      weight fragments in registers and loops over the B rows: per row the same prologue (split-record merge or
//                      post-LN), the same FMA order over the thread's K chunks, the same wave / block reduction. No MFMA: its rounding
//                      differs from the FMA chain.
//   * bdec_attn_kernel dec_attn_kernel on a (H, records, B) grid: row b's position, K/V cache, encoder mask, visible extent and cross
//                      split geometry (chunk from ITS s_enc, as pb_decoder_create derives it from S_enc).
//   * bdec_embed / bdec_sample   one workgroup per row.
// Per-row state in device memory: pos[b] (last decoded position), done[b] (the sampler's special id, the position limit, or the host),
// so rows advance, stop and rewind independently. A done row writes nothing: no K/V row, no log, never past row S - 1.
#include "pb_common.h"
#include "pb_api_internal.h"

namespace {

constexpr int BMAX = PB_DECODE_BATCH_MAX;

__device__ __forceinline__ float block_sum4(float v, float* red, int lane, int wave) {
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ float half_sum(float v) {            // sum over the 32 lanes of a half-wave, in every lane of it
    v += PB_DPP_F(v, 0xb1);
    v += PB_DPP_F(v, 0x4e);
    v += PB_DPP_F(v, 0x141);
    v += PB_DPP_F(v, 0x140);
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}

// device state of a batched decoder: one allocation
struct BState {
    int pos[BMAX];                         // last decoded position of each row (-1 at reset)
    int done[BMAX];                        // 0 = live; 1 = special id sampled / stopped by the host; 2 = position limit reached
    int limit;                             // positions per row
};

// ---------------------------------------------------------------- GEMV over B rows (gemv_kernel per row, weights loaded once)
struct BMergeIn { const float* part; int nsplit, hd, stride; long row_stride; };   // records of row b at part + b row_stride

template <typename TO, int NCH, bool MERGE>
__global__ __launch_bounds__(256) void bgemv_kernel(const bf16_t* __restrict__ W, const bf16_t* __restrict__ x, const float* __restrict__ bias,
                                                    TO* __restrict__ y, int N, int K, int gelu, const bf16_t* __restrict__ res,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, bf16_t* __restrict__ ln_out,
                                                    float eps, const BMergeIn mg, const BState* __restrict__ st, int B) {
    constexpr int EPV = 8;
    typedef bf16x8 V;
    __shared__ float red[4][2];
    __shared__ float red1[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 2;
    const bool two = n0 + 1 < N;
    const bf16_t* w0 = W + (long)n0 * K;
    const bf16_t* w1 = W + (long)(two ? n0 + 1 : n0) * K;
    const V zero4 = V{};
    const float bias_v = (threadIdx.x < 2 && (threadIdx.x == 0 || two) && bias) ? bias[n0 + threadIdx.x] : 0.f;
    // shared operands, held for every row: the two weight rows' chunks of this thread, gamma / beta of a LayerNorm prologue
    V u0[NCH], u1[NCH];
    f32x4 gm[NCH][EPV / 4], bt[NCH][EPV / 4];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = (threadIdx.x + 256 * i) * EPV;
        const bool in = c < K;
        u0[i] = in ? *reinterpret_cast<const V*>(w0 + c) : zero4;
        u1[i] = in ? *reinterpret_cast<const V*>(w1 + c) : zero4;
#pragma unroll
        for (int v4 = 0; v4 < EPV / 4; ++v4) {
            gm[i][v4] = (in && res) ? *reinterpret_cast<const f32x4*>(gamma + c + 4 * v4) : f32x4{0.f, 0.f, 0.f, 0.f};
            bt[i][v4] = (in && res) ? *reinterpret_cast<const f32x4*>(beta + c + 4 * v4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    for (int b = 0; b < B; ++b) {
        if (st->done[b]) continue;                                      // block-uniform
        __syncthreads();                                                // red / red1 of the previous row are read
        const bf16_t* xb = MERGE ? nullptr : x + (long)b * K;
        const bf16_t* rb = res ? res + (long)b * K : nullptr;
        V xr[NCH], rr[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = (threadIdx.x + 256 * i) * EPV;
            const bool in = c < K;
            xr[i] = (in && !MERGE) ? *reinterpret_cast<const V*>(xb + c) : zero4;
            rr[i] = (in && rb) ? *reinterpret_cast<const V*>(rb + c) : zero4;
        }
        float xf[NCH][EPV];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = (threadIdx.x + 256 * i) * EPV;
            if (MERGE && c < K) {
                const int h = c / mg.hd, off = c % mg.hd;
                const float* rec = mg.part + (size_t)b * mg.row_stride + (size_t)h * mg.nsplit * mg.stride;
                float ms[PB_DECODE_MAX_SPLITS], ls[PB_DECODE_MAX_SPLITS];
                f32x4 oa[PB_DECODE_MAX_SPLITS][EPV / 4];
#pragma unroll
                for (int sp = 0; sp < PB_DECODE_MAX_SPLITS; ++sp) {
                    const float* r = rec + (size_t)(sp < mg.nsplit ? sp : 0) * mg.stride;
                    ms[sp] = sp < mg.nsplit ? r[0] : -INFINITY;
                    ls[sp] = r[1];
#pragma unroll
                    for (int v4 = 0; v4 < EPV / 4; ++v4) oa[sp][v4] = *reinterpret_cast<const f32x4*>(r + 4 + off + 4 * v4);
                }
                float M = -INFINITY;
#pragma unroll
                for (int sp = 0; sp < PB_DECODE_MAX_SPLITS; ++sp) M = fmaxf(M, ms[sp]);
                float L = 0.f, o[EPV];
#pragma unroll
                for (int j = 0; j < EPV; ++j) o[j] = 0.f;
#pragma unroll
                for (int sp = 0; sp < PB_DECODE_MAX_SPLITS; ++sp) {
                    const float wgt = (M == -INFINITY || ms[sp] == -INFINITY) ? 0.f : __expf(ms[sp] - M);
                    L = fmaf(ls[sp], wgt, L);
#pragma unroll
                    for (int j = 0; j < EPV; ++j) o[j] = fmaf(oa[sp][j >> 2][j & 3], wgt, o[j]);
                }
                const float inv = L > 0.f ? 1.0f / L : 0.f;
#pragma unroll
                for (int j = 0; j < EPV; ++j) xf[i][j] = to_f(from_f<bf16_t>(o[j] * inv));
            } else {
#pragma unroll
                for (int j = 0; j < EPV; ++j) xf[i][j] = to_f(xr[i][j]);
            }
        }
        if (rb) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
#pragma unroll
                for (int j = 0; j < EPV; ++j) { xf[i][j] += to_f(rr[i][j]); s += xf[i][j]; }
            }
            const float mean = block_sum4(s, red1, lane, wave) / (float)K;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const bool in = (threadIdx.x + 256 * i) * EPV < K;
#pragma unroll
                for (int j = 0; j < EPV; ++j) { const float z = xf[i][j] - mean; q = in ? fmaf(z, z, q) : q; }
            }
            const float rstd = rsqrtf(block_sum4(q, red1, lane, wave) / (float)K + eps);
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = (threadIdx.x + 256 * i) * EPV;
                V xo;
#pragma unroll
                for (int j = 0; j < EPV; ++j) {
                    xo[j] = from_f<bf16_t>((xf[i][j] - mean) * rstd * gm[i][j >> 2][j & 3] + bt[i][j >> 2][j & 3]);
                    xf[i][j] = to_f(xo[j]);
                }
                if (blockIdx.x == 0 && c < K) *reinterpret_cast<V*>(ln_out + (long)b * K + c) = xo;
            }
        }
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
#pragma unroll
            for (int j = 0; j < EPV; ++j) { a0 = fmaf(to_f(u0[i][j]), xf[i][j], a0); a1 = fmaf(to_f(u1[i][j]), xf[i][j], a1); }
        }
        a0 = wave_sum(a0); a1 = wave_sum(a1);
        if (lane == 0) { red[wave][0] = a0; red[wave][1] = a1; }
        __syncthreads();
        if (threadIdx.x < 2 && (threadIdx.x == 0 || two)) {
            const int n = n0 + threadIdx.x;
            float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x] + bias_v;
            if (gelu) v = gelu_f(v);
            y[(long)b * N + n] = from_f<TO>(v);
        }
    }
}

struct BLn { const bf16_t* res; const float* gamma; const float* beta; bf16_t* out; };

static int bgemv_launch(const void* W, const void* x, const float* bias, void* y, int N, int K, int y_f32, int gelu, const BState* st, int B,
                        hipStream_t stream, BLn ln = BLn{nullptr, nullptr, nullptr, nullptr}, BMergeIn mg = BMergeIn{nullptr, 0, 0, 0, 0}) {
    PB_REQUIRE(N > 0 && K > 0 && K % 8 == 0, "pb_batch_decoder: GEMV K=%d must be a multiple of 8", K);
    const int nch = (K + 2047) / 2048;
    PB_REQUIRE(nch <= 4 && (!mg.part || nch <= 1), "pb_batch_decoder: GEMV K=%d out of range", K);
    dim3 grid((N + 1) / 2), block(256);
#define PB_BG(TO, NCH_, MG_) hipLaunchKernelGGL((bgemv_kernel<TO, NCH_, MG_>), grid, block, 0, stream, (const bf16_t*)W, (const bf16_t*)x, bias, (TO*)y, N, K, \
                                                gelu, ln.res, ln.gamma, ln.beta, ln.out, 1e-5f, mg, st, B)
#define PB_BG_NCH(TO) do { if (mg.part) PB_BG(TO, 1, true); else if (nch <= 1) PB_BG(TO, 1, false); else if (nch == 2) PB_BG(TO, 2, false); else PB_BG(TO, 4, false); } while (0)
    if (y_f32) PB_BG_NCH(float); else PB_BG_NCH(bf16_t);
#undef PB_BG_NCH
#undef PB_BG
    PB_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------- single-query attention, (head, key split, row) workgroups
struct BAttnArgs {
    const bf16_t* x_in;                                          // (B, d) input rows when res == NULL
    const bf16_t* res; const bf16_t* add; const float* gamma; const float* beta; bf16_t* ln_out;   // x' = LN(res + add) gamma + beta, (B, d) rows
    const bf16_t* Wq; const float* bq;
    const bf16_t* Wk; const float* bk; const bf16_t* Wv; const float* bv;
    bf16_t* kc; bf16_t* vc; long kv_ss; long kv_rs;             // row b's cached key j at kc + b kv_rs + j kv_ss + h HD
    const float* key_mask; long mask_rs;                         // cross: row b's (Sk) mask at key_mask + b mask_rs, or NULL
    BState* st;
    int d, nreg;
    float scale, eps;
    float* part; long part_rs;                                   // row b's records at part + b part_rs: [H][gridDim.y][HD + 4]
    int s_enc[BMAX], ck[BMAX];                                   // cross: keys and keys per split of each row
};

template <int NC, int HD, bool SELF>
__global__ __launch_bounds__(SELF ? 768 : 256) void bdec_attn_kernel(const BAttnArgs a) {
    constexpr int CPR = HD / 8, KPW = 64 / CPR, STEP = 4 * KPW, UR = 4, RPW = HD / 4, NP = RPW / 2;
    constexpr int PBATCH = (NC <= 3 && !SELF) || NC <= 2 ? (NP < 8 ? NP : 8) : 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qs = reinterpret_cast<float*>(smem);
    float* red = qs + HD;
    float* sc = red + 4 * HD;
    const int h = blockIdx.x, sp = blockIdx.y, nrec = gridDim.y, b = blockIdx.z;
    if (a.st->done[b]) return;                                   // block-uniform: a done row writes no K/V row and no record
    const int t = threadIdx.x, lane = t & 63, l32 = lane & 31, half = lane >> 5;
    const int wgrp = SELF ? (int)(t >> 8) : 0;
    const int wave = (t >> 6) & 3;
    const int d = a.d;
    const int Sk = SELF ? a.st->pos[b] : a.s_enc[b];
    const bool is_new = SELF && sp == a.nreg;
    if (SELF && wgrp > 0 && !is_new) return;
    bf16_t* const kc = a.kc + (long)b * a.kv_rs;
    bf16_t* const vc = a.vc + (long)b * a.kv_rs;
    const float* const key_mask = a.key_mask ? a.key_mask + (long)b * a.mask_rs : nullptr;
    int ck = SELF ? 0 : a.ck[b];
    if (SELF) { ck = (Sk + a.nreg - 1) / a.nreg; ck = ck < 64 ? 64 : (ck + 15) & ~15; }
    const int j0 = sp * ck, j1 = min(Sk, j0 + ck);
    float* rec = a.part + (long)b * a.part_rs + ((size_t)h * nrec + sp) * (HD + 4);
    if (!is_new && j0 >= Sk) {
        if (t == 0) { rec[0] = -INFINITY; rec[1] = 0.f; }
        if (t < HD) rec[4 + t] = 0.f;
        return;
    }
    const int tq = t & 255;
    const int sub = lane % CPR, grp = lane / CPR;
    const int jfirst = j0 + wave * KPW;
    uint4 kpre[UR], vpre[UR];
#pragma unroll
    for (int r = 0; r < UR; ++r) {
        const int j = jfirst + r * STEP + grp;
        kpre[r] = uint4{0u, 0u, 0u, 0u}; vpre[r] = uint4{0u, 0u, 0u, 0u};
        if (!is_new && j < j1) {
            kpre[r] = *reinterpret_cast<const uint4*>(kc + (long)j * a.kv_ss + h * HD + sub * 8);
            vpre[r] = *reinterpret_cast<const uint4*>(vc + (long)j * a.kv_ss + h * HD + sub * 8);
        }
    }
    float xf[NC][8];
    if (a.res) {
        const bf16_t* resb = a.res + (long)b * d;
        const bf16_t* addb = a.add + (long)b * d;
        bf16x8 rr[NC], aa[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            rr[c] = *reinterpret_cast<const bf16x8*>(resb + (l32 + 32 * c) * 8);
            aa[c] = *reinterpret_cast<const bf16x8*>(addb + (l32 + 32 * c) * 8);
        }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) { xf[c][j] = (float)rr[c][j] + (float)aa[c][j]; s += xf[c][j]; }
        const float mean = half_sum(s) / (float)d;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float z = xf[c][j] - mean; q = fmaf(z, z, q); }
        const float rstd = rsqrtf(half_sum(q) / (float)d + a.eps);
        const bool store_ln = h == 0 && wgrp == 0 && wave == 0 && half == 0 && (SELF ? is_new : sp == 0);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int e0 = (l32 + 32 * c) * 8;
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.gamma + e0), g1 = *reinterpret_cast<const f32x4*>(a.gamma + e0 + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.beta + e0), b1 = *reinterpret_cast<const f32x4*>(a.beta + e0 + 4);
            bf16x8 xo;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                xo[j] = (bf16_t)((xf[c][j] - mean) * rstd * (j < 4 ? g0[j & 3] : g1[j & 3]) + (j < 4 ? b0[j & 3] : b1[j & 3]));
                xf[c][j] = (float)xo[j];
            }
            if (store_ln) *reinterpret_cast<bf16x8*>(a.ln_out + (long)b * d + e0) = xo;
        }
    } else {
        const bf16_t* xb = a.x_in + (long)b * d;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xb + (l32 + 32 * c) * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) xf[c][j] = (float)xv[j];
        }
    }
    auto project = [&](const bf16_t* __restrict__ W, const float* __restrict__ bias, float* out, float mul) {
#pragma unroll 1
        for (int pb = 0; pb < NP; pb += PBATCH) {
            bf16x8 w[PBATCH][NC];
            float bv[PBATCH];
#pragma unroll
            for (int p = 0; p < PBATCH; ++p) {
                const int row = h * HD + wave * RPW + 2 * (pb + p) + half;
                bv[p] = bias[row];
#pragma unroll
                for (int c = 0; c < NC; ++c) w[p][c] = *reinterpret_cast<const bf16x8*>(W + (size_t)row * d + (l32 + 32 * c) * 8);
            }
#pragma unroll
            for (int p = 0; p < PBATCH; ++p) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc = fmaf((float)w[p][c][j], xf[c][j], acc);
                acc = half_sum(acc);
                if (l32 == 0) out[wave * RPW + 2 * (pb + p) + half] = (float)(bf16_t)(acc + bv[p]) * mul;
            }
        }
    };
    if (is_new) {
        float* ks = red; float* vs = red + HD;
        if (wgrp == 0) project(a.Wq, a.bq, qs, a.scale);
        else if (wgrp == 1) project(a.Wk, a.bk, ks, 1.f);
        else project(a.Wv, a.bv, vs, 1.f);
        __syncthreads();
        if (t < HD) {
            kc[(long)Sk * a.kv_ss + h * HD + t] = (bf16_t)ks[t];         // Sk < limit <= S (the embedding kernel's guard)
            vc[(long)Sk * a.kv_ss + h * HD + t] = (bf16_t)vs[t];
            rec[4 + t] = vs[t];
        }
        if (t < 64) {
            float p = 0.f;
#pragma unroll
            for (int e = lane; e < HD; e += 64) p = fmaf(qs[e], ks[e], p);
            p = wave_sum(p);
            if (lane == 0) { rec[0] = p; rec[1] = 1.f; }
        }
        return;
    }
    project(a.Wq, a.bq, qs, a.scale);
    __syncthreads();
    float qv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] = qs[sub * 8 + e];
    float mx = -INFINITY;
    for (int jb = jfirst; jb < j1; jb += UR * STEP) {
        uint4 kraw[UR];
#pragma unroll
        for (int r = 0; r < UR; ++r) {
            const int j = jb + r * STEP + grp;
            kraw[r] = kpre[r];
            if (jb != jfirst) {
                kraw[r] = uint4{0u, 0u, 0u, 0u};
                if (j < j1) kraw[r] = *reinterpret_cast<const uint4*>(kc + (long)j * a.kv_ss + h * HD + sub * 8);
            }
        }
#pragma unroll
        for (int r = 0; r < UR; ++r) {
            const int j = jb + r * STEP + grp;
            float s = 0.f;
            if (j < j1) {
                const bf16_t* kv = reinterpret_cast<const bf16_t*>(&kraw[r]);
#pragma unroll
                for (int e = 0; e < 8; ++e) s = fmaf((float)kv[e], qv[e], s);
            }
#pragma unroll
            for (int o = 1; o < CPR; o <<= 1) s += __shfl_xor(s, o, 64);
            if (j < j1) {
                const float sv = (!key_mask || key_mask[j] != 0.f) ? s : -INFINITY;
                if (sub == 0) sc[j - j0] = sv;
                mx = fmaxf(mx, sv);
            }
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    if (mx != -INFINITY)
        for (int j = tq; j < j1 - j0; j += 256) { const float e = __expf(sc[j] - mx); sc[j] = e; sum += e; }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    sum = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (mx != -INFINITY)
        for (int jb = jfirst; jb < j1; jb += UR * STEP) {
            uint4 vraw[UR];
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                const int j = jb + r * STEP + grp;
                vraw[r] = vpre[r];
                if (jb != jfirst) {
                    vraw[r] = uint4{0u, 0u, 0u, 0u};
                    if (j < j1) vraw[r] = *reinterpret_cast<const uint4*>(vc + (long)j * a.kv_ss + h * HD + sub * 8);
                }
            }
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                const int j = jb + r * STEP + grp;
                if (j < j1) {
                    const bf16_t* vv = reinterpret_cast<const bf16_t*>(&vraw[r]);
                    const float pj = sc[j - j0];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, (float)vv[e], acc[e]);
                }
            }
        }
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int o = CPR; o < 64; o <<= 1) acc[e] += __shfl_xor(acc[e], o, 64);
    if (grp == 0)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[wave * HD + sub * 8 + e] = acc[e];
    __syncthreads();
    if (t == 0) { rec[0] = mx; rec[1] = sum; }
    if (t < HD) rec[4 + t] = (red[t] + red[HD + t]) + (red[2 * HD + t] + red[3 * HD + t]);
}

// ---------------------------------------------------------------- token embedding + position + LayerNorm, one workgroup per row
struct SegOff9 { int off[9]; };
__global__ __launch_bounds__(256) void bdec_embed_kernel(const int16_t* __restrict__ tok16, const float* __restrict__ P, const SegOff9 so,
                                                         const float* __restrict__ lin_b, const float* __restrict__ pos_tab,
                                                         const float* __restrict__ w, const float* __restrict__ bb, bf16_t* __restrict__ y,
                                                         BState* __restrict__ st, int d, float eps) {
    __shared__ float red1[4];
    const int b = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, d4 = d >> 2;
    if (st->done[b]) return;                                     // block-uniform
    const int i = st->pos[b] + 1;
    if (i >= st->limit) {                                        // the row's last position is decoded: it stops here (no row past limit - 1 <= S - 1)
        __syncthreads();                                         // every thread has read done[b] before it changes
        if (t == 0) st->done[b] = 2;
        return;
    }
    tok16 += b * 8;
    y += (long)b * d;
    const uint4 raw = *reinterpret_cast<const uint4*>(tok16);
    int id[8];
    id[0] = (int)(raw.x & 0xffff); id[1] = (int)(raw.x >> 16); id[2] = (int)(raw.y & 0xffff); id[3] = (int)(raw.y >> 16);
    id[4] = (int)(raw.z & 0xffff); id[5] = (int)(raw.z >> 16); id[6] = (int)(raw.w & 0xffff); id[7] = (int)(raw.w >> 16);
    const bool in = t < d4;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (in) {
        v = load4(lin_b + 4 * t) + load4(pos_tab + (size_t)(i + 2) * d + 4 * t);
#pragma unroll
        for (int k = 0; k < 8; ++k) v += load4(P + (size_t)(so.off[k] + id[k]) * d + 4 * t);
    }
    const float mean = block_sum4(in ? v[0] + v[1] + v[2] + v[3] : 0.f, red1, lane, wave) / (float)d;
    float q = 0.f;
    if (in) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float c = v[j] - mean; q += c * c; }
    }
    const float rstd = rsqrtf(block_sum4(q, red1, lane, wave) / (float)d + eps);
    if (in) store4(y + 4 * t, (v - mean) * rstd * load4(w + 4 * t) + load4(bb + 4 * t));
    if (t == 0) st->pos[b] = i;
}

// ---------------------------------------------------------------- device-side nucleus sampling, one workgroup per row
// dec_sample_kernel (pb_decode.hip) with row b's logits, draws, logs and next input; a special id (>= pad[h] for any head) marks the row done.
struct BSampleArgs {
    const float* logits;                  // (B, vocab) f32
    const double* u;                      // (B, S, 8) draws, device
    BState* st;
    int16_t* tok_dev;                     // (B, 8) next decoder inputs
    float* log_logits;                    // pinned host (B, S, vocab)
    int16_t* log_tok;                     // pinned host (B, S, 8)
    int vocab, S, fault_row, fault_period;
    int off[8], n[8], pad[8];
    float temp[8], p[8];
};
constexpr int SMP_W = 272;
__device__ __forceinline__ float wave_scan_f(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
    return v;
}
__global__ __launch_bounds__(512) void bdec_sample_kernel(const BSampleArgs a) {
    __shared__ __attribute__((aligned(16))) float pn[8][SMP_W];
    __shared__ float sp[8][SMP_W + 64];
    __shared__ int si[8][SMP_W];
    __shared__ int htok[8];
    const int b = blockIdx.x;
    if (a.st->done[b]) return;                                   // block-uniform
    const int t = threadIdx.x, lane = t & 63, h = t >> 6;
    const int pos = a.st->pos[b];
    const float* logits = a.logits + (size_t)b * a.vocab;
    float* log_logits = a.log_logits + ((size_t)b * a.S + pos) * a.vocab;
    const int n = a.n[h], off = a.off[h];
    const float T = a.temp[h];
    const double u_draw = a.u[((size_t)b * a.S + pos) * 8 + h];
    float y[5], e[5];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int c = lane + 64 * k;
        const bool in = c < n;
        const float lg = in ? logits[off + c] : 0.f;
        if (in) log_logits[off + c] = lg;
        y[k] = in ? lg / T : -INFINITY;
        mx = fmaxf(mx, y[k]);
    }
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 5; ++k) { e[k] = (lane + 64 * k < n) ? expf(y[k] - mx) : 0.f; s += e[k]; }
    s = wave_sum(s);
    const float inv = 1.0f / (s * 1.00001f);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int c = lane + 64 * k;
        if (c < SMP_W) pn[h][c] = c < n ? e[k] * inv : -1.f;
    }
    __syncthreads();
    {
        int hh = -1, c = t;
        for (int q = 0; q < 8; ++q) {
            if (a.p[q] < 1.0f) {
                if (hh < 0 && c < a.n[q]) hh = q;
                if (hh < 0) c -= a.n[q];
            }
        }
        if (hh >= 0) {
            const float v = pn[hh][c];
            int rank = 0;
#pragma unroll 17
            for (int j4 = 0; j4 < SMP_W / 4; ++j4) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(&pn[hh][4 * j4]);
#pragma unroll
                for (int r = 0; r < 4; ++r) rank += (w[r] > v || (w[r] == v && 4 * j4 + r < c)) ? 1 : 0;
            }
            sp[hh][rank] = v; si[hh][rank] = c;
        }
        if (t < 8 * 64) sp[t >> 6][SMP_W + (t & 63)] = 0.f;
    }
    __syncthreads();
    const float ph = a.p[h];
    if (ph < 1.0f) {
        float v5[5], pre[5];
        float run = 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k) { const int i = 5 * lane + k; v5[k] = i < n ? sp[h][i] : 0.f; run += v5[k]; pre[k] = run; }
        const float base = wave_scan_f(run, lane) - run;
        int first = 0x7fffffff;
#pragma unroll
        for (int k = 4; k >= 0; --k) if (5 * lane + k < n && base + pre[k] > ph) first = 5 * lane + k;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        const int kc = first == 0x7fffffff ? 1 : first + 1;
        float myqs = 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k) if (5 * lane + k == kc - 1) myqs = base + pre[k];
        const float qs = wave_sum(myqs);
        const float thr = (float)(u_draw * (double)qs);
        int best = kc - 1;
#pragma unroll
        for (int k = 4; k >= 0; --k) if (5 * lane + k < kc && base + pre[k] > thr) best = 5 * lane + k;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        if (lane == 0) htok[h] = si[h][best];
    } else {
        float bv = -1.f; int bi = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int c = lane + 64 * k;
            if (c < n) { const float v = pn[h][c]; if (v > bv) { bv = v; bi = c; } }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) htok[h] = bi;
    }
    __syncthreads();
    if (t < 8) {
        int id = htok[t];
        if (a.fault_period > 0 && b == a.fault_row && t == 0 && (pos % a.fault_period) == a.fault_period - 1) id = (id + 1) % a.n[0];
        a.tok_dev[b * 8 + t] = (int16_t)id;
        a.log_tok[((size_t)b * a.S + pos) * 8 + t] = (int16_t)id;
        if (id >= a.pad[t]) a.st->done[b] = 1;                   // the device stops the row here; the host confirms or rewinds it
    }
}

constexpr int SPEC_K = 8;                  // batched steps per graph replay
constexpr int SPEC_EVENTS = 8;

struct BDecoder {
    pb_decode_batch bp;
    int B = 0;
    hipStream_t stream = nullptr;
    BState* st = nullptr;                  // device
    int16_t* tok_dev = nullptr;            // device (B, 8)
    int16_t* tok_host = nullptr;           // pinned (B, 8)
    double* u_dev = nullptr;
    float* log_logits = nullptr;           // pinned (B, S, vocab)
    int16_t* log_tok = nullptr;            // pinned (B, S, 8)
    BSampleArgs sa{};
    bool sampler = false;
    hipGraph_t graph1 = nullptr, graphK = nullptr;
    hipGraphExec_t exec1 = nullptr, execK = nullptr;
    hipEvent_t ev = nullptr;
    hipEvent_t evs[SPEC_EVENTS] = {};
    int next_ev = 0;
    int launches = 0, use_graph = 1, ns_self = PB_DECODE_MAX_SPLITS, ns_cross = PB_DECODE_MAX_SPLITS;
    int ck_cross[BMAX] = {};
    size_t lds_attn = 0;
};

template <int NC, int HD>
static void bdec_attn_go(const BAttnArgs& a, bool self, int H, int nrec, int B, size_t lds, hipStream_t st) {
    if (self) hipLaunchKernelGGL((bdec_attn_kernel<NC, HD, true>), dim3(H, nrec, B), dim3(768), lds, st, a);
    else hipLaunchKernelGGL((bdec_attn_kernel<NC, HD, false>), dim3(H, nrec, B), dim3(256), lds, st, a);
}
static int bdec_attn_launch(const BAttnArgs& a, bool self, int H, int hd, int nrec, int B, size_t lds, hipStream_t st) {
    const int nc = a.d / 256;
#define PB_DA(NC_) do { if (hd == 64) bdec_attn_go<NC_, 64>(a, self, H, nrec, B, lds, st); else bdec_attn_go<NC_, 128>(a, self, H, nrec, B, lds, st); } while (0)
    if (nc == 1) PB_DA(1); else if (nc == 2) PB_DA(2); else if (nc == 3) PB_DA(3); else PB_DA(4);
#undef PB_DA
    PB_LAUNCH_CHECK();
    return 0;
}

// the launches of one batched step (decoder_issue of pb_decode.hip over B rows) followed by the sampler; returns their number in *count
static int bdecoder_issue(BDecoder* D, hipStream_t st, int* count) {
    const pb_decode_plan* p = &D->bp.plan;
    const int d = p->d, H = p->H, hd = d / H, f = p->ffn, B = D->B, S = p->S;
    const float scale = 1.0f / sqrtf((float)hd);
    const long kv_rs = (long)S * 2 * d, part_rs = (long)H * PB_DECODE_MAX_SPLITS * (hd + 4);
    int n = 0;
    SegOff9 so;
    for (int k = 0; k < 9; ++k) so.off[k] = p->tab_off[k];
    hipLaunchKernelGGL(bdec_embed_kernel, dim3(B), dim3(256), 0, st, D->tok_dev, p->ptab, so, p->lin_b, p->pos, p->lne_w, p->lne_b, (bf16_t*)p->x, D->st, d, 1e-5f);
    PB_LAUNCH_CHECK(); ++n;
    bf16_t* x = (bf16_t*)p->x; bf16_t* alt = (bf16_t*)p->y2;
    bf16_t* h = x;
    BLn ln{nullptr, nullptr, nullptr, nullptr};
    const BMergeIn mg_self{p->attn_part, D->ns_self, hd, hd + 4, part_rs}, mg_cross{p->attn_part, D->ns_cross, hd, hd + 4, part_rs};
    for (int l = 0; l < p->n_layers; ++l) {
        const pb_decode_layer& L = p->layers[l];
        BAttnArgs a{};
        a.d = d; a.scale = scale; a.eps = 1e-5f; a.part = p->attn_part; a.part_rs = part_rs; a.st = D->st; a.kv_ss = 2 * d; a.kv_rs = kv_rs;
        a.x_in = h; a.res = ln.res; a.add = (const bf16_t*)p->a; a.gamma = ln.gamma; a.beta = ln.beta; a.ln_out = ln.out;
        a.Wq = (const bf16_t*)L.wqkv; a.bq = L.bqkv;
        a.Wk = a.Wq + (size_t)d * d; a.bk = L.bqkv + d; a.Wv = a.Wq + (size_t)2 * d * d; a.bv = L.bqkv + 2 * d;
        a.kc = (bf16_t*)L.kv_self; a.vc = a.kc + d; a.key_mask = nullptr; a.mask_rs = 0; a.nreg = D->ns_self - 1;
        if (bdec_attn_launch(a, true, H, hd, D->ns_self, B, D->lds_attn, st)) return -1;
        ++n;
        if (ln.res) h = alt;
        if (bgemv_launch(L.wo, nullptr, L.bo, p->a, d, d, 0, 0, D->st, B, st, BLn{nullptr, nullptr, nullptr, nullptr}, mg_self)) return -1;
        ++n;
        BAttnArgs c{};
        c.d = d; c.scale = scale; c.eps = 1e-5f; c.part = p->attn_part; c.part_rs = part_rs; c.st = D->st; c.kv_ss = 2 * d; c.kv_rs = kv_rs;
        c.x_in = nullptr; c.res = h; c.add = (const bf16_t*)p->a; c.gamma = L.ln1_w; c.beta = L.ln1_b; c.ln_out = (bf16_t*)p->y1;
        c.Wq = (const bf16_t*)L.wq_c; c.bq = L.bq_c;
        c.kc = (bf16_t*)const_cast<void*>(L.kv_cross); c.vc = c.kc + d; c.key_mask = p->enc_mask; c.mask_rs = S; c.nreg = D->ns_cross;
        for (int b = 0; b < B; ++b) { c.s_enc[b] = D->bp.s_enc[b]; c.ck[b] = D->ck_cross[b]; }
        if (bdec_attn_launch(c, false, H, hd, D->ns_cross, B, D->lds_attn, st)) return -1;
        ++n;
        if (bgemv_launch(L.wo_c, nullptr, L.bo_c, p->a, d, d, 0, 0, D->st, B, st, BLn{nullptr, nullptr, nullptr, nullptr}, mg_cross)) return -1;
        ++n;
        if (bgemv_launch(L.w1, p->a, L.b1, p->g, f, d, 0, 1, D->st, B, st, BLn{(const bf16_t*)p->y1, L.lnc_w, L.lnc_b, (bf16_t*)p->yc})) return -1;
        ++n;
        if (bgemv_launch(L.w2, p->g, L.b2, p->a, d, f, 0, 0, D->st, B, st)) return -1;
        ++n;
        ln = BLn{(const bf16_t*)p->yc, L.ln2_w, L.ln2_b, alt};
    }
    if (bgemv_launch(p->head_w, p->a, p->head_b, p->logits, p->vocab, d, 1, 0, D->st, B, st, ln)) return -1;
    ++n;
    hipLaunchKernelGGL(bdec_sample_kernel, dim3(B), dim3(512), 0, st, D->sa);
    PB_LAUNCH_CHECK(); ++n;
    *count = n;
    return 0;
}

static int bspec_issue(BDecoder* D, hipStream_t st, int ntok, int* count) {
    for (int k = 0; k < ntok; ++k)
        if (bdecoder_issue(D, st, count)) return -1;
    return 0;
}

// K steps as one graph: a single linear stream of kernels (no parallel branches)
static bool bspec_capture(BDecoder* D, int ntok, hipGraph_t* g, hipGraphExec_t* x) {
    int n = 0;
    if (hipStreamBeginCapture(D->stream, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); return false; }
    const int rc = bspec_issue(D, D->stream, ntok, &n);
    const hipError_t e = hipStreamEndCapture(D->stream, g);
    if (rc || e != hipSuccess || !*g || hipGraphInstantiate(x, *g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (*g) { (void)hipGraphDestroy(*g); *g = nullptr; }
        *x = nullptr;
        return false;
    }
    D->launches = n;
    return true;
}

}  // namespace

extern "C" int pb_batch_decoder_create(const pb_decode_batch* bp, void** out) {
    PB_REQUIRE(bp && out, "pb_batch_decoder_create: null argument");
    *out = nullptr;
    const pb_decode_plan* plan = &bp->plan;
    const int d = plan->d, H = plan->H, hd = H > 0 ? d / H : 0;
    // the shapes of pb_decoder_create (return 1 = declined, not an error), 1 <= B <= 16, every row with a visible encoder extent
    if (plan->dtype != PB_BF16 || H <= 0 || d % H != 0 || (hd != 64 && hd != 128) || d % 256 != 0 || d > 1024 || !plan->attn_part ||
        plan->n_layers <= 0 || plan->n_layers > PB_DECODE_MAX_LAYERS || plan->ffn % 8 != 0 || plan->ffn > 8192 || plan->S <= 0 ||
        bp->B < 1 || bp->B > BMAX) return 1;
    for (int b = 0; b < bp->B; ++b)
        if (bp->s_enc[b] <= 0 || bp->s_enc[b] > plan->S) return 1;
    BDecoder* D = new BDecoder();
    D->bp = *bp;
    D->B = bp->B;
    if (hipStreamCreateWithFlags(&D->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&D->ev, hipEventDisableTiming) != hipSuccess ||
        hipMalloc(&D->st, sizeof(BState)) != hipSuccess || hipMalloc(&D->tok_dev, 16 * BMAX) != hipSuccess ||
        hipHostMalloc(&D->tok_host, 16 * BMAX, hipHostMallocDefault) != hipSuccess) {
        pb_set_error("pb_batch_decoder_create: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        pb_batch_decoder_destroy(D);
        return -1;
    }
    // split geometry exactly as pb_decoder_create, the cross-attention chunk from each row's own visible extent
    auto env_splits = [](const char* name, int dflt) { const char* e = getenv(name); int v = e ? atoi(e) : dflt; return v < 2 ? 2 : (v > PB_DECODE_MAX_SPLITS ? PB_DECODE_MAX_SPLITS : v); };
    D->ns_self = env_splits("PB_DECODE_SPLITS_SELF", PB_DECODE_MAX_SPLITS);
    D->ns_cross = env_splits("PB_DECODE_SPLITS_CROSS", PB_DECODE_MAX_SPLITS);
    int ck_max = 0;
    for (int b = 0; b < D->B; ++b) {
        int ck = (bp->s_enc[b] + D->ns_cross - 1) / D->ns_cross;
        ck = ck < 64 ? 64 : (ck + 15) & ~15;
        D->ck_cross[b] = ck;
        ck_max = ck > ck_max ? ck : ck_max;
    }
    int ck_self = (plan->S + D->ns_self - 2) / (D->ns_self - 1);
    ck_self = ck_self < 64 ? 64 : (ck_self + 15) & ~15;
    D->lds_attn = sizeof(float) * (size_t)(5 * hd + (ck_max > ck_self ? ck_max : ck_self) + 16);
    *out = D;
    return 0;
}

extern "C" int pb_batch_decoder_destroy(void* dec) {
    BDecoder* D = (BDecoder*)dec;
    if (!D) return 0;
    if (D->stream) (void)hipStreamSynchronize(D->stream);
    if (D->exec1) (void)hipGraphExecDestroy(D->exec1);
    if (D->graph1) (void)hipGraphDestroy(D->graph1);
    if (D->execK) (void)hipGraphExecDestroy(D->execK);
    if (D->graphK) (void)hipGraphDestroy(D->graphK);
    for (int i = 0; i < SPEC_EVENTS; ++i) if (D->evs[i]) (void)hipEventDestroy(D->evs[i]);
    if (D->u_dev) (void)hipFree(D->u_dev);
    if (D->log_logits) (void)hipHostFree(D->log_logits);
    if (D->log_tok) (void)hipHostFree(D->log_tok);
    if (D->ev) (void)hipEventDestroy(D->ev);
    if (D->st) (void)hipFree(D->st);
    if (D->tok_dev) (void)hipFree(D->tok_dev);
    if (D->tok_host) (void)hipHostFree(D->tok_host);
    if (D->stream) (void)hipStreamDestroy(D->stream);
    delete D;
    return 0;
}

// Start of a batch: every row at position -1 and live (pos = -1: 0xff bytes, done = 0), behind the caller's stream.
extern "C" int pb_batch_decoder_reset(void* dec, void* caller_stream, int32_t use_graph) {
    BDecoder* D = (BDecoder*)dec;
    PB_REQUIRE(D, "pb_batch_decoder_reset: null decoder");
    PB_CHECK_HIP(hipEventRecord(D->ev, (hipStream_t)caller_stream));
    PB_CHECK_HIP(hipStreamWaitEvent(D->stream, D->ev, 0));
    PB_CHECK_HIP(hipMemsetAsync(D->st->pos, 0xff, sizeof(int) * BMAX, D->stream));
    PB_CHECK_HIP(hipMemsetAsync(D->st->done, 0, sizeof(int) * BMAX, D->stream));
    D->use_graph = use_graph;
    return 0;
}

extern "C" int pb_batch_decoder_sampler_init(void* dec, const float* temps8, const float* p8, const int32_t* n8, const int32_t* off8, const int32_t* pad8,
                                             const double* u, int64_t n_u, int32_t limit, int32_t fault_row, int32_t fault_period) {
    BDecoder* D = (BDecoder*)dec;
    PB_REQUIRE(D && temps8 && p8 && n8 && off8 && pad8 && u, "pb_batch_decoder_sampler_init: null argument");
    const size_t S = (size_t)D->bp.plan.S, B = (size_t)D->B, vocab = (size_t)D->bp.plan.vocab;
    PB_REQUIRE(n_u >= (int64_t)(B * S * 8), "pb_batch_decoder_sampler_init: %lld draws for %d rows x %d positions x 8 heads", (long long)n_u, D->B, (int)S);
    PB_REQUIRE(limit >= 0 && limit <= (int)S, "pb_batch_decoder_sampler_init: limit %d outside 0..%d", limit, (int)S);
    for (int h = 0; h < 8; ++h) {
        PB_REQUIRE(n8[h] > 0 && n8[h] <= SMP_W && n8[h] <= 320 && off8[h] >= 0 && off8[h] + n8[h] <= (int)vocab && temps8[h] > 0.f,
                   "pb_batch_decoder_sampler_init: head %d (n %d, offset %d, temperature %g)", h, n8[h], off8[h], (double)temps8[h]);
        D->sa.n[h] = n8[h]; D->sa.off[h] = off8[h]; D->sa.temp[h] = temps8[h]; D->sa.p[h] = p8[h]; D->sa.pad[h] = pad8[h];
    }
    int sorted = 0;
    for (int h = 0; h < 8; ++h) if (p8[h] < 1.0f) sorted += n8[h];
    PB_REQUIRE(sorted <= 512, "pb_batch_decoder_sampler_init: %d classes under heads with p < 1 (one thread each, 512 threads)", sorted);
    if (!D->u_dev) {
        if (hipMalloc(&D->u_dev, sizeof(double) * B * S * 8) != hipSuccess ||
            hipHostMalloc(&D->log_logits, sizeof(float) * B * S * vocab, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&D->log_tok, sizeof(int16_t) * B * S * 8, hipHostMallocDefault) != hipSuccess) {
            pb_set_error("pb_batch_decoder_sampler_init: allocation failed: %s", hipGetErrorString(hipGetLastError()));
            return -1;
        }
        for (int i = 0; i < SPEC_EVENTS; ++i) PB_CHECK_HIP(hipEventCreateWithFlags(&D->evs[i], hipEventDisableTiming));
    }
    PB_CHECK_HIP(hipMemcpyAsync(D->u_dev, u, sizeof(double) * B * S * 8, hipMemcpyHostToDevice, D->stream));
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->limit, limit, 1, D->stream));
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));
    D->sa.logits = D->bp.plan.logits; D->sa.u = D->u_dev; D->sa.st = D->st; D->sa.tok_dev = D->tok_dev;
    D->sa.log_logits = D->log_logits; D->sa.log_tok = D->log_tok; D->sa.vocab = (int)vocab; D->sa.S = (int)S;
    D->sa.fault_row = fault_row; D->sa.fault_period = fault_period;
    if (D->exec1 || D->execK) {                                         // captured with the previous constants
        if (D->exec1) { (void)hipGraphExecDestroy(D->exec1); D->exec1 = nullptr; }
        if (D->graph1) { (void)hipGraphDestroy(D->graph1); D->graph1 = nullptr; }
        if (D->execK) { (void)hipGraphExecDestroy(D->execK); D->execK = nullptr; }
        if (D->graphK) { (void)hipGraphDestroy(D->graphK); D->graphK = nullptr; }
    }
    D->sampler = true;
    return 0;
}

// Enqueue `ntok` batched steps; first_tok ((B, 8) host ids, may be NULL) is copied up in front as the rows' decoder inputs.
extern "C" int pb_batch_decoder_launch(void* dec, int32_t ntok, const int16_t* first_tok) {
    BDecoder* D = (BDecoder*)dec;
    PB_REQUIRE(D && D->sampler, "pb_batch_decoder_launch: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(ntok > 0, "pb_batch_decoder_launch: %d steps", ntok);
    if (first_tok) {
        PB_CHECK_HIP(hipStreamSynchronize(D->stream));                 // tok_host is about to be rewritten: no copy of it may be in flight
        for (int k = 0; k < 8 * D->B; ++k) D->tok_host[k] = first_tok[k];
        PB_CHECK_HIP(hipMemcpyAsync(D->tok_dev, D->tok_host, 16 * (size_t)D->B, hipMemcpyHostToDevice, D->stream));
    }
    if (D->use_graph && !D->exec1) {
        PB_CHECK_HIP(hipStreamSynchronize(D->stream));
        if (!bspec_capture(D, 1, &D->graph1, &D->exec1) || !bspec_capture(D, SPEC_K, &D->graphK, &D->execK)) D->use_graph = 0;
    }
    int left = ntok;
    while (left > 0) {
        if (D->use_graph && left >= SPEC_K) { PB_CHECK_HIP(hipGraphLaunch(D->execK, D->stream)); left -= SPEC_K; }
        else if (D->use_graph) { PB_CHECK_HIP(hipGraphLaunch(D->exec1, D->stream)); left -= 1; }
        else { int n = 0; if (bspec_issue(D, D->stream, 1, &n)) return -1; D->launches = n; left -= 1; }
    }
    const int tk = D->next_ev;
    D->next_ev = (D->next_ev + 1) % SPEC_EVENTS;
    PB_CHECK_HIP(hipEventRecord(D->evs[tk], D->stream));
    return tk;
}
extern "C" int pb_batch_decoder_wait(void* dec, int32_t ticket) {
    BDecoder* D = (BDecoder*)dec;
    PB_REQUIRE(D && D->sampler && ticket >= 0 && ticket < SPEC_EVENTS, "pb_batch_decoder_wait: bad ticket %d", ticket);
    PB_CHECK_HIP(hipEventSynchronize(D->evs[ticket]));
    return 0;
}
extern "C" int pb_batch_decoder_logs(void* dec, float** logits_rows, int16_t** tok_rows) {
    BDecoder* D = (BDecoder*)dec;
    PB_REQUIRE(D && D->sampler && logits_rows && tok_rows, "pb_batch_decoder_logs: no sampler");
    *logits_rows = D->log_logits; *tok_rows = D->log_tok;
    return 0;
}
// Rewind one row (tok8 != NULL): drain what is enqueued, then row's last decoded position = pos, its next input = tok8, live again. The
// other rows keep their positions, inputs and flags. tok8 == NULL: the row is done from the next enqueued step on (no drain).
extern "C" int pb_batch_decoder_seek(void* dec, int32_t row, int32_t pos, const int16_t* tok8) {
    BDecoder* D = (BDecoder*)dec;
    PB_REQUIRE(D && row >= 0 && row < D->B, "pb_batch_decoder_seek: row %d", row);
    if (!tok8) {
        PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->done[row], 1, 1, D->stream));
        return 0;
    }
    PB_REQUIRE(pos >= -1 && pos < D->bp.plan.S, "pb_batch_decoder_seek: position %d", pos);
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));
    for (int k = 0; k < 8; ++k) D->tok_host[row * 8 + k] = tok8[k];
    PB_CHECK_HIP(hipMemcpyAsync(D->tok_dev + row * 8, D->tok_host + row * 8, 16, hipMemcpyHostToDevice, D->stream));
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->pos[row], pos, 1, D->stream));
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->done[row], 0, 1, D->stream));
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));
    return 0;
}

extern "C" int pb_batch_decoder_launches(void* dec) { return dec ? ((BDecoder*)dec)->launches : 0; }
extern "C" int pb_batch_decoder_graph(void* dec) { return dec ? (((BDecoder*)dec)->use_graph && ((BDecoder*)dec)->execK ? 1 : 0) : 0; }
