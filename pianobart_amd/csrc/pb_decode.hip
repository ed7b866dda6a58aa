// K13: batch-1 KV-cached decode (PianoBartLM.forward(generate=True), /root/reference/model.py:28-66).
// The reference re-runs the full encoder + decoder over all S positions for every generated position; here one decoder
// token goes through the layers against cached keys/values. At batch 1 every op is a weight-streaming GEMV (HBM-bound:
// ~203 MB of bf16 decoder weights per token at cfg 2) or a tiny row op, so the kernels are:
//   * gemv_kernel    y = act(W x + b): 2 output rows per workgroup, K split over its 4 waves, 16-byte weight loads straight
//                    to VGPRs (no LDS: the operand is streamed once and not shared, cdna_hip_programming.md "GEMV" row);
//   * attn_decode    single-query attention, one 16-wave workgroup per head, coalesced row-chunk loads of the cached K/V
//                    (the stand-alone pb_attn_decode op); inside pb_decode_step the keys of a head are split over up to 16
//                    workgroups (attn_split_kernel) whose partial {max, sum, output} records the out-projection GEMV merges
//                    in its prologue -- no merge launch, no inter-workgroup hand-off;
//   * pb_decode_step a native host function that issues the 8*ND + 2 launches of one token (embed -> ND x [q|k|v (+LN2 of the
//                    layer below), self-attn, out, q_c (+LN1), cross-attn, out_c, fc1+GELU (+LNc), fc2] -> heads (+LN2))
//                    without Python between; the post-LNs ride in the prologue of the GEMV that consumes them.
#include <vector>

#include "pb_common.h"
#include "pb_api_internal.h"

namespace {

// ---------------------------------------------------------------- GEMV: y[n] = act(sum_k W[n][k] x'[k] + b[n])
// One workgroup = 4 waves = 2 output rows; the 4 waves split K (16-byte loads, each weight byte read once), partial sums meet in
// LDS. N/2 workgroups keep every CU streaming even at N = 768. Rows n >= n_split go to y2 (the K|V cache row) instead of y.
// With `res` set the input is the post-LN residual row x' = LayerNorm(res + x) * gamma + beta, recomputed by every workgroup
// (d reads from L2, two block reductions) so that the BART post-LN needs no launch of its own; workgroup 0 also stores x'
// to ln_out, where the next residual add finds it.
__device__ __forceinline__ float block_sum4(float v, float* red, int lane, int wave) {
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// With `part` set the input vector is the attention context that attn_split_kernel left as per-key-split partials
// part[h][s] = {m, l, -, -, o[hd]} (f32): every workgroup merges the splits of the heads its K range touches on the fly
// (ctx = sum_s o_s e^(m_s - M) / sum_s l_s e^(m_s - M), rounded to T like the stored context of the one-kernel form), so the
// split needs neither a merge launch nor any inter-workgroup hand-off inside the attention kernel.
struct MergeIn { const float* part; int nsplit, hd, stride; long row_stride; };    // stride = floats per (head, split) record;
                                                                                    // row form: row b's records at part + b row_stride

// NCH = chunks of EPV elements a thread owns along K (K <= NCH * 256 * EPV). Everything a thread will ever read -- its weight chunks
// of both rows, x, the residual, gamma / beta, the split records' maxima -- is requested up front, so the kernel is ONE memory round
// trip deep (plus the two block reductions of the LayerNorm statistics): at batch 1 these kernels are latency, not bandwidth.
template <typename T> struct VecOf;
template <> struct VecOf<bf16_t> { typedef bf16x8 type; };
template <> struct VecOf<float> { typedef f32x4 type; };

// Device state of the fused decoder (pb_batch_decoder_*, below): one allocation.
constexpr int BMAX = PB_DECODE_BATCH_MAX;
struct BState {
    int pos[BMAX];                         // last decoded position of each row (-1 at reset)
    int done[BMAX];                        // row form: 0 = live; 1 = special id sampled / stopped by the host; 2 = position limit reached
    int limit[BMAX];                       // row form: the row stops before this position (a primed row: its prefix + max_new)
    // cross-attention geometry of each row, read by the dynamic decoder's cross-attention launch only (pb_batch_decoder_dynamic; the other
    // forms carry it in their kernarg block): set at create, reset, start and by pb_batch_decoder_admit
    int s_enc[BMAX];                       // visible encoder keys
    int ck[BMAX];                          // keys per split
    int kv_row[BMAX];                      // the slice of the cross K|V cache the row attends to
    // row form, the device sampler only: the row is done when head 0 (the bar) of its token is >= stop[b]. pad[0] = no stop beyond the special
    // ids; a lower value is the bar the row stops at (pb_batch_decoder_stop, pb_batch_decoder_admit_stop). Set by sampler_init, start and admit
    int stop[BMAX];
    // the device sampler, both forms: order[b] >= 0 = the row is time-ordered with that bar floor, -1 = sampled freely
    // (pb_batch_decoder_order, pb_batch_decoder_admit_order). opad = the first special ids of heads 0 (bar) and 1 (position): the single-row
    // sampler's kernargs hold no pad. Set by sampler_init, start and admit
    // ... and rule[b].allow >= 0 = the row samples only the classes whose bit is set in mask allow of the table amask ((n_masks, awords)
    // uint32 words in device memory the decoder owns, bit c & 31 of word c >> 5 = vocabulary column c), -1 = every class is allowed
    // (pb_batch_decoder_allow, pb_batch_decoder_admit_allow). The two per-row rules sit side by side: the sampler reads them with ONE
    // 8-byte load, so a free row's requests are those of a sampler that knew the bar floor alone
    // ... and rule[b].sched >= 0 = the row follows bar schedule sched of the table stab ((n_sched, nbar) ints in device memory the decoder
    // owns, nbar = pad[0]: entry k = the index in amask of the mask heads 1 .. 7 take in a token of bar k, -1 = the row's own mask), -1 =
    // no schedule (pb_batch_decoder_schedule, pb_batch_decoder_admit_schedule). With it the rules are ONE 16-byte load; `reserved` padded
    // the record to that size
    // ... and rule[b].reserved >= 0 = the row carries anchors (pb_batch_decoder_anchor, pb_batch_decoder_admit_anchor): its value is the
    // row's base in the anchor table atab ((n, 8) int16 ordinary ids, 16 bytes a row, in device memory the decoder owns), acnt[b] the
    // number of its anchors and aplaced[b] the counter k of those written so far -- the one field of a row's rules that the SAMPLER
    // writes, so a rewind restores it (pb_batch_decoder_seek_anchor). -1 = no anchors: the 16-byte rule load is all a free row makes.
    // apad = the first special id of every head: the single-row sampler's kernargs hold none, and an anchored row tests all 8
    struct alignas(16) RowRule { int order, allow, sched, reserved; };
    RowRule rule[BMAX];
    int opad[2];
    int awords;
    const uint32_t* amask;
    int nbar;
    const int* stab;
    int acnt[BMAX];
    int aplaced[BMAX];
    int apad[8];
    const int16_t* atab;
};

// ROWS (the fused decoder's row form, B > 1 rows of x / res / y / ln_out / split records, bf16): the workgroup keeps its weight fragments
// (and gamma / beta) in registers and runs the per-row part below for each row that is not done, requesting the row's input, residual
// and split records after the barrier behind the previous row's reductions: only the shared operands are loaded once. The arithmetic of a
// row is the single-row kernel's (no MFMA: its rounding would differ from the FMA chain).
template <typename T, typename TO, int NCH, bool MERGE, bool ROWS>
__global__ __launch_bounds__(256) void gemv_kernel(const T* __restrict__ W, const T* __restrict__ x, const float* __restrict__ bias,
                                                   TO* __restrict__ y, TO* __restrict__ y2, int n_split, int N, int K, int gelu,
                                                   const T* __restrict__ res, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, T* __restrict__ ln_out, float eps, const MergeIn mg,
                                                   const BState* __restrict__ st, int B) {
    constexpr int EPV = 16 / sizeof(T);
    __shared__ float red[4][2];
    __shared__ float red1[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n0 = blockIdx.x * 2;
    const bool two = n0 + 1 < N;
    const T* w0 = W + (long)n0 * K;
    const T* w1 = W + (long)(two ? n0 + 1 : n0) * K;
    typedef typename VecOf<T>::type V;                                     // EPV elements = 16 bytes, kept as a register vector (no address taken)
    const V zero4 = V{};
    const float bias_v = (threadIdx.x < 2 && (threadIdx.x == 0 || two) && bias) ? bias[n0 + threadIdx.x] : 0.f;   // requested with everything else
    V u0[NCH], u1[NCH], xr[NCH], rr[NCH];
    f32x4 gm[NCH][EPV / 4], bt[NCH][EPV / 4];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = (threadIdx.x + 256 * i) * EPV;
        const bool in = c < K;
        u0[i] = in ? *reinterpret_cast<const V*>(w0 + c) : zero4;
        u1[i] = in ? *reinterpret_cast<const V*>(w1 + c) : zero4;
        if constexpr (!ROWS) {
            xr[i] = (in && !MERGE) ? *reinterpret_cast<const V*>(x + c) : zero4;
            rr[i] = (in && res) ? *reinterpret_cast<const V*>(res + c) : zero4;
        }
#pragma unroll
        for (int v4 = 0; v4 < EPV / 4; ++v4) {
            gm[i][v4] = (in && res) ? *reinterpret_cast<const f32x4*>(gamma + c + 4 * v4) : f32x4{0.f, 0.f, 0.f, 0.f};
            bt[i][v4] = (in && res) ? *reinterpret_cast<const f32x4*>(beta + c + 4 * v4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    for (int b = 0; !ROWS || b < B; ++b) {                                  // rows b = 0 .. B - 1 (one row: no loop at all)
        const T* rb = ROWS && res ? res + (long)b * K : res;
        if constexpr (ROWS) {
            if (st->done[b]) continue;                                      // block-uniform
            __syncthreads();                                                // red / red1 of the previous row are read
            const T* xb = MERGE ? nullptr : x + (long)b * K;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = (threadIdx.x + 256 * i) * EPV;
                const bool in = c < K;
                xr[i] = (in && !MERGE) ? *reinterpret_cast<const V*>(xb + c) : zero4;
                rr[i] = (in && rb) ? *reinterpret_cast<const V*>(rb + c) : zero4;
            }
        }
        float xf[NCH][EPV];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c = (threadIdx.x + 256 * i) * EPV;
            if (MERGE && c < K) {
                const int h = c / mg.hd, off = c % mg.hd;                  // EPV columns of one head (hd is a multiple of EPV)
                const float* rec = mg.part + (size_t)b * mg.row_stride + (size_t)h * mg.nsplit * mg.stride;
                // all loads of the <= PB_DECODE_MAX_SPLITS records are issued before the first use: one L2 round trip, not one per split
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
                    const float wgt = (M == -INFINITY || ms[sp] == -INFINITY) ? 0.f : __expf(ms[sp] - M);   // no visible key in the split (or at all): weight 0
                    L = fmaf(ls[sp], wgt, L);
#pragma unroll
                    for (int j = 0; j < EPV; ++j) o[j] = fmaf(oa[sp][j >> 2][j & 3], wgt, o[j]);
                }
                const float inv = L > 0.f ? 1.0f / L : 0.f;                // nothing visible -> zero row (oracle header)
#pragma unroll
                for (int j = 0; j < EPV; ++j) xf[i][j] = to_f(from_f<T>(o[j] * inv));     // rounded to T like the stored context of the one-kernel form
            } else {
#pragma unroll
                for (int j = 0; j < EPV; ++j) xf[i][j] = to_f(xr[i][j]);
            }
        }
        if (rb) {
            // x' = LayerNorm(res + x) * gamma + beta, two-pass statistics from the registers
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
#pragma unroll
                for (int j = 0; j < EPV; ++j) { xf[i][j] += to_f(rr[i][j]); s += xf[i][j]; }       // lanes beyond K hold zeros
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
                for (int j = 0; j < EPV; ++j) {       // rounded to T exactly like the stored LayerNorm output the unfused path would read back
                    xo[j] = from_f<T>((xf[i][j] - mean) * rstd * gm[i][j >> 2][j & 3] + bt[i][j >> 2][j & 3]);
                    xf[i][j] = to_f(xo[j]);
                }
                if (blockIdx.x == 0 && c < K) *reinterpret_cast<V*>(ln_out + (long)b * K + c) = xo;
            }
        }
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
#pragma unroll
            for (int j = 0; j < EPV; ++j) { a0 = fmaf(to_f(u0[i][j]), xf[i][j], a0); a1 = fmaf(to_f(u1[i][j]), xf[i][j], a1); }    // weights beyond K are zeros
        }
        a0 = wave_sum(a0); a1 = wave_sum(a1);
        if (lane == 0) { red[wave][0] = a0; red[wave][1] = a1; }
        __syncthreads();
        if (threadIdx.x < 2 && (threadIdx.x == 0 || two)) {
            const int n = n0 + threadIdx.x;
            float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x] + bias_v;
            if (gelu) v = gelu_f(v);
            if (ROWS) y[(long)b * N + n] = from_f<TO>(v);
            else if (n < n_split) y[n] = from_f<TO>(v); else y2[n - n_split] = from_f<TO>(v);
        }
        if (!ROWS) break;
    }
}

// ---------------------------------------------------------------- single-query attention over a K/V cache
// One workgroup of 16 waves per head. A key row (hd elements) is CPR = hd*sizeof(T)/16 consecutive 16-byte chunks, one per
// lane, so one wave load covers 64/CPR whole rows as fully used 128/256-byte segments (a row-per-thread layout touched 64
// cache lines per instruction and took 17 us at Sk = 1024). Splitting the keys of a head over several workgroups was
// measured too: the agent-scope release/acquire its last-block merge needs costs an L2 write-back + invalidate per launch
// on this multi-XCD part (20 us), more than the parallelism returns at these sizes.
constexpr int AD_WAVES = 16;

// CPR = lanes per key row (a power of two), CR = 16-byte chunks a row really has (head_dim 96: 12 of 16 bf16 / 24 of 32 f32 lanes
// carry data, the others hold zeros and load nothing).
template <typename T, int CPR, int CR = CPR>
__global__ __launch_bounds__(AD_WAVES * 64) void attn_decode_kernel(const T* __restrict__ q, const T* __restrict__ kc,
                                                                    const T* __restrict__ vc, T* __restrict__ out,
                                                                    const float* __restrict__ key_mask, int Sk, long k_ss, long v_ss,
                                                                    float scale) {
    constexpr int EPV = 16 / sizeof(T), HD = CR * EPV, KPW = 64 / CPR;        // keys per wave-wide load
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);            // [Sk] scores -> probabilities
    float* red = sc + ((Sk + 3) & ~3);                     // [16] reductions, then [16][HD] partial outputs
    const int h = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, sub = lane % CPR, grp = lane / CPR;
    const bool live = CR == CPR || sub < CR;
    float qv[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) qv[e] = 0.f;
    if (live) {
        T qq[EPV];
        *reinterpret_cast<uint4*>(qq) = *reinterpret_cast<const uint4*>(q + h * HD + sub * EPV);
#pragma unroll
        for (int e = 0; e < EPV; ++e) qv[e] = to_f(qq[e]) * scale;
    }
    float mx = -INFINITY;
    constexpr int UR = 8, STEP = AD_WAVES * KPW;           // UR row-chunk loads in flight per lane before the first use
    for (int jb = wave * KPW; jb < Sk; jb += UR * STEP) {
        uint4 kraw[UR];
#pragma unroll
        for (int r = 0; r < UR; ++r) {
            const int j = jb + r * STEP + grp;
            kraw[r] = uint4{0u, 0u, 0u, 0u};
            if (j < Sk && live) kraw[r] = *reinterpret_cast<const uint4*>(kc + (long)j * k_ss + h * HD + sub * EPV);
        }
#pragma unroll
        for (int r = 0; r < UR; ++r) {
            const int j = jb + r * STEP + grp;
            float a = 0.f;
            if (j < Sk) {
                const T* kv = reinterpret_cast<const T*>(&kraw[r]);
#pragma unroll
                for (int e = 0; e < EPV; ++e) a = fmaf(to_f(kv[e]), qv[e], a);
            }
#pragma unroll
            for (int o = 1; o < CPR; o <<= 1) a += __shfl_xor(a, o, 64);
            if (j < Sk) {
                const float sv = (!key_mask || key_mask[j] != 0.f) ? a : -INFINITY;
                if (sub == 0) sc[j] = sv;
                mx = fmaxf(mx, sv);
            }
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w2 = 1; w2 < AD_WAVES; ++w2) mx = fmaxf(mx, red[w2]);
    __syncthreads();
    float sum = 0.f;
    if (mx != -INFINITY)
        for (int j = t; j < Sk; j += AD_WAVES * 64) { const float e = __expf(sc[j] - mx); sc[j] = e; sum += e; }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    sum = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < AD_WAVES; ++w2) sum += red[w2];
    const float inv = (mx != -INFINITY && sum > 0.f) ? 1.0f / sum : 0.f;       // nothing visible -> zero row (oracle header)
    __syncthreads();
    // o[c] = sum_j p_j V[j][c]: same row-chunk ownership; a lane keeps the EPV columns of its chunk
    float acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.f;
    if (inv > 0.f)
        for (int jb = wave * KPW; jb < Sk; jb += UR * STEP) {
            uint4 vraw[UR];
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                const int j = jb + r * STEP + grp;
                vraw[r] = uint4{0u, 0u, 0u, 0u};
                if (j < Sk && live) vraw[r] = *reinterpret_cast<const uint4*>(vc + (long)j * v_ss + h * HD + sub * EPV);
            }
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                const int j = jb + r * STEP + grp;
                if (j < Sk) {
                    const T* vv = reinterpret_cast<const T*>(&vraw[r]);
                    const float pj = sc[j];
#pragma unroll
                    for (int e = 0; e < EPV; ++e) acc[e] = fmaf(pj, to_f(vv[e]), acc[e]);
                }
            }
        }
#pragma unroll
    for (int e = 0; e < EPV; ++e)
#pragma unroll
        for (int o = CPR; o < 64; o <<= 1) acc[e] += __shfl_xor(acc[e], o, 64);
    if (grp == 0 && live)
#pragma unroll
        for (int e = 0; e < EPV; ++e) red[wave * HD + sub * EPV + e] = acc[e];
    __syncthreads();
    if (t < HD) {
        float o = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < AD_WAVES; ++w2) o += red[w2 * HD + t];
        out[h * HD + t] = from_f<T>(o * inv);
    }
}


// ---------------------------------------------------------------- single-query attention, keys split over workgroups
// The one-workgroup-per-head form above keeps 12 of 256 CUs busy at cfg 2 (10.7 us per call, 24 calls per token = 40 % of the
// decode step's GPU time). Here a (head, key-split) pair is one 4-wave workgroup: it computes the scores of its <= `chunk` keys,
// their local maximum m, l = sum e^(s - m) and o = sum e^(s - m) v (unnormalised) and stores {m, l, -, -, o[hd]} as f32; the consumer
// GEMV merges the splits in its prologue (gemv_kernel / MergeIn). Same row-chunk ownership of the cached K / V rows as above.
constexpr int AS_WAVES = 4;
template <typename T, int CPR, int CR = CPR>
__global__ __launch_bounds__(AS_WAVES * 64) void attn_split_kernel(const T* __restrict__ q, const T* __restrict__ kc, const T* __restrict__ vc,
                                                                   float* __restrict__ part, const float* __restrict__ key_mask, int Sk, int chunk,
                                                                   long k_ss, long v_ss, float scale) {
    constexpr int EPV = 16 / sizeof(T), HD = CR * EPV, KPW = 64 / CPR, STEP = AS_WAVES * KPW, UR = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = reinterpret_cast<float*>(smem);            // [chunk] scores -> probabilities
    float* red = sc + ((chunk + 3) & ~3);                  // [AS_WAVES] reductions, then [AS_WAVES][HD] partial outputs
    const int h = blockIdx.x, sp = blockIdx.y, nsplit = gridDim.y;
    const int j0 = sp * chunk, j1 = min(Sk, j0 + chunk);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, sub = lane % CPR, grp = lane / CPR;
    const bool live = CR == CPR || sub < CR;
    float qv[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) qv[e] = 0.f;
    if (live) {
        T qq[EPV];
        *reinterpret_cast<uint4*>(qq) = *reinterpret_cast<const uint4*>(q + h * HD + sub * EPV);
#pragma unroll
        for (int e = 0; e < EPV; ++e) qv[e] = to_f(qq[e]) * scale;
    }
    float mx = -INFINITY;
    const int jfirst = j0 + wave * KPW;
    uint4 vpre[UR];                                        // V rows of the first (usually the only) block, requested together with its K rows
    for (int jb = jfirst; jb < j1; jb += UR * STEP) {
        uint4 kraw[UR];
#pragma unroll
        for (int r = 0; r < UR; ++r) {
            const int j = jb + r * STEP + grp;
            kraw[r] = uint4{0u, 0u, 0u, 0u};
            if (j < j1 && live) kraw[r] = *reinterpret_cast<const uint4*>(kc + (long)j * k_ss + h * HD + sub * EPV);
        }
        if (jb == jfirst) {
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                const int j = jb + r * STEP + grp;
                vpre[r] = uint4{0u, 0u, 0u, 0u};
                if (j < j1 && live) vpre[r] = *reinterpret_cast<const uint4*>(vc + (long)j * v_ss + h * HD + sub * EPV);
            }
        }
#pragma unroll
        for (int r = 0; r < UR; ++r) {
            const int j = jb + r * STEP + grp;
            float a = 0.f;
            if (j < j1) {
                const T* kv = reinterpret_cast<const T*>(&kraw[r]);
#pragma unroll
                for (int e = 0; e < EPV; ++e) a = fmaf(to_f(kv[e]), qv[e], a);
            }
#pragma unroll
            for (int o = 1; o < CPR; o <<= 1) a += __shfl_xor(a, o, 64);
            if (j < j1) {
                const float sv = (!key_mask || key_mask[j] != 0.f) ? a : -INFINITY;
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
        for (int j = t; j < j1 - j0; j += AS_WAVES * 64) { const float e = __expf(sc[j] - mx); sc[j] = e; sum += e; }
    sum = wave_sum(sum);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    sum = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    float acc[EPV];
#pragma unroll
    for (int e = 0; e < EPV; ++e) acc[e] = 0.f;
    if (mx != -INFINITY)
        for (int jb = jfirst; jb < j1; jb += UR * STEP) {
            uint4 vraw[UR];
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                const int j = jb + r * STEP + grp;
                vraw[r] = vpre[r];
                if (jb != jfirst) {
                    vraw[r] = uint4{0u, 0u, 0u, 0u};
                    if (j < j1 && live) vraw[r] = *reinterpret_cast<const uint4*>(vc + (long)j * v_ss + h * HD + sub * EPV);
                }
            }
#pragma unroll
            for (int r = 0; r < UR; ++r) {
                const int j = jb + r * STEP + grp;
                if (j < j1) {
                    const T* vv = reinterpret_cast<const T*>(&vraw[r]);
                    const float pj = sc[j - j0];
#pragma unroll
                    for (int e = 0; e < EPV; ++e) acc[e] = fmaf(pj, to_f(vv[e]), acc[e]);
                }
            }
        }
#pragma unroll
    for (int e = 0; e < EPV; ++e)
#pragma unroll
        for (int o = CPR; o < 64; o <<= 1) acc[e] += __shfl_xor(acc[e], o, 64);
    if (grp == 0 && live)
#pragma unroll
        for (int e = 0; e < EPV; ++e) red[wave * HD + sub * EPV + e] = acc[e];
    __syncthreads();
    float* rec = part + ((size_t)h * nsplit + sp) * (HD + 4);          // {m, l, -, -, o[HD]}: o starts 16-byte aligned
    if (t == 0) { rec[0] = mx; rec[1] = sum; }
    if (t < HD) rec[4 + t] = (red[t] + red[HD + t]) + (red[2 * HD + t] + red[3 * HD + t]);
}

}  // namespace

struct LnIn { const void* res; const float* gamma; const float* beta; void* out; };

// st / B > 1: the fused decoder's row form (bf16; y, ln_out and the split records of row b at + b N, + b K, + b mg.row_stride)
static int gemv_launch(const void* W, const void* x, const float* bias, void* y, void* y2, int n_split, int N, int K, int dtype, int y_f32,
                       int gelu, hipStream_t stream, LnIn ln = LnIn{nullptr, nullptr, nullptr, nullptr}, MergeIn mg = MergeIn{nullptr, 0, 0, 0, 0},
                       const BState* st = nullptr, int B = 1) {
    const int epv = dtype == PB_BF16 ? 8 : 4;
    PB_REQUIRE(N > 0 && K > 0 && K % epv == 0, "pb_gemv: K=%d must be a multiple of %d", K, epv);
    PB_REQUIRE(((uintptr_t)W % 16 == 0) && ((uintptr_t)x % 16 == 0), "pb_gemv: operands must be 16-byte aligned");
    PB_REQUIRE(B == 1 || (dtype == PB_BF16 && st), "pb_gemv: rows need bf16 and the decoder state");
    dim3 grid((N + 1) / 2), block(256);
    const float eps = 1e-5f;
    const int nch = (K + 256 * epv - 1) / (256 * epv);
    PB_REQUIRE(nch <= 4, "pb_gemv: K=%d exceeds %d", K, 4 * 256 * epv);
#define PB_GEMV_GO(TT, TO, NCH_, MG_, ROWS_)                                                                                               \
    hipLaunchKernelGGL((gemv_kernel<TT, TO, NCH_, MG_, ROWS_>), grid, block, 0, stream, (const TT*)W, (const TT*)x, bias, (TO*)y, (TO*)y2, n_split, \
                       N, K, gelu, (const TT*)ln.res, ln.gamma, ln.beta, (TT*)ln.out, eps, mg, st, B)
#define PB_GEMV_NCH(TT, TO, ROWS_)                                                                            \
    do {                                                                                                      \
        if (mg.part) { PB_REQUIRE(nch <= 1, "pb_gemv: the split-merge prologue needs K <= %d", 256 * epv); PB_GEMV_GO(TT, TO, 1, true, ROWS_); } \
        else if (nch <= 1) PB_GEMV_GO(TT, TO, 1, false, ROWS_);                                               \
        else if (nch == 2) PB_GEMV_GO(TT, TO, 2, false, ROWS_);                                               \
        else PB_GEMV_GO(TT, TO, 4, false, ROWS_);                                                             \
    } while (0)
    if (dtype == PB_BF16 && B > 1) {
        if (y_f32) PB_GEMV_NCH(bf16_t, float, true); else PB_GEMV_NCH(bf16_t, bf16_t, true);
    } else if (dtype == PB_BF16) {
        if (y_f32) PB_GEMV_NCH(bf16_t, float, false); else PB_GEMV_NCH(bf16_t, bf16_t, false);
    } else {
        PB_GEMV_NCH(float, float, false);
    }
#undef PB_GEMV_NCH
#undef PB_GEMV_GO
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_gemv(const void* W, const void* x, const float* bias, void* y, int32_t N, int32_t K, int32_t dtype, int32_t y_f32,
                       int32_t gelu, void* stream_) {
    return gemv_launch(W, x, bias, y, nullptr, N, N, K, dtype, y_f32, gelu, (hipStream_t)stream_);
}

template <typename T, int CPR, int CR = CPR>
static void attn_decode_launch(const void* q, const void* kc, const void* vc, void* out, const float* key_mask, int H, int Sk, long k_ss,
                               long v_ss, float scale, hipStream_t stream) {
    constexpr int HD = CR * (16 / (int)sizeof(T));
    const size_t lds = (size_t)(((Sk + 3) & ~3) + AD_WAVES * HD) * sizeof(float);
    hipLaunchKernelGGL((attn_decode_kernel<T, CPR, CR>), dim3(H), dim3(AD_WAVES * 64), lds, stream, (const T*)q, (const T*)kc, (const T*)vc, (T*)out,
                       key_mask, Sk, k_ss, v_ss, scale);
}

extern "C" int pb_attn_decode(const void* q, const void* k_cache, const void* v_cache, void* out, const float* key_mask, int32_t H, int32_t Sk,
                              int32_t hd, int64_t k_ss, int64_t v_ss, float scale, int32_t dtype, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PB_REQUIRE(H > 0 && Sk > 0 && Sk <= 8192 && (hd == 32 || hd == 64 || hd == 96 || hd == 128),
               "pb_attn_decode: H=%d Sk=%d hd=%d (head_dim must be 32, 64, 96 or 128; Sk <= 8192)", H, Sk, hd);
    const int epv = dtype == PB_BF16 ? 8 : 4;
    PB_REQUIRE(k_ss % epv == 0 && v_ss % epv == 0 && ((uintptr_t)k_cache % 16 == 0) && ((uintptr_t)v_cache % 16 == 0) && ((uintptr_t)q % 16 == 0),
               "pb_attn_decode: rows must be 16-byte aligned");
    if (dtype == PB_BF16) {
        if (hd == 32) attn_decode_launch<bf16_t, 4>(q, k_cache, v_cache, out, key_mask, H, Sk, k_ss, v_ss, scale, stream);
        else if (hd == 64) attn_decode_launch<bf16_t, 8>(q, k_cache, v_cache, out, key_mask, H, Sk, k_ss, v_ss, scale, stream);
        else if (hd == 96) attn_decode_launch<bf16_t, 16, 12>(q, k_cache, v_cache, out, key_mask, H, Sk, k_ss, v_ss, scale, stream);
        else attn_decode_launch<bf16_t, 16>(q, k_cache, v_cache, out, key_mask, H, Sk, k_ss, v_ss, scale, stream);
    } else {
        if (hd == 32) attn_decode_launch<float, 8>(q, k_cache, v_cache, out, key_mask, H, Sk, k_ss, v_ss, scale, stream);
        else if (hd == 64) attn_decode_launch<float, 16>(q, k_cache, v_cache, out, key_mask, H, Sk, k_ss, v_ss, scale, stream);
        else if (hd == 96) attn_decode_launch<float, 32, 24>(q, k_cache, v_cache, out, key_mask, H, Sk, k_ss, v_ss, scale, stream);
        else attn_decode_launch<float, 32>(q, k_cache, v_cache, out, key_mask, H, Sk, k_ss, v_ss, scale, stream);
    }
    PB_LAUNCH_CHECK();
    return 0;
}

// key-split single-query attention into `part` (H * nsplit records of hd + 4 floats); returns the number of splits used
template <typename T, int CPR, int CR = CPR>
static void attn_split_launch(const void* q, const void* kc, const void* vc, float* part, const float* key_mask, int H, int Sk, int chunk, int nsplit,
                              long k_ss, long v_ss, float scale, hipStream_t stream) {
    constexpr int HD = CR * (16 / (int)sizeof(T));
    const size_t lds = (size_t)(((chunk + 3) & ~3) + AS_WAVES * HD) * sizeof(float);
    hipLaunchKernelGGL((attn_split_kernel<T, CPR, CR>), dim3(H, nsplit), dim3(AS_WAVES * 64), lds, stream, (const T*)q, (const T*)kc, (const T*)vc, part,
                       key_mask, Sk, chunk, k_ss, v_ss, scale);
}
static int attn_split(const void* q, const void* kc, const void* vc, float* part, const float* key_mask, int H, int Sk, int hd, long k_ss, long v_ss,
                      float scale, int dtype, hipStream_t stream, int& nsplit) {
    // <= PB_DECODE_MAX_SPLITS splits of >= 64 keys: H * nsplit workgroups cover the chip at cfg 2 from 512 keys on
    int chunk = (Sk + PB_DECODE_MAX_SPLITS - 1) / PB_DECODE_MAX_SPLITS;
    chunk = chunk < 64 ? 64 : (chunk + 15) & ~15;
    nsplit = (Sk + chunk - 1) / chunk;
    if (dtype == PB_BF16) {
        if (hd == 32) attn_split_launch<bf16_t, 4>(q, kc, vc, part, key_mask, H, Sk, chunk, nsplit, k_ss, v_ss, scale, stream);
        else if (hd == 64) attn_split_launch<bf16_t, 8>(q, kc, vc, part, key_mask, H, Sk, chunk, nsplit, k_ss, v_ss, scale, stream);
        else if (hd == 96) attn_split_launch<bf16_t, 16, 12>(q, kc, vc, part, key_mask, H, Sk, chunk, nsplit, k_ss, v_ss, scale, stream);
        else attn_split_launch<bf16_t, 16>(q, kc, vc, part, key_mask, H, Sk, chunk, nsplit, k_ss, v_ss, scale, stream);
    } else {
        if (hd == 32) attn_split_launch<float, 8>(q, kc, vc, part, key_mask, H, Sk, chunk, nsplit, k_ss, v_ss, scale, stream);
        else if (hd == 64) attn_split_launch<float, 16>(q, kc, vc, part, key_mask, H, Sk, chunk, nsplit, k_ss, v_ss, scale, stream);
        else if (hd == 96) attn_split_launch<float, 32, 24>(q, kc, vc, part, key_mask, H, Sk, chunk, nsplit, k_ss, v_ss, scale, stream);
        else attn_split_launch<float, 32>(q, kc, vc, part, key_mask, H, Sk, chunk, nsplit, k_ss, v_ss, scale, stream);
    }
    PB_LAUNCH_CHECK();
    return 0;
}

// ---------------------------------------------------------------- one decoder token, natively sequenced
extern "C" int pb_decode_step(const pb_decode_plan* p, int32_t i, void* stream) {
    PB_REQUIRE(p && p->n_layers > 0 && p->n_layers <= PB_DECODE_MAX_LAYERS, "pb_decode_step: bad plan");
    PB_REQUIRE(i >= 0 && i < p->S, "pb_decode_step: step %d outside 0..%d", i, p->S - 1);
    const int d = p->d, H = p->H, hd = d / H, f = p->ffn, dt = p->dtype;
    const size_t esz = dt == PB_BF16 ? 2 : 4;
    const float scale = 1.0f / sqrtf((float)hd);
    const int32_t* seg = p->tab_off;
    char* x = (char*)p->x; char* alt = (char*)p->y2;
    // token embedding + position i + LayerNorm (S = 1 with the position table advanced by i rows)
    if (pb_embed_ln_fwd(p->tok16, p->ptab, seg, p->lin_b, p->pos + (size_t)i * d, p->lne_w, p->lne_b, x, p->stat, p->stat + 1, 1, 1, d, dt,
                        1e-5f, 0, 0, 0.f, stream)) return -1;
    hipStream_t st = (hipStream_t)stream;
    LnIn ln{nullptr, nullptr, nullptr, nullptr};            // pending post-LN of the previous sub-layer, applied by the next GEMV
    char* h = x;
    for (int l = 0; l < p->n_layers; ++l) {
        const pb_decode_layer& L = p->layers[l];
        char* kvs = (char*)L.kv_self;
        // q | k|v in one launch; k|v land in row i of the self-attention cache. Input: h (layer 0) or LN2 of the layer below.
        if (gemv_launch(L.wqkv, ln.res ? (const void*)p->a : (const void*)h, L.bqkv, p->q, kvs + (size_t)i * 2 * d * esz, d, 3 * d, d, dt, 0, 0, st, ln)) return -1;
        if (ln.res) h = alt;
        int ns = 0;
        if (p->attn_part) {                                // keys split over workgroups, merged in the out-projection's prologue
            if (attn_split(p->q, kvs, kvs + (size_t)d * esz, p->attn_part, nullptr, H, i + 1, hd, 2 * d, 2 * d, scale, dt, st, ns)) return -1;
            if (gemv_launch(L.wo, p->ctx, L.bo, p->a, nullptr, d, d, d, dt, 0, 0, st, LnIn{nullptr, nullptr, nullptr, nullptr}, MergeIn{p->attn_part, ns, hd, hd + 4})) return -1;
        } else {
            if (pb_attn_decode(p->q, kvs, kvs + (size_t)d * esz, p->ctx, nullptr, H, i + 1, hd, 2 * d, 2 * d, scale, dt, stream)) return -1;
            if (pb_gemv(L.wo, p->ctx, L.bo, p->a, d, d, dt, 0, 0, stream)) return -1;
        }
        // cross attention against the cached encoder K/V; the q projection applies LN1(h + a) -> y1
        ln = LnIn{h, L.ln1_w, L.ln1_b, p->y1};
        if (gemv_launch(L.wq_c, p->a, L.bq_c, p->q, nullptr, d, d, d, dt, 0, 0, st, ln)) return -1;
        if (p->attn_part) {
            if (attn_split(p->q, L.kv_cross, (const char*)L.kv_cross + (size_t)d * esz, p->attn_part, p->enc_mask, H, p->S_enc, hd, 2 * d, 2 * d, scale, dt, st, ns)) return -1;
            if (gemv_launch(L.wo_c, p->ctx, L.bo_c, p->a, nullptr, d, d, d, dt, 0, 0, st, LnIn{nullptr, nullptr, nullptr, nullptr}, MergeIn{p->attn_part, ns, hd, hd + 4})) return -1;
        } else {
            if (pb_attn_decode(p->q, L.kv_cross, (const char*)L.kv_cross + (size_t)d * esz, p->ctx, p->enc_mask, H, p->S_enc, hd, 2 * d, 2 * d, scale, dt, stream)) return -1;
            if (pb_gemv(L.wo_c, p->ctx, L.bo_c, p->a, d, d, dt, 0, 0, stream)) return -1;
        }
        // FFN; fc1 applies LNc(y1 + a) -> yc
        ln = LnIn{p->y1, L.lnc_w, L.lnc_b, p->yc};
        if (gemv_launch(L.w1, p->a, L.b1, p->g, nullptr, f, f, d, dt, 0, 1, st, ln)) return -1;
        if (pb_gemv(L.w2, p->g, L.b2, p->a, d, f, dt, 0, 0, stream)) return -1;
        ln = LnIn{p->yc, L.ln2_w, L.ln2_b, alt};            // LN2(yc + a) -> next layer's h, applied by its q|k|v GEMV (or the heads)
    }
    return gemv_launch(p->head_w, p->a, p->head_b, p->logits, nullptr, p->vocab, p->vocab, d, dt, 1, 0, st, ln);
}


// =====================================================================================================================
// Decode, second form: the fused decoder (pb_batch_decoder_*). One step = ONE hipGraph replay of 6 launches per decoder layer
// (+ embed + heads, + the device sampler). What changed against pb_decode_step above:
//   * the positions live in DEVICE memory (advanced by the first kernel of a step), so the launches of a step have no
//     position-dependent argument or grid and one captured graph serves every position: the host's ~3.5 us of enqueue per launch
//     (host-bound with kernels this short) become one hipGraphLaunch per token;
//   * the q projection is fused into the single-query attention (dec_attn_kernel): a (head, key split) workgroup needs q of ITS
//     head only (hd rows of W_q, 98 KB at cfg 2: re-read by the <= 16 splits of a head from L2), so it applies the pending post-LN
//     itself, projects q_h, and goes on to its keys -- the q|k|v GEMV launch and its all-to-all seam are gone. For the self-attention
//     one more workgroup per head projects k_h and v_h of the new token as well, writes them to the cache row and contributes
//     the new token's own {score, 1, v} record, so the regular splits only read rows that older launches wrote;
//   * per layer: self-attn(+LN2 of the layer below, q|k|v) -> out-proj (merges the split records) -> cross-attn(+LN1, q_c) ->
//     out_c (merge) -> fc1 (+LNc, GELU) -> fc2. Every remaining boundary is a real all-to-all seam (each output needs the whole
//     input vector, produced by all workgroups of the launch before): cdna_hip_programming.md 5.6 prices a grid barrier above a
//     kernel boundary, so they stay launches.
// Rows: 1 <= B <= PB_DECODE_BATCH_MAX prompts go through the same launches, so a step reads each weight byte once for all of them. Each
// kernel is one template with a ROWS switch. The single-row instance (ROWS = false, launched at B == 1) has the row fixed at 0, no done /
// limit checks and every load issued up front: the batch-1 token is pure latency. The row instance takes its row from the grid (embedding,
// attention, sampler) or loops over the rows (bgemv_kernel), addresses row b's slice of the scratch rows, caches and split records, and
// skips rows that are done. The arithmetic of a row is the same source in both, so a row's logits do not depend on B
// (tests/test_generate_batch_gpu.py).
// Per-row state in device memory (BState): pos[b], and for the row form done[b] (the sampler's special id, the position limit, or the
// host) and the limit, so rows advance, stop and rewind independently; a done row writes nothing, never a row past S - 1. At B == 1 the
// host keeps the count of enqueued positions instead.
// bf16, head_dim 64 or 128, d a multiple of 256 up to 1024; anything else keeps pb_decode_step.
namespace {

__device__ __forceinline__ float half_sum(float v) {            // sum over the 32 lanes of a half-wave, in every lane of it
    v += PB_DPP_F(v, 0xb1);
    v += PB_DPP_F(v, 0x4e);
    v += PB_DPP_F(v, 0x141);
    v += PB_DPP_F(v, 0x140);
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(a[0]) + __uint_as_float(a[1]);
}

// ---------------------------------------------------------------- single-query attention with the q projection, (head, key split, row) workgroups
// The arguments of the two forms share their first fields; each form's member order is its kernarg layout.
struct DecAttnCommon {
    const bf16_t* x_in;                                          // the input vector (d) when res == NULL
    const bf16_t* res; const bf16_t* add; const float* gamma; const float* beta; bf16_t* ln_out;   // x' = LN(res + add) gamma + beta
    const bf16_t* Wq; const float* bq;                           // q projection rows [d][d] (+ bias); head h owns rows h HD ..
    const bf16_t* Wk; const float* bk; const bf16_t* Wv; const float* bv;      // SELF: the new token's k / v rows
    bf16_t* kc; bf16_t* vc; long kv_ss;                          // cached rows: kc + j kv_ss + h HD
};
template <bool ROWS> struct DecAttnArgs;
template <> struct DecAttnArgs<false> : DecAttnCommon {
    const float* key_mask;                                       // cross: [Sk] (0 = masked) or NULL
    BState* st;                                                  // SELF: keys cached so far = pos[0], row pos[0] is written
    int Sk_fixed;                                                // cross: Sk_fixed keys
    int d, nreg, ck_fixed;                                       // regular key splits; cross: keys per split
    float scale, eps;
    float* part;                                                 // [H][gridDim.y][HD + 4] records {m, l, -, -, o[HD]}
    static constexpr long kv_rs = 0, mask_rs = 0, part_rs = 0;
    __device__ int s_enc(int) const { return Sk_fixed; }
    __device__ int ck(int) const { return ck_fixed; }
    __device__ int kv_row(int) const { return 0; }
};
template <> struct DecAttnArgs<true> : DecAttnCommon {           // x_in, res, add, ln_out: (B, d) rows
    long kv_rs;                                                  // row b's cached rows at kc / vc + b kv_rs
    const float* key_mask; long mask_rs;                         // cross: row b's (Sk) mask at key_mask + b mask_rs, or NULL
    BState* st;
    int d, nreg;
    float scale, eps;
    float* part; long part_rs;                                   // row b's records at part + b part_rs
    int s_enc_[BMAX], ck_[BMAX];                                 // cross: keys and keys per split of each row
    int kv_row_[BMAX];                                           // cross: row b attends to slice kv_row_[b] of kc / vc (pb_batch_decoder_share_cross;
                                                                 // b itself without it); the self-attention cache is always the row's own
    __device__ int s_enc(int b) const { return s_enc_[b]; }
    __device__ int ck(int b) const { return ck_[b]; }
    __device__ int kv_row(int b) const { return kv_row_[b]; }
};
// The dynamic form (pb_batch_decoder_dynamic): a row's cross-attention geometry lives in BState, so a slot can change its prompt between two
// replays of a captured graph (pb_batch_decoder_admit). The kernel loads done[b] and pos[b] from the same struct anyway.
struct DecAttnDynArgs : DecAttnCommon {
    long kv_rs;
    const float* key_mask; long mask_rs;
    BState* st;
    int d, nreg;
    float scale, eps;
    float* part; long part_rs;
    __device__ int s_enc(int b) const { return st->s_enc[b]; }
    __device__ int ck(int b) const { return st->ck[b]; }
    __device__ int kv_row(int b) const { return st->kv_row[b]; }
};
// The grouped cross-attention form (dec_attn_group_kernel): the rows ordered by their cross K|V slice and cut into tiles of <= RT rows of
// one slice; tile t = rows_[tile_first[t] .. + tile_n[t]).
struct DecAttnGroupArgs : DecAttnArgs<true> {
    int rows_[BMAX], tile_first[BMAX], tile_n[BMAX];
};

// Threads: 256; the self-attention form launches 768 so that the new token's workgroup projects q, k and v side by side (wave
// groups 0 / 1 / 2, every weight load of a group in flight at once: ONE memory round trip instead of six dependent ones -- these
// kernels are pure latency); in the other workgroups of that launch waves 4 .. 11 leave at once.
// A = the argument form: DecAttnArgs<ROWS>, or DecAttnDynArgs for the cross-attention of a dynamic decoder (same body, the three geometry
// accessors read device memory).
template <int NC, int HD, bool SELF, bool ROWS, typename A = DecAttnArgs<ROWS>>
__global__ __launch_bounds__(SELF ? 768 : 256) void dec_attn_kernel(const A a) {
    constexpr int CPR = HD / 8, KPW = 64 / CPR, STEP = 4 * KPW, UR = 4, RPW = HD / 4, NP = RPW / 2;
    constexpr int PBATCH = (NC <= 3 && !SELF) || NC <= 2 ? (NP < 8 ? NP : 8) : 4;       // passes of weight rows in flight per lane (registers)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qs = reinterpret_cast<float*>(smem);                  // [HD] q of this head, rounded to bf16 like a stored q row, times the softmax scale
    float* red = qs + HD;                                        // [4 HD] reductions / per-wave partial outputs (new-token workgroup: k | v)
    float* sc = red + 4 * HD;                                    // [keys per split] scores -> probabilities
    const int h = blockIdx.x, sp = blockIdx.y, nrec = gridDim.y, b = ROWS ? (int)blockIdx.z : 0;
    if (ROWS && a.st->done[b]) return;                           // block-uniform: a done row writes no K/V row and no record
    const int t = threadIdx.x, lane = t & 63, l32 = lane & 31, half = lane >> 5;
    const int wgrp = SELF ? (int)(t >> 8) : 0;                   // 0: q (and the attention), 1: k, 2: v of the new token
    const int wave = (t >> 6) & 3;
    const int d = a.d;
    const int Sk = SELF ? a.st->pos[b] : a.s_enc(b);
    const bool is_new = SELF && sp == a.nreg;
    if (SELF && wgrp > 0 && !is_new) return;                     // only the new token's workgroup uses the other two wave groups
    const int kvb = SELF ? b : a.kv_row(b);                      // the slice of the cache this row reads (cross: may be shared with other rows)
    bf16_t* const kc = a.kc + (long)kvb * a.kv_rs;
    bf16_t* const vc = a.vc + (long)kvb * a.kv_rs;
    const float* const key_mask = a.key_mask ? a.key_mask + (long)b * a.mask_rs : nullptr;
    int ck = SELF ? 0 : a.ck(b);
    if (SELF) { ck = (Sk + a.nreg - 1) / a.nreg; ck = ck < 64 ? 64 : (ck + 15) & ~15; }
    const int j0 = sp * ck, j1 = min(Sk, j0 + ck);
    float* rec = a.part + (long)b * a.part_rs + ((size_t)h * nrec + sp) * (HD + 4);
    if (!is_new && j0 >= Sk) {                                   // no key in this split: a record of weight zero
        if (t == 0) { rec[0] = -INFINITY; rec[1] = 0.f; }
        if (t < HD) rec[4 + t] = 0.f;
        return;
    }
    const int tq = t & 255;                                       // thread index inside its wave group
    // cached rows of the first block of this split: requested before anything else (they do not depend on q)
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
    // the input vector, whole, in every half-wave: lane l32 holds the 8 elements of chunks l32 + 32 c
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
            for (int j = 0; j < 8; ++j) {                        // rounded to bf16 like the stored LayerNorm output the residual path reads back
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
    // HD rows of a projection: a half-wave per row (2 rows per pass and wave), 4 passes of weight loads in flight
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
            kc[(long)Sk * a.kv_ss + h * HD + t] = (bf16_t)ks[t];         // Sk < S (row form: < limit, the embedding kernel's guard)
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

// ---------------------------------------------------------------- grouped cross-attention: (head, key split, row tile) workgroups
// Rows that share one slice of the cross K|V cache (samples of one prompt, pb_batch_decoder_share_cross) go through ONE workgroup per
// (head, key split) in tiles of <= RT rows: the 16-byte K and V chunks of the split, the head's W_q rows and b_q are loaded once and
// applied to every live row of the tile, where the per-row form streams them once per row. What a row computes is the per-row kernel's,
// operation for operation: LN1 in a half-wave, the projection's fma chain over (chunk, element) and its half_sum, the same lane -> key
// mapping, fma / shuffle order of the scores, block maximum, __expf and sum order, the P V chain and the wave / block reductions -- so each
// row's {m, l, o[HD]} record, and with the unchanged out-projection merge its logits, are bit-identical to the per-row form's
// (tests/test_samples_per_prompt_gpu.py). Per-row state between the phases: LN1 output as bf16 in LDS (it is rounded to bf16 anyway), q,
// scores and reduction scratch in LDS per row; maxima, sums and the RT x 8 output accumulators in registers. RT is the row tile: the
// accumulators, the PBATCH x NC weight fragments of the projection and the K / V chunks in flight bound it (RT = 8: 64 + 96 + 32 VGPRs at
// NC = 3), and every row of a tile runs in series behind one workgroup's loads, so a small tile also keeps more workgroups in flight.
// The rows of a tile have one prompt: equal s_enc, hence equal split geometry, and equal mask rows (read through the tile's first live row).
// Done rows are skipped; a tile without a live row writes nothing. ln_out is written once per row (by the head-0, split-0 workgroup).
template <int NC, int HD, int RT>
__global__ __launch_bounds__(256) void dec_attn_group_kernel(const DecAttnGroupArgs a) {
    constexpr int CPR = HD / 8, KPW = 64 / CPR, STEP = 4 * KPW, UR = 4, RPW = HD / 4, NP = RPW / 2;
    constexpr int PBATCH = NC <= 3 ? (NP < 8 ? NP : 8) : 4;      // as the per-row cross form
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int d = a.d;
    const int h = blockIdx.x, sp = blockIdx.y, nrec = gridDim.y, tile = blockIdx.z;
    const int first = a.tile_first[tile], nrow = a.tile_n[tile];
    int rowb[RT];
    bool lv[RT];
    int b0 = -1;                                                 // first live row: the tile's geometry, cache slice and mask
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        rowb[r] = r < nrow ? a.rows_[first + r] : 0;
        lv[r] = r < nrow && !a.st->done[rowb[r]];                // block-uniform
        if (lv[r] && b0 < 0) b0 = rowb[r];
    }
    if (b0 < 0) return;
    const int Sk = a.s_enc(b0), ck = a.ck(b0), ckp = (ck + 3) & ~3;
    float* qs = reinterpret_cast<float*>(smem);                  // [RT][HD] q of this head per row, bf16-rounded, times the softmax scale
    float* red = qs + RT * HD;                                   // [RT][4 HD] reductions / per-wave partial outputs
    bf16_t* xs = reinterpret_cast<bf16_t*>(red + RT * 4 * HD);   // [RT][d] LN1 output rows
    float* sc = reinterpret_cast<float*>(xs + (size_t)RT * d);   // [RT][ckp] scores -> probabilities
    const int t = threadIdx.x, lane = t & 63, l32 = lane & 31, half = lane >> 5, wave = t >> 6;
    const bf16_t* const kc = a.kc + (long)a.kv_row(b0) * a.kv_rs;
    const bf16_t* const vc = a.vc + (long)a.kv_row(b0) * a.kv_rs;
    const float* const key_mask = a.key_mask ? a.key_mask + (long)b0 * a.mask_rs : nullptr;
    const int j0 = sp * ck, j1 = min(Sk, j0 + ck);
    const size_t rec_off = ((size_t)h * nrec + sp) * (HD + 4);
    if (j0 >= Sk) {                                              // no key in this split: a record of weight zero per live row
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            if (!lv[r]) continue;
            float* rec = a.part + (long)rowb[r] * a.part_rs + rec_off;
            if (t == 0) { rec[0] = -INFINITY; rec[1] = 0.f; }
            if (t < HD) rec[4 + t] = 0.f;
        }
        return;
    }
    const int sub = lane % CPR, grp = lane / CPR;
    const int jfirst = j0 + wave * KPW;
    uint4 kpre[UR], vpre[UR];                                    // the first block of the split, requested before anything else
#pragma unroll
    for (int r = 0; r < UR; ++r) {
        const int j = jfirst + r * STEP + grp;
        kpre[r] = uint4{0u, 0u, 0u, 0u}; vpre[r] = uint4{0u, 0u, 0u, 0u};
        if (j < j1) {
            kpre[r] = *reinterpret_cast<const uint4*>(kc + (long)j * a.kv_ss + h * HD + sub * 8);
            vpre[r] = *reinterpret_cast<const uint4*>(vc + (long)j * a.kv_ss + h * HD + sub * 8);
        }
    }
    // LN1 of the tile's rows: wave w takes rows w, w + 4, ..; both half-waves compute the row (as every half-wave of the per-row form does)
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (!lv[r] || (r & 3) != wave) continue;                 // wave-uniform
        const int b = rowb[r];
        const bf16_t* resb = a.res + (long)b * d;
        const bf16_t* addb = a.add + (long)b * d;
        float xf[NC][8];
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
        const bool store_ln = h == 0 && sp == 0 && half == 0;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int e0 = (l32 + 32 * c) * 8;
            const f32x4 g0 = *reinterpret_cast<const f32x4*>(a.gamma + e0), g1 = *reinterpret_cast<const f32x4*>(a.gamma + e0 + 4);
            const f32x4 b0v = *reinterpret_cast<const f32x4*>(a.beta + e0), b1v = *reinterpret_cast<const f32x4*>(a.beta + e0 + 4);
            bf16x8 xo;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                xo[j] = (bf16_t)((xf[c][j] - mean) * rstd * (j < 4 ? g0[j & 3] : g1[j & 3]) + (j < 4 ? b0v[j & 3] : b1v[j & 3]));
            if (half == 0) *reinterpret_cast<bf16x8*>(xs + (size_t)r * d + e0) = xo;
            if (store_ln) *reinterpret_cast<bf16x8*>(a.ln_out + (long)b * d + e0) = xo;
        }
    }
    __syncthreads();
    // q_h of every live row: each pass batch of W_q rows is loaded once and applied to the rows in turn
#pragma unroll 1
    for (int pb = 0; pb < NP; pb += PBATCH) {
        bf16x8 w[PBATCH][NC];
        float bv[PBATCH];
#pragma unroll
        for (int p = 0; p < PBATCH; ++p) {
            const int row = h * HD + wave * RPW + 2 * (pb + p) + half;
            bv[p] = a.bq[row];
#pragma unroll
            for (int c = 0; c < NC; ++c) w[p][c] = *reinterpret_cast<const bf16x8*>(a.Wq + (size_t)row * d + (l32 + 32 * c) * 8);
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            if (!lv[r]) continue;
            float xf[NC][8];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const bf16x8 xv = *reinterpret_cast<const bf16x8*>(xs + (size_t)r * d + (l32 + 32 * c) * 8);
#pragma unroll
                for (int j = 0; j < 8; ++j) xf[c][j] = (float)xv[j];
            }
#pragma unroll
            for (int p = 0; p < PBATCH; ++p) {
                float acc = 0.f;
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc = fmaf((float)w[p][c][j], xf[c][j], acc);
                acc = half_sum(acc);
                if (l32 == 0) qs[r * HD + wave * RPW + 2 * (pb + p) + half] = (float)(bf16_t)(acc + bv[p]) * a.scale;
            }
        }
    }
    __syncthreads();
    // scores: every K chunk of the split is loaded once and meets the q of each live row
    float mx[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) mx[r] = -INFINITY;
    for (int jb = jfirst; jb < j1; jb += UR * STEP) {
        uint4 kraw[UR];
        bool vis[UR];
#pragma unroll
        for (int u = 0; u < UR; ++u) {
            const int j = jb + u * STEP + grp;
            kraw[u] = kpre[u];
            if (jb != jfirst) {
                kraw[u] = uint4{0u, 0u, 0u, 0u};
                if (j < j1) kraw[u] = *reinterpret_cast<const uint4*>(kc + (long)j * a.kv_ss + h * HD + sub * 8);
            }
            vis[u] = j < j1 && (!key_mask || key_mask[j] != 0.f);
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            if (!lv[r]) continue;
            float qv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) qv[e] = qs[r * HD + sub * 8 + e];
#pragma unroll
            for (int u = 0; u < UR; ++u) {
                const int j = jb + u * STEP + grp;
                float s = 0.f;
                if (j < j1) {
                    const bf16_t* kv = reinterpret_cast<const bf16_t*>(&kraw[u]);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s = fmaf((float)kv[e], qv[e], s);
                }
#pragma unroll
                for (int o = 1; o < CPR; o <<= 1) s += __shfl_xor(s, o, 64);
                if (j < j1) {
                    const float sv = vis[u] ? s : -INFINITY;
                    if (sub == 0) sc[r * ckp + j - j0] = sv;
                    mx[r] = fmaxf(mx[r], sv);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (!lv[r]) continue;
        mx[r] = wave_max(mx[r]);
        if (lane == 0) red[r * 4 * HD + wave] = mx[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (!lv[r]) continue;
        const float* rd = red + r * 4 * HD;
        mx[r] = fmaxf(fmaxf(rd[0], rd[1]), fmaxf(rd[2], rd[3]));
    }
    __syncthreads();
    float sum[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        sum[r] = 0.f;
        if (!lv[r]) continue;
        float sm = 0.f;
        if (mx[r] != -INFINITY)
            for (int j = t; j < j1 - j0; j += 256) { const float e = __expf(sc[r * ckp + j] - mx[r]); sc[r * ckp + j] = e; sm += e; }
        sm = wave_sum(sm);
        if (lane == 0) red[r * 4 * HD + wave] = sm;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (!lv[r]) continue;
        const float* rd = red + r * 4 * HD;
        sum[r] = (rd[0] + rd[1]) + (rd[2] + rd[3]);
    }
    __syncthreads();
    // o = sum_j p_j V[j]: every V chunk loaded once, one accumulator set per row
    float acc[RT][8];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[r][e] = 0.f;
    for (int jb = jfirst; jb < j1; jb += UR * STEP) {
        uint4 vraw[UR];
#pragma unroll
        for (int u = 0; u < UR; ++u) {
            const int j = jb + u * STEP + grp;
            vraw[u] = vpre[u];
            if (jb != jfirst) {
                vraw[u] = uint4{0u, 0u, 0u, 0u};
                if (j < j1) vraw[u] = *reinterpret_cast<const uint4*>(vc + (long)j * a.kv_ss + h * HD + sub * 8);
            }
        }
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            if (!lv[r] || mx[r] == -INFINITY) continue;
#pragma unroll
            for (int u = 0; u < UR; ++u) {
                const int j = jb + u * STEP + grp;
                if (j < j1) {
                    const bf16_t* vv = reinterpret_cast<const bf16_t*>(&vraw[u]);
                    const float pj = sc[r * ckp + j - j0];
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[r][e] = fmaf(pj, (float)vv[e], acc[r][e]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (!lv[r]) continue;
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int o = CPR; o < 64; o <<= 1) acc[r][e] += __shfl_xor(acc[r][e], o, 64);
        if (grp == 0)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[r * 4 * HD + wave * HD + sub * 8 + e] = acc[r][e];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        if (!lv[r]) continue;
        const float* rd = red + r * 4 * HD;
        float* rec = a.part + (long)rowb[r] * a.part_rs + rec_off;
        if (t == 0) { rec[0] = mx[r]; rec[1] = sum[r]; }
        if (t < HD) rec[4 + t] = (rd[t] + rd[HD + t]) + (rd[2 * HD + t] + rd[3 * HD + t]);
    }
}

// token embedding + learned position + LayerNorm of ONE decoder token per row at the position kept in device memory: i = ++pos[b]
// (PianoBart.py:60-71 through the projected table, modeling_bart.py positions offset 2; same sums as embed_ln_fwd_kernel)
struct SegOff9 { int off[9]; };
template <bool ROWS>
__global__ __launch_bounds__(256) void dec_embed_kernel(const int16_t* __restrict__ tok16, const float* __restrict__ P, const SegOff9 so,
                                                        const float* __restrict__ lin_b, const float* __restrict__ pos_tab,
                                                        const float* __restrict__ w, const float* __restrict__ bb, bf16_t* __restrict__ y,
                                                        BState* __restrict__ st, int d, float eps) {
    __shared__ float red1[4];
    const int b = ROWS ? (int)blockIdx.x : 0;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, d4 = d >> 2;
    if (ROWS && st->done[b]) return;                             // block-uniform
    const int i = st->pos[b] + 1;
    if (ROWS && i >= st->limit[b]) {                             // the row's last position is decoded: it stops here (no row past limit - 1 <= S - 1)
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
    if (t == 0) st->pos[b] = i;                                  // every thread has read pos[b] (two barriers ago); later launches see i
}

// ---------------------------------------------------------------- device-side nucleus sampling (round 6), one workgroup per row
// model.py:68-107 for the 8 heads of ONE position, on the device: logits row -> y = logit / T[h] -> softmax -> nucleus(p[h]) with
// the uniform draw u[pos][h] the host drew AHEAD for this position (the draws do not depend on the logits, model.py:97 /
// np.random.choice) -> the 8 ids of the next decoder input, written to tok_dev for the next step's embedding kernel, and -- with the
// raw logits row -- to pinned host logs indexed by position. The arithmetic follows pb_nucleus_rows above step for step (probs /= (sum +
// 1e-5), descending order with ties by index, candidates up to the first cumsum > p, q = cand / sum(cand), f64 cdf / cdf[-1] > u) with
// wave-parallel prefix sums in place of numpy's left-to-right ones (33.6 -> 19.3 us per token under the profiler); it cannot reproduce the host path bit
// for bit anyway (torch's vectorised CPU exp and its summation order are 1 ulp apart), so the HOST remains the authority: it replays every position
// from the logged logits row with the reference code path and rolls the row back on the (rare) position where the device chose
// differently (Engine._decode_device_sampled). The device result is a PREDICTION that lets the next token start without a host round trip.
// One workgroup of 512 threads: wave h = head h for the softmax and the scans; the rank counting of the heads with p < 1 uses one
// thread per (head, class). fault_period > 0 (tests only) corrupts head 0's id of row fault_row (the single row: row 0) at every
// fault_period-th position. Row form: a special id (>= pad[h] for any head) marks the row done.
// FORCED (pb_batch_decoder_force): a (B, S, 8) table of given ids, -1 = free. The given heads of a position overwrite the sampled ones
// in the last stage, in front of the fault injection and the done test, so the arithmetic of a free head is the unforced kernel's; a
// position with all 8 heads given writes its ids and returns (no logits log: the host does not read that row). The FORCED = false
// instantiations are the kernels and kernarg layouts of a decoder without a table.
// Stop at a bar (pb_batch_decoder_stop), row form: head 0's done test compares against stop[b] of BState in place of pad[0]; stop[b] <=
// pad[0], so the one comparison covers the special ids and the bar. It is no template parameter and no kernarg form of its own: one 4-byte
// load, from the struct done[b] and pos[b] are read from and issued with them, in 1 of the step's launches does not justify doubling the
// instantiations. The ROWS = false kernels have no done flag and are untouched: the host ends a B = 1 run, as it does for EOS.
// Time-ordered sampling (pb_batch_decoder_order), both forms: a row with order[b] >= 0 never samples a (bar, position) below its decoder
// input's -- heads 0 and 1 get -inf quotients for the classes that would go back (the rule: the header), in front of the softmax, and
// everything behind it is the unordered arithmetic. It is a block-uniform branch on order[b], not a template parameter: the row form
// mixes ordered and free rows in one launch (one workgroup per row), so a template would still need the per-row test, and four
// more instantiations would double the captured graphs' variants for code that an unordered row skips with one load and one compare.
// Allowed classes (pb_batch_decoder_allow), both forms and both widths: a row with allow[b] >= 0 carries one bit per vocabulary column; a
// class whose bit is 0 gets the quotient -inf in the expression that forms y, beside the bar floor, so the softmax, the ranking, the
// nucleus rule, the arg-max of a p = 1 head and head 1's second pass (which reuses y) never see it. The logged logits stay the raw ones:
// the host masks its own copy. The bit of class c of head h is bit off[h] + c of the row's mask -- the heads' offsets are no multiples
// of 32, so the word is indexed by column. Block-uniform on the row's index and no template parameter, for order[b]'s reasons: a free
// row pays one compare and 4 more bytes in the load that brings its bar floor, a masked row K loads of words its wave shares.
// Bar schedules (pb_batch_decoder_schedule), both forms and both widths: a row with rule[b].sched >= 0 takes the mask of heads 1 .. 7
// from the bar of the token it is sampling, b0 = head 0's id after forcing -- which exists only behind the barrier that publishes
// htok[0]. Waves 1 .. 7 therefore sample under a GUESS first: the entry of the decoder input's bar (tok_dev[b * 8], which the ordered path
// reads too; entry 0 where that bar is special, the SOS row). Behind the barrier the entry of b0 is read (b0 special: the guess stands,
// the row ends); if it names another mask, waves 1 .. 7 run the three stages again with it and the draws they had -- the quotients
// re-formed from the logits row, which this kernel never writes (the rank counting in between takes all 512 threads, as in the first pass). The result does not depend on the guess; the guess makes the second pass
// rare (the first token of a bar whose mask differs from the previous bar's). Wave 0 keeps the row's own mask: the schedule never
// touches head 0. The schedule pass needs b0 != the input's bar (equal bars have equal entries), head 1's time-ordered pass needs b0 ==
// it, and with a special input bar (the only case where the guess is not the input bar's entry) low1 is 0: a position pays at most ONE
// second pass. Block-uniform like the other rules (BState, tok_dev, the force table, htok[0] behind a barrier): a row without a schedule
// pays one compare and 8 more bytes in the rule load.
// Anchored notes (pb_batch_decoder_anchor), both forms and both widths, the instantiations WITHOUT the force table: a row with
// rule[b].reserved >= 0 carries a list of complete tokens A[0 .. n) in (bar, position) order and a counter k of those written. The
// position is sampled as ever -- the candidate c -- and the last stage decides: if k < n and (c ends the row, or c's (bar, position) >=
// A[k]'s) the 8 ids written are A[k], k becomes k + 1 and the row lives; else c is written and the done test is the one it was. The
// counter and A[k] (one 16-byte row) are requested at the top of the kernel beside done[b] / pos[b]; the comparison sits behind the last
// barrier, where htok[0] and htok[1] are final, in the 8 threads that write, each of which forms the whole decision from htok (LDS) and
// block-uniform values -- no barrier is added. k is device state the SAMPLER advances: a rewind sets it (pb_batch_decoder_seek_anchor).
// A row without anchors pays one compare on the slot of the rule load that was padding.
struct SampleCommon {
    const float* logits;                  // (B, vocab) f32 rows of the positions just decoded
    const double* u;                      // (B, S, 8) uniform draws, device
    BState* st;                           // the positions the rows belong to
    int16_t* tok_dev;                     // (B, 8) next decoder inputs
    float* log_logits;                    // pinned host (B, S, vocab)
    int16_t* log_tok;                     // pinned host (B, S, 8)
};
template <bool ROWS> struct SampleArgs;   // each form's member order is its kernarg layout
template <> struct SampleArgs<false> : SampleCommon {
    int vocab, fault_period;
    int off[8], n[8];
    float temp[8], p[8];
    static constexpr int S = 0, fault_row = 0;
};
template <> struct SampleArgs<true> : SampleCommon {
    int vocab, S, fault_row, fault_period;   // S: the rows' stride in u and the logs
    int off[8], n[8], pad[8];             // pad: the first special id of each head
    float temp[8], p[8];
};
template <bool ROWS> struct ForcedSampleArgs : SampleArgs<ROWS> {
    const int16_t* force;                 // (B, S, 8) given ids of every position, -1 = free, device
};
template <bool ROWS, bool FORCED> struct SampleKernArgs { using type = SampleArgs<ROWS>; };
template <bool ROWS> struct SampleKernArgs<ROWS, true> { using type = ForcedSampleArgs<ROWS>; };
// Two forms of the sampler, chosen by sampler_init from the decoder's heads (wide: a head over SMP_W classes, or more than 512 classes under the
// heads with p < 1, which the narrow form ranks with one thread each): the narrow one (K = SMP_K = 5 classes per lane, rows of
// SMP_W = 272 floats in static LDS; the default dictionary's heads are <= 262) and the wide one (K = SMP_KW = 17, rows of 64 * 17 = 1088, the
// three arrays in ~104 KB of dynamic LDS). Same steps in the same order; K is a template parameter so that the narrow form keeps its
// registers and its LDS.
constexpr int SMP_K = 5, SMP_W = 272;     // narrow: SMP_W >= the largest head, a multiple of 16 (the rank loop's f32x4 reads)
constexpr int SMP_KW = 17;                // wide: heads up to 64 * SMP_KW classes (ops.Layout's limit)
template <int K> struct SmpForm { static constexpr int W = 64 * K; };
template <> struct SmpForm<SMP_K> { static constexpr int W = SMP_W; };
constexpr size_t smp_lds_bytes(int K) { return K == SMP_K ? 0 : sizeof(float) * 8 * (size_t)(64 * K) * 2 + sizeof(float) * 8 * 64 + sizeof(int) * 8 * (size_t)(64 * K); }
// inclusive prefix sums over a wave (lane order), by shuffles
__device__ __forceinline__ float wave_scan_f(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const float u = __shfl_up(v, o, 64); if (lane >= o) v += u; }
    return v;
}
// The three stages of one head, each run by the head's wave (the rank counting of the first pass: by one thread per class). They are
// functions because the time-ordered form runs them a second time for head 1 (below); inlined, the first pass is the code it was.
// softmax(y) of the head's n classes (lane l holds classes l, l + 64, ..; -inf = no such class or a masked one) -> pnh[0 .. SMP_W): torch.softmax(logit / t,
// dim=-1) (model.py:103-104), then probs /= (sum(probs) + 1e-5) (model.py:85). The sums here are wave reductions, not numpy's left-to-right
// ones: a common divisor that differs in its last bit moves every probability alike, so the order and (but for a 1e-7 neighbourhood of a
// threshold) the choice stay -- the host checks every position.
template <int K>
__device__ __forceinline__ void smp_softmax(const float (&y)[K], int n, int lane, float* __restrict__ pnh) {
    constexpr int W = SmpForm<K>::W;
    float e[K];
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, y[k]);
    mx = wave_max(mx);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { e[k] = (lane + 64 * k < n) ? expf(y[k] - mx) : 0.f; s += e[k]; }
    s = wave_sum(s);
    // probs = e / s, then probs /= (sum(probs) + 1e-5) with sum(probs) = 1 to rounding: one division by s (1 + 1e-5). A common factor a few ulps off
    // numpy's moves every probability alike (same order, same candidates but for a 1e-6 neighbourhood of the threshold): the host checks.
    const float inv = 1.0f / (s * 1.00001f);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = lane + 64 * k;
        if (c < W) pnh[c] = c < n ? e[k] * inv : -1.f;       // -1 behind the head's classes: never ranked in front of a class
    }
}
// class c's place in the descending order of pnh (ties by class index) -> sph / sih
template <int W>
__device__ __forceinline__ void smp_rank(const float* __restrict__ pnh, int c, float* __restrict__ sph, int* __restrict__ sih) {
    const float v = pnh[c];
    int rank = 0;
#pragma unroll 17                                                  // fixed trip count (the tail holds -1: never in front of a class), four independent LDS reads in flight
    for (int j4 = 0; j4 < W / 4; ++j4) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(&pnh[4 * j4]);
#pragma unroll
        for (int r = 0; r < 4; ++r) rank += (w[r] > v || (w[r] == v && 4 * j4 + r < c)) ? 1 : 0;
    }
    sph[rank] = v; sih[rank] = c;
}
// nucleus(ph) of the head with the draw u_draw; the id in every lane. ph is wave-uniform; no barrier inside
template <int K>
__device__ __forceinline__ int smp_pick(float ph, int n, int lane, double u_draw, const float* __restrict__ pnh, const float* __restrict__ sph,
                                        const int* __restrict__ sih) {
    if (ph < 1.0f) {
        // lane l owns sorted entries K l .. K l + K - 1 (0 behind the head's classes): prefix sums in sorted order
        float v5[K], pre[K];
        float run = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) { const int i = K * lane + k; v5[k] = i < n ? sph[i] : 0.f; run += v5[k]; pre[k] = run; }
        const float base = wave_scan_f(run, lane) - run;
        int first = 0x7fffffff;                                  // candidates: up to and including the first cumsum > p; none -> top 1
#pragma unroll
        for (int k = K - 1; k >= 0; --k) if (K * lane + k < n && base + pre[k] > ph) first = K * lane + k;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
        const int kc = first == 0x7fffffff ? 1 : first + 1;
        // q = cand / sum(cand), cdf = cumsum(q) / cdf[-1] > u  <=>  prefix_i > u * prefix_{kc - 1}: the prefix sums of the threshold test serve again
        // (numpy renormalises in f32 and accumulates the cdf in f64: a relative 1e-7 against a uniform u)
        float myqs = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) if (K * lane + k == kc - 1) myqs = base + pre[k];
        const float qs = wave_sum(myqs);                         // exactly one lane holds a non-zero term
        const float thr = (float)(u_draw * (double)qs);
        int best = kc - 1;                                       // first candidate whose running sum exceeds u times the candidates' total
#pragma unroll
        for (int k = K - 1; k >= 0; --k) if (K * lane + k < kc && base + pre[k] > thr) best = K * lane + k;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
        return sih[best];
    }
    // p = 1: the cumsum never exceeds it -> the largest probability (lowest class among equals)
    float bv = -1.f; int bi = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = lane + 64 * k;
        if (c < n) { const float v = pnh[c]; if (v > bv) { bv = v; bi = c; } }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    return bi;
}
template <bool ROWS, bool FORCED, int K = SMP_K>
__global__ __launch_bounds__(512) void dec_sample_kernel(const typename SampleKernArgs<ROWS, FORCED>::type a) {
    constexpr int W = SmpForm<K>::W;
    constexpr bool WIDE = K != SMP_K;     // the wide form's three arrays are dynamic LDS (smp_lds_bytes, over the 64 KB a kernel has without the opt-in)
    __shared__ __attribute__((aligned(16))) float pn_s[WIDE ? 1 : 8][WIDE ? 4 : W];   // normalised probabilities, class order
    __shared__ float sp_s[WIDE ? 1 : 8][WIDE ? 1 : W + 64];                            // ... in descending order (heads with p < 1), zero tail
    __shared__ int si_s[WIDE ? 1 : 8][WIDE ? 1 : W];                                   // class of each sorted entry
    extern __shared__ __attribute__((aligned(16))) char smp_dyn[];
    float (*pn)[W] = reinterpret_cast<float (*)[W]>(WIDE ? (void*)smp_dyn : (void*)pn_s);
    float (*sp)[W + 64] = reinterpret_cast<float (*)[W + 64]>(WIDE ? (void*)(smp_dyn + sizeof(float) * 8 * W) : (void*)sp_s);
    int (*si)[W] = reinterpret_cast<int (*)[W]>(WIDE ? (void*)(smp_dyn + sizeof(float) * 8 * (2 * W + 64)) : (void*)si_s);
    __shared__ int htok[8];
    const int b = ROWS ? (int)blockIdx.x : 0;
    if (ROWS && a.st->done[b]) return;                           // block-uniform
    const int t = threadIdx.x, lane = t & 63, h = t >> 6;
    const int pos = a.st->pos[b];
    [[maybe_unused]] int stop0 = 0;                              // head 0's first id that ends the row: requested with done[b] and pos[b]
    if constexpr (ROWS) stop0 = a.st->stop[b];
    // time-ordered row (order[b] >= 0, block-uniform): low0 = the first bar head 0 may sample; low1 > 0 = the first position head 1 may
    // sample IF the token's bar stays prev0 (0: head 1 is free whatever the bar). prev = the row's decoder input, read here, in front of
    // the first barrier; the last stage overwrites it behind the last one.
    const BState::RowRule rule = a.st->rule[b];                  // one 16-byte load: the bar floor, the allow mask and the bar schedule (below) of the row
    const int ord = rule.order, alw = rule.allow, sch = rule.sched;
    // anchored row (rule[b].reserved >= 0, block-uniform; never with the force table): the counter, the count and the anchor the counter
    // names are requested here; the last stage compares and writes. ak == an: every anchor is placed and the row samples on (the row
    // read is then the last one, unused). A row's count is >= 1 wherever its base is >= 0 (pb_batch_decoder_anchor stores -1 for 0).
    [[maybe_unused]] const int anc = rule.reserved;
    [[maybe_unused]] int ak = 0, an = 0, astop = stop0;
    [[maybe_unused]] uint4 arow = {0u, 0u, 0u, 0u};
    if constexpr (!FORCED) {
        if (anc >= 0) {
            ak = a.st->aplaced[b]; an = a.st->acnt[b];
            if constexpr (!ROWS) astop = a.st->stop[b];          // the single-row form has no done test of its own: the anchor rule needs the bar
            arow = *reinterpret_cast<const uint4*>(a.st->atab + (size_t)(anc + max(min(ak, an - 1), 0)) * 8);     // 16 bytes, 16-byte aligned
        }
    }
    int low0 = 0, low1 = 0, prev0 = -1;
    if (ord >= 0) {
        const int p0 = a.tok_dev[b * 8 + 0], p1 = a.tok_dev[b * 8 + 1];
        const bool bar = p0 < a.st->opad[0];                     // an ordinary event: not the SOS row
        low0 = max(ord, bar ? p0 : 0);
        if (bar && p1 < a.st->opad[1]) { low1 = p1; prev0 = p0; }
    }
    // bar schedule (rule[b].sched >= 0, block-uniform): guess = the mask of the decoder input's bar, for waves 1 .. 7. An entry of -1
    // means the row's own mask, so what is compared behind the barrier is the index the waves actually used. The row's entries are
    // stab[sch * nbar .. + nbar - 1]; nbar = pad[0] and the bar indexed is < opad[0] = pad[0] (checked by pb_batch_decoder_schedule).
    const int* srow = a.st->stab + (size_t)max(sch, 0) * a.st->nbar;     // formed for every row, read by a scheduled one (amask's remark, below)
    int guess = alw;
    if (sch >= 0) {
        const int p0 = a.tok_dev[b * 8 + 0];
        const int g = srow[(unsigned)p0 < (unsigned)a.st->opad[0] ? p0 : 0];
        if (g >= 0) guess = g;
    }
    // allowed classes (rule[b].allow >= 0, block-uniform): the row's mask, one bit per vocabulary column
    // The address is formed whether the row has a mask or not (index 0 for a free row; never read then): with a branch of its own here
    // the compiler requests pos[b] a scalar-load round trip later than it did, which every free row would pay (1 us per launch, measured).
    const int mine = h == 0 ? alw : guess;                       // wave-uniform: head 0 never sees the schedule
    const bool masked = mine >= 0;
    const uint32_t* amask = a.st->amask + (size_t)max(mine, 0) * a.st->awords;
    const float* logits = a.logits + (size_t)b * a.vocab;
    float* log_logits = a.log_logits + ((size_t)b * a.S + pos) * a.vocab;
    const int n = a.n[h], off = a.off[h];
    const float T = a.temp[h];
    const double u_draw = a.u[((size_t)b * a.S + pos) * 8 + h];  // requested now: a load that depends on pos would otherwise sit at the end of the chain
    [[maybe_unused]] int f = -1;                                 // the given id of head t & 7 at this position
    [[maybe_unused]] int f0 = -1, f1 = -1;                       // ... of heads 0 and 1, in every thread
    if constexpr (FORCED) {
        const int16_t* fr = a.force + ((size_t)b * a.S + pos) * 8;
        const uint4 all = *reinterpret_cast<const uint4*>(fr);   // the 8 entries of the position: 16 bytes, 16-byte aligned
        f = fr[t & 7];
        f0 = (int16_t)(all.x & 0xffffu); f1 = (int16_t)(all.x >> 16);
        if ((((all.x | all.y) | (all.z | all.w)) & 0x80008000u) == 0) {     // all 8 heads given (block-uniform): nothing to sample
            if constexpr (ROWS) __syncthreads();                 // every thread has read done[b] before it may change
            if (t < 8) {
                a.tok_dev[b * 8 + t] = (int16_t)f;
                a.log_tok[((size_t)b * a.S + pos) * 8 + t] = (int16_t)f;
                if constexpr (ROWS) { if (f >= (t == 0 ? stop0 : a.pad[t])) a.st->done[b] = 1; }
            }
            return;
        }
    }
    // y = logit / T of head h's classes; a time-ordered row's bars below low0 get -inf here, so their probability is an exact 0: the
    // rank count puts them behind every positive class and the p = 1 arg-max never picks one (the largest class has e = 1). The classes
    // a row's allow mask removes get -inf the same way (column off + c <= vocab - 1: inside the mask's ceil(vocab / 32) words).
    float y[K];
    const int lowh = h == 0 ? low0 : 0;                          // wave-uniform
    // bit k of `allowed` = the lane's class k may be sampled. A masked row reads its K bits here, behind one block-uniform branch and in
    // front of the loop, so that the loop below keeps the free row's shape: its K logits loads in flight together, no branch per class.
    unsigned allowed = ~0u;
    if (masked) {
        allowed = 0u;
#pragma unroll
        for (int k = 0; k < K; ++k) {                            // every lane reads a word of the mask (the column clamped into it; `in` below decides): K loads in flight
            const int col = min(off + lane + 64 * k, a.vocab - 1);
            allowed |= ((amask[col >> 5] >> (col & 31)) & 1u) << k;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = lane + 64 * k;
        const bool in = c < n;
        const float lg = in ? logits[off + c] : 0.f;
        if (in) ROWS ? log_logits[off + c] = lg : a.log_logits[(size_t)pos * a.vocab + off + c] = lg;
        y[k] = (in && c >= lowh && ((allowed >> k) & 1u)) ? lg / T : -INFINITY;
    }
    smp_softmax(y, n, lane, pn[h]);
    __syncthreads();
    // descending order of the heads with p < 1 by rank counting, one thread per (head, class): ties by class index
    {
        // narrow: at most 512 such classes (sampler_init), one round; wide: rounds of 512 until every class of those heads had its thread
        int tot = 0;                                             // wide only: the classes under heads with p < 1 (block-uniform)
        if constexpr (WIDE) { for (int q = 0; q < 8; ++q) tot += a.p[q] < 1.0f ? a.n[q] : 0; }
        for (int c0 = t; WIDE ? c0 < tot : c0 == t; c0 += 512) {
            int hh = -1, c = c0;
            for (int q = 0; q < 8; ++q) {
                if (a.p[q] < 1.0f) {
                    if (hh < 0 && c < a.n[q]) hh = q;
                    if (hh < 0) c -= a.n[q];
                }
            }
            if (hh >= 0) smp_rank<W>(pn[hh], c, sp[hh], si[hh]);
        }
        if (t < 8 * 64) sp[t >> 6][W + (t & 63)] = 0.f;
    }
    __syncthreads();
    const float ph = a.p[h];
    {                                                            // wave h = head h; no barrier inside
        const int id = smp_pick<K>(ph, n, lane, u_draw, pn[h], sp[h], si[h]);
        if (lane == 0) htok[h] = id;
    }
    __syncthreads();
    // Bar schedule: the mask of heads 1 .. 7 is that of bar b0, head 0's id AFTER forcing. Where it is not the guessed one, waves 1 .. 7
    // sample again (the kernel's comment); every condition is block-uniform, so the barriers below are reached by all 512 threads or by
    // none. The quotients come from the logits row again (the first pass left -inf where its mask bit); no bar floor: that is head 0's.
    // Head 1's time-ordered pass below then starts from these quotients, and cannot follow a pass taken here (b0 == prev0 there).
    if (sch >= 0) {
        int b0 = htok[0];
        if constexpr (FORCED) { if (f0 >= 0) b0 = f0; }
        int want = guess;
        if ((unsigned)b0 < (unsigned)a.st->opad[0]) { const int s = srow[b0]; want = s >= 0 ? s : alw; }
        if (want != guess) {
            if (h != 0) {
                unsigned allowed = ~0u;
                if (want >= 0) {
                    const uint32_t* wmask = a.st->amask + (size_t)want * a.st->awords;
                    allowed = 0u;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int col = min(off + lane + 64 * k, a.vocab - 1);
                        allowed |= ((wmask[col >> 5] >> (col & 31)) & 1u) << k;
                    }
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int c = lane + 64 * k;
                    const bool in = c < n;
                    const float lg = in ? logits[off + c] : 0.f;
                    y[k] = (in && ((allowed >> k) & 1u)) ? lg / T : -INFINITY;
                }
                smp_softmax(y, n, lane, pn[h]);
            }
            __syncthreads();
            {
                // the first pass's rank counting again, one thread per (head, class) over all 512 threads: a wave that ranked its own head
                // class by class took 4x the whole first pass (measured). Head 0's probabilities did not change: its classes keep their
                // thread and write nothing.
                int tot = 0;
                if constexpr (WIDE) { for (int q = 0; q < 8; ++q) tot += a.p[q] < 1.0f ? a.n[q] : 0; }
                for (int c0 = t; WIDE ? c0 < tot : c0 == t; c0 += 512) {
                    int hh = -1, c = c0;
                    for (int q = 0; q < 8; ++q) {
                        if (a.p[q] < 1.0f) {
                            if (hh < 0 && c < a.n[q]) hh = q;
                            if (hh < 0) c -= a.n[q];
                        }
                    }
                    if (hh >= 1) smp_rank<W>(pn[hh], c, sp[hh], si[hh]);
                }
            }
            __syncthreads();
            if (h != 0) {
                const int id = smp_pick<K>(ph, n, lane, u_draw, pn[h], sp[h], si[h]);
                if (lane == 0) htok[h] = id;
            }
            __syncthreads();
        }
    }
    // Time-ordered row, head 1: its mask depends on head 0's id AFTER forcing (b0 == prev0: the token stays in the bar of its
    // predecessor), which exists only now. Wave 1 therefore samples a second time behind the barrier that published htok[0]. The other
    // way -- both variants in the first pass, one selected here -- would give the masked variant a ninth wave or a second round of wave 1 at
    // EVERY position of every ordered row, and rows of pn / sp / si of its own; the second pass is paid only where the mask bites
    // (same bar, predecessor's position > 0, head 1 not given), runs 134 classes on one wave, and leaves the first pass -- all an
    // unordered row executes -- as it was. Every condition is block-uniform (BState, tok_dev, the force table, htok[0] behind a barrier),
    // so the barriers below are reached by all 512 threads or by none. Same draw u[1]: the draws do not move.
    if (low1 > 0) {
        int b0 = htok[0];
        if constexpr (FORCED) { if (f0 >= 0) b0 = f0; }
        if (b0 == prev0 && f1 < 0) {
            const bool sorted1 = a.p[1] < 1.0f;
            if (h == 1) {
#pragma unroll
                for (int k = 0; k < K; ++k) if (lane + 64 * k < low1) y[k] = -INFINITY;
                smp_softmax(y, n, lane, pn[1]);
            }
            __syncthreads();
            if (sorted1) {
                if (h == 1) {
#pragma unroll
                    for (int k = 0; k < K; ++k) { const int c = lane + 64 * k; if (c < n) smp_rank<W>(pn[1], c, sp[1], si[1]); }
                }
                __syncthreads();
            }
            if (h == 1) {
                const int id = smp_pick<K>(ph, n, lane, u_draw, pn[1], sp[1], si[1]);
                if (lane == 0) htok[1] = id;
            }
            __syncthreads();
        }
    }
    if (t < 8) {
        int id = htok[t];
        if constexpr (FORCED) { if (f >= 0) id = f; }
        if (a.fault_period > 0 && (!ROWS || b == a.fault_row) && t == 0 && (pos % a.fault_period) == a.fault_period - 1) id = (id + 1) % a.n[0];
        // Anchored row with an anchor left: each of the 8 writing threads forms the whole decision from the candidate in htok (final: behind
        // the last barrier; head 0 as the fault hook left it) and block-uniform values, so all 8 agree without another barrier. The
        // candidate ends the row (the done test below, over all 8 heads) or its time has reached the anchor's: the anchor is written, all
        // 8 heads as given, the counter advances and the row lives. Thread 0 alone stores the counter, which every thread read at the top.
        [[maybe_unused]] bool placed = false;
        if constexpr (!FORCED) {
            if (anc >= 0 && ak < an) {
                int c0 = htok[0];
                const int c1 = htok[1];
                if (a.fault_period > 0 && (!ROWS || b == a.fault_row) && (pos % a.fault_period) == a.fault_period - 1) c0 = (c0 + 1) % a.n[0];
                bool ends = c0 >= astop;
#pragma unroll
                for (int q = 1; q < 8; ++q) {
                    int padq;
                    if constexpr (ROWS) padq = a.pad[q]; else padq = a.st->apad[q];
                    ends = ends || htok[q] >= padq;
                }
                const int a0 = (int16_t)(arow.x & 0xffffu), a1 = (int16_t)(arow.x >> 16);
                if (ends || c0 > a0 || (c0 == a0 && c1 >= a1)) {
                    const unsigned w = t < 2 ? arow.x : (t < 4 ? arow.y : (t < 6 ? arow.z : arow.w));
                    id = (int16_t)((t & 1) ? (w >> 16) : (w & 0xffffu));
                    placed = true;
                    if (t == 0) a.st->aplaced[b] = ak + 1;
                }
            }
        }
        a.tok_dev[b * 8 + t] = (int16_t)id;
        a.log_tok[((size_t)b * a.S + pos) * 8 + t] = (int16_t)id;
        if constexpr (ROWS) { if (!placed && id >= (t == 0 ? stop0 : a.pad[t])) a.st->done[b] = 1; }    // the device stops the row here; the host confirms or rewinds it
    }
}

// ---------------------------------------------------------------- the rows' cross-attention geometry and the hand-over of a slot
// Both take their values by kernarg, so nothing on the host has to outlive the call and the stores land in stream order.
struct GeomArgs { int s_enc[BMAX], ck[BMAX], kv_row[BMAX]; };
__global__ __launch_bounds__(64) void dec_geom_kernel(BState* __restrict__ st, const GeomArgs g) {
    const int t = threadIdx.x;
    if (t < BMAX) { st->s_enc[t] = g.s_enc[t]; st->ck[t] = g.ck[t]; st->kv_row[t] = g.kv_row[t]; }
}
struct StopArgs { int stop[BMAX]; };
__global__ __launch_bounds__(64) void dec_stop_kernel(BState* __restrict__ st, const StopArgs g) {
    const int t = threadIdx.x;
    if (t < BMAX) st->stop[t] = g.stop[t];
}
struct OrderArgs { int order[BMAX]; };
__global__ __launch_bounds__(64) void dec_order_kernel(BState* __restrict__ st, const OrderArgs g) {
    const int t = threadIdx.x;
    if (t < BMAX) st->rule[t].order = g.order[t];
}
struct AllowArgs { int allow[BMAX]; int words; const uint32_t* table; };
__global__ __launch_bounds__(64) void dec_allow_kernel(BState* __restrict__ st, const AllowArgs g) {
    const int t = threadIdx.x;
    if (t < BMAX) st->rule[t].allow = g.allow[t];
    if (t == 0) { st->awords = g.words; st->amask = g.table; }
}
struct SchedArgs { int sched[BMAX]; int nbar; const int* table; };
__global__ __launch_bounds__(64) void dec_sched_kernel(BState* __restrict__ st, const SchedArgs g) {
    const int t = threadIdx.x;
    if (t < BMAX) st->rule[t].sched = g.sched[t];
    if (t == 0) { st->nbar = g.nbar; st->stab = g.table; }
}
struct AnchorArgs { int base[BMAX], cnt[BMAX]; int pad[8]; const int16_t* table; };
__global__ __launch_bounds__(64) void dec_anchor_kernel(BState* __restrict__ st, const AnchorArgs g) {
    const int t = threadIdx.x;
    if (t < BMAX) { st->rule[t].reserved = g.cnt[t] > 0 ? g.base[t] : -1; st->acnt[t] = g.cnt[t]; st->aplaced[t] = 0; }
    if (t < 8) st->apad[t] = g.pad[t];
    if (t == 0) st->atab = g.table;
}
struct AdmitArgs {
    BState* st; int16_t* tok_dev;
    int row, s_enc, ck, slice, pos, limit;   // row < B <= BMAX (checked by pb_batch_decoder_admit)
    int stop;                                // the new occupant's stop bar (pad[0]: none)
    int order;                               // ... and its bar floor of time-ordered sampling (-1: a free row)
    int allow;                               // ... and the index of its allow mask in the decoder's table (-1: every class allowed)
    int sched;                               // ... and the index of its bar schedule in the decoder's table (-1: none)
    int anchor, n_anchor;                    // ... and its anchors: base in the decoder's table and count (-1, 0: none); the counter starts at 0
    int16_t tok[8];
};
__global__ __launch_bounds__(64) void dec_admit_kernel(const AdmitArgs a) {
    const int t = threadIdx.x, b = a.row;
    if (t < 8) a.tok_dev[b * 8 + t] = a.tok[t];
    if (t == 0) {
        a.st->s_enc[b] = a.s_enc; a.st->ck[b] = a.ck; a.st->kv_row[b] = a.slice;
        a.st->pos[b] = a.pos; a.st->limit[b] = a.limit; a.st->done[b] = 0; a.st->stop[b] = a.stop;
        a.st->rule[b].order = a.order; a.st->rule[b].allow = a.allow; a.st->rule[b].sched = a.sched;
        a.st->rule[b].reserved = a.n_anchor > 0 ? a.anchor : -1; a.st->acnt[b] = a.n_anchor; a.st->aplaced[b] = 0;
    }
}

constexpr int SPEC_K = 8;                  // steps per graph replay of the device-sampled decode
constexpr int N_STAGE = 2 * BMAX;          // pinned staging entries of pb_batch_decoder_admit
constexpr int SPEC_EVENTS = 8;
enum { G_STEP, G_ONE, G_RUN, N_GRAPHS };   // captured graphs: one host-sampled step; 1 and SPEC_K device-sampled steps

struct Decoder {
    pb_decode_batch bp;
    int B = 0;
    hipStream_t stream = nullptr;
    BState* st = nullptr;                  // device
    int16_t* tok_dev = nullptr;            // device (B, 8): the rows' current decoder inputs
    int16_t* tok_host = nullptr;           // pinned (B, 8)
    float* logits_host = nullptr;          // pinned (vocab): the host-sampled step's row
    double* u_dev = nullptr;
    float* log_logits = nullptr;           // pinned (B, S, vocab)
    int16_t* log_tok = nullptr;            // pinned (B, S, 8)
    SampleArgs<true> sa{};                 // the sampler constants (the single-row kernel takes its subset)
    bool sampler = false;
    bool wide = false;                     // sampler_init: a head over SMP_W classes -> the wide sampler (K = SMP_KW, dynamic LDS)
    int16_t* force_dev = nullptr;          // pb_batch_decoder_force: (B, S, 8) given ids, -1 = free; the steps then end with the FORCED sampler
    hipGraph_t graph[N_GRAPHS] = {};
    hipGraphExec_t exec[N_GRAPHS] = {};
    hipEvent_t ev = nullptr;
    hipEvent_t evs[SPEC_EVENTS] = {};
    int next_ev = 0;
    int launches = 0, use_graph = 1, ns_self = PB_DECODE_MAX_SPLITS, ns_cross = PB_DECODE_MAX_SPLITS;   // workgroups per head of the two attention launches
    int ck_cross[BMAX] = {};
    int steps = 0, limit = 0;              // B == 1: positions enqueued since the reset and their bound (the single-row kernels do not check)
    size_t lds_attn = 0;
    // pb_batch_decoder_share_cross: kv_cross is (n_groups, S, 2d) and row b reads slice kv_row[b] (0 groups: (B, S, 2d), row b its own)
    int n_groups = 0, kv_row[BMAX] = {};
    bool issued = false;                   // a step was issued or captured: the cross-cache layout is fixed
    int group_rt = 0;                      // > 0: the grouped cross-attention kernel with this row tile; 0: the per-row kernel through kv_row
    int n_tiles = 0, rows_by_group[BMAX] = {}, tile_first[BMAX] = {}, tile_n[BMAX] = {};
    size_t lds_group = 0;                  // the grouped kernel's LDS: q, reduction, LN1 and score rows of a tile
    // pb_batch_decoder_dynamic: kv_cross is (dynamic, S, 2d) and each row's geometry is read from BState; 0 = not dynamic
    int dynamic = 0;
    GeomArgs geo{};                        // host mirror of the rows' geometry in BState
    bool live[BMAX] = {};                  // the host has started the row and not ended it (pb_batch_decoder_admit refuses a live row)
    StopArgs stop{};                       // host mirror of the rows' stop bars in BState (pb_batch_decoder_start uploads the whole struct)
    int admit_stop[BMAX] = {};             // pb_batch_decoder_admit_stop: the value the row's next admit stores (-1: none staged -> pad[0])
    OrderArgs order{};                     // host mirror of the rows' bar floors in BState (-1: a free row), valid behind sampler_init
    int admit_order[BMAX] = {};            // pb_batch_decoder_admit_order: the value the row's next admit stores (-1: none staged -> a free row)
    AllowArgs allow{};                     // host mirror of the rows' mask indices in BState (-1: every class allowed) and of the table's address
    int admit_allow[BMAX] = {};            // pb_batch_decoder_admit_allow: the index the row's next admit stores (-1: none staged -> a free row)
    uint32_t* allow_dev = nullptr;         // pb_batch_decoder_allow: (n_allow, allow.words) masks, one bit per vocabulary column
    int n_allow = 0;                       // masks in allow_dev; 0 behind sampler_init until pb_batch_decoder_allow
    SchedArgs sched{};                     // host mirror of the rows' schedule indices in BState (-1: no schedule) and of the table's address
    int admit_sched[BMAX] = {};            // pb_batch_decoder_admit_schedule: the index the row's next admit stores (-1: none staged -> no schedule)
    int* sched_dev = nullptr;              // pb_batch_decoder_schedule: (n_sched, sched.nbar) indices into allow_dev's masks, -1 = the row's own mask
    int n_sched = 0;                       // schedules in sched_dev; 0 behind sampler_init until pb_batch_decoder_schedule
    AnchorArgs anchor{};                   // host mirror of the rows' anchor bases and counts in BState (count 0: none) and of the table's address
    int admit_anchor[BMAX] = {}, admit_nanchor[BMAX] = {};     // pb_batch_decoder_admit_anchor: what the row's next admit stores (count 0: none staged -> no anchors)
    int16_t* anchor_dev = nullptr;         // pb_batch_decoder_anchor: (n_anchor, 8) ordinary ids, the anchors of ALL rows of the call
    std::vector<int16_t> anchor_host;      // ... and the host's copy, for pb_batch_decoder_admit_anchor's checks
    int n_anchor = 0;                      // rows in anchor_dev; 0 behind sampler_init until pb_batch_decoder_anchor
    hipEvent_t ev_fence = nullptr;
    char* stage = nullptr;                 // pinned: N_STAGE entries of {u (S, 8) f64 | forced (S, 8) i16 | mask (S) f32}
    size_t stage_bytes = 0;
    hipEvent_t stage_ev[N_STAGE] = {};     // recorded behind the copies out of an entry
    bool stage_used[N_STAGE] = {};
    int next_stage = 0;
};

template <int NC, int HD, bool ROWS>
static void dec_attn_go(const DecAttnArgs<ROWS>& a, bool self, int H, int nrec, int B, size_t lds, hipStream_t st) {
    if (self) hipLaunchKernelGGL((dec_attn_kernel<NC, HD, true, ROWS>), dim3(H, nrec, B), dim3(768), lds, st, a);
    else hipLaunchKernelGGL((dec_attn_kernel<NC, HD, false, ROWS>), dim3(H, nrec, B), dim3(256), lds, st, a);
}
template <bool ROWS>
static int dec_attn_launch(const DecAttnArgs<ROWS>& a, bool self, int H, int hd, int nrec, int B, size_t lds, hipStream_t st) {
    const int nc = a.d / 256;
#define PB_DA(NC_) do { if (hd == 64) dec_attn_go<NC_, 64>(a, self, H, nrec, B, lds, st); else dec_attn_go<NC_, 128>(a, self, H, nrec, B, lds, st); } while (0)
    if (nc == 1) PB_DA(1); else if (nc == 2) PB_DA(2); else if (nc == 3) PB_DA(3); else PB_DA(4);
#undef PB_DA
    PB_LAUNCH_CHECK();
    return 0;
}

template <int NC, int HD>
static void dec_attn_dyn_go(const DecAttnDynArgs& a, int H, int nrec, int B, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL((dec_attn_kernel<NC, HD, false, true, DecAttnDynArgs>), dim3(H, nrec, B), dim3(256), lds, st, a);
}
static int dec_attn_dyn_launch(const DecAttnDynArgs& a, int H, int hd, int nrec, int B, size_t lds, hipStream_t st) {
    const int nc = a.d / 256;
#define PB_DD(NC_) do { if (hd == 64) dec_attn_dyn_go<NC_, 64>(a, H, nrec, B, lds, st); else dec_attn_dyn_go<NC_, 128>(a, H, nrec, B, lds, st); } while (0)
    if (nc == 1) PB_DD(1); else if (nc == 2) PB_DD(2); else if (nc == 3) PB_DD(3); else PB_DD(4);
#undef PB_DD
    PB_LAUNCH_CHECK();
    return 0;
}

template <int NC, int HD>
static void dec_attn_group_go(const DecAttnGroupArgs& a, int rt, int H, int nrec, int ntile, size_t lds, hipStream_t st) {
    if (rt == 2) hipLaunchKernelGGL((dec_attn_group_kernel<NC, HD, 2>), dim3(H, nrec, ntile), dim3(256), lds, st, a);
    else if (rt == 4) hipLaunchKernelGGL((dec_attn_group_kernel<NC, HD, 4>), dim3(H, nrec, ntile), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((dec_attn_group_kernel<NC, HD, 8>), dim3(H, nrec, ntile), dim3(256), lds, st, a);
}
static int dec_attn_group_launch(const DecAttnGroupArgs& a, int rt, int H, int hd, int nrec, int ntile, size_t lds, hipStream_t st) {
    const int nc = a.d / 256;
#define PB_DG(NC_) do { if (hd == 64) dec_attn_group_go<NC_, 64>(a, rt, H, nrec, ntile, lds, st); else dec_attn_group_go<NC_, 128>(a, rt, H, nrec, ntile, lds, st); } while (0)
    if (nc == 1) PB_DG(1); else if (nc == 2) PB_DG(2); else if (nc == 3) PB_DG(3); else PB_DG(4);
#undef PB_DG
    PB_LAUNCH_CHECK();
    return 0;
}

// the launches of one step on D->stream (the single-row instances when ROWS is false, B == 1), the sampler last when `sample`;
// D->launches = their number
template <bool ROWS>
static int step_issue(Decoder* D, bool sample) {
    const pb_decode_plan* p = &D->bp.plan;
    const int d = p->d, H = p->H, hd = d / H, f = p->ffn, B = D->B;
    const float scale = 1.0f / sqrtf((float)hd);
    const long part_rs = (long)H * PB_DECODE_MAX_SPLITS * (hd + 4);
    const LnIn none{nullptr, nullptr, nullptr, nullptr};
    const MergeIn none_mg{nullptr, 0, 0, 0, 0};
    hipStream_t st = D->stream;
    int n = 0;
    SegOff9 so;
    for (int k = 0; k < 9; ++k) so.off[k] = p->tab_off[k];
    hipLaunchKernelGGL(dec_embed_kernel<ROWS>, dim3(B), dim3(256), 0, st, D->tok_dev, p->ptab, so, p->lin_b,
                       p->pos, p->lne_w, p->lne_b, (bf16_t*)p->x, D->st, d, 1e-5f);
    PB_LAUNCH_CHECK(); ++n;
    char* x = (char*)p->x; char* alt = (char*)p->y2;
    char* h = x;
    LnIn ln = none;                                      // pending post-LN of the previous layer, applied by the next attention (or the heads)
    const MergeIn mg_self{p->attn_part, D->ns_self, hd, hd + 4, part_rs}, mg_cross{p->attn_part, D->ns_cross, hd, hd + 4, part_rs};
    DecAttnArgs<ROWS> a{};
    a.d = d; a.scale = scale; a.eps = 1e-5f; a.part = p->attn_part; a.st = D->st; a.kv_ss = 2 * d;
    if constexpr (ROWS) {
        a.kv_rs = (long)p->S * 2 * d; a.mask_rs = p->S; a.part_rs = part_rs;
        for (int b = 0; b < B; ++b) { a.s_enc_[b] = D->bp.s_enc[b]; a.ck_[b] = D->ck_cross[b]; a.kv_row_[b] = D->n_groups ? D->kv_row[b] : b; }
    }
    D->issued = true;
    for (int l = 0; l < p->n_layers; ++l) {
        const pb_decode_layer& L = p->layers[l];
        // self-attention: LN2 of the layer below (or the embedding row), q|k|v of this token, keys 0 .. i
        a.x_in = (const bf16_t*)h; a.res = (const bf16_t*)ln.res; a.add = (const bf16_t*)p->a; a.gamma = ln.gamma; a.beta = ln.beta; a.ln_out = (bf16_t*)ln.out;
        a.Wq = (const bf16_t*)L.wqkv; a.bq = L.bqkv;
        a.Wk = a.Wq + (size_t)d * d; a.bk = L.bqkv + d; a.Wv = a.Wq + (size_t)2 * d * d; a.bv = L.bqkv + 2 * d;
        a.kc = (bf16_t*)L.kv_self; a.vc = a.kc + d; a.key_mask = nullptr; a.nreg = D->ns_self - 1;
        if (dec_attn_launch(a, true, H, hd, D->ns_self, B, D->lds_attn, st)) return -1;
        ++n;
        if (ln.res) h = alt;
        if (gemv_launch(L.wo, nullptr, L.bo, p->a, nullptr, d, d, d, PB_BF16, 0, 0, st, none, mg_self, D->st, B)) return -1;
        ++n;
        // cross-attention: LN1(h + a) -> y1, q_c, the cached encoder keys
        a.x_in = nullptr; a.res = (const bf16_t*)h; a.add = (const bf16_t*)p->a; a.gamma = L.ln1_w; a.beta = L.ln1_b; a.ln_out = (bf16_t*)p->y1;
        a.Wq = (const bf16_t*)L.wq_c; a.bq = L.bq_c; a.Wk = nullptr; a.bk = nullptr; a.Wv = nullptr; a.bv = nullptr;
        a.kc = (bf16_t*)const_cast<void*>(L.kv_cross); a.vc = a.kc + d; a.key_mask = p->enc_mask; a.nreg = D->ns_cross;
        if constexpr (!ROWS) { a.ck_fixed = D->ck_cross[0]; a.Sk_fixed = D->bp.s_enc[0]; }
        bool grouped = false;
        if constexpr (ROWS) {
            if (D->dynamic) {                             // the geometry comes from BState: a slot may change its prompt between replays
                DecAttnDynArgs da{};
                static_cast<DecAttnCommon&>(da) = a;
                da.kv_rs = a.kv_rs; da.key_mask = a.key_mask; da.mask_rs = a.mask_rs; da.st = a.st; da.d = a.d; da.nreg = a.nreg;
                da.scale = a.scale; da.eps = a.eps; da.part = a.part; da.part_rs = a.part_rs;
                if (dec_attn_dyn_launch(da, H, hd, D->ns_cross, B, D->lds_attn, st)) return -1;
                grouped = true;
            } else if (D->group_rt > 0) {                 // rows of one cross K|V slice share a workgroup (same launch count)
                DecAttnGroupArgs ga{};
                static_cast<DecAttnArgs<true>&>(ga) = a;
                for (int b = 0; b < B; ++b) ga.rows_[b] = D->rows_by_group[b];
                for (int k = 0; k < D->n_tiles; ++k) { ga.tile_first[k] = D->tile_first[k]; ga.tile_n[k] = D->tile_n[k]; }
                if (dec_attn_group_launch(ga, D->group_rt, H, hd, D->ns_cross, D->n_tiles, D->lds_group, st)) return -1;
                grouped = true;
            }
        }
        if (!grouped && dec_attn_launch(a, false, H, hd, D->ns_cross, B, D->lds_attn, st)) return -1;
        ++n;
        if (gemv_launch(L.wo_c, nullptr, L.bo_c, p->a, nullptr, d, d, d, PB_BF16, 0, 0, st, none, mg_cross, D->st, B)) return -1;
        ++n;
        // FFN: fc1 applies LNc(y1 + a) -> yc
        if (gemv_launch(L.w1, p->a, L.b1, p->g, nullptr, f, f, d, PB_BF16, 0, 1, st, LnIn{p->y1, L.lnc_w, L.lnc_b, p->yc}, none_mg, D->st, B)) return -1;
        ++n;
        if (gemv_launch(L.w2, p->g, L.b2, p->a, nullptr, d, d, f, PB_BF16, 0, 0, st, none, none_mg, D->st, B)) return -1;
        ++n;
        ln = LnIn{p->yc, L.ln2_w, L.ln2_b, alt};
    }
    if (gemv_launch(p->head_w, p->a, p->head_b, p->logits, nullptr, p->vocab, p->vocab, d, PB_BF16, 1, 0, st, ln, none_mg, D->st, B)) return -1;
    ++n;
    if (sample) {
        if constexpr (ROWS) {
            if (D->force_dev) {
                ForcedSampleArgs<true> sf{};
                static_cast<SampleArgs<true>&>(sf) = D->sa;
                sf.force = D->force_dev;
                if (D->wide) hipLaunchKernelGGL((dec_sample_kernel<true, true, SMP_KW>), dim3(B), dim3(512), smp_lds_bytes(SMP_KW), st, sf);
                else hipLaunchKernelGGL((dec_sample_kernel<true, true>), dim3(B), dim3(512), 0, st, sf);
            } else {
                if (D->wide) hipLaunchKernelGGL((dec_sample_kernel<true, false, SMP_KW>), dim3(B), dim3(512), smp_lds_bytes(SMP_KW), st, D->sa);
                else hipLaunchKernelGGL((dec_sample_kernel<true, false>), dim3(B), dim3(512), 0, st, D->sa);
            }
        } else {
            SampleArgs<false> s1{};
            static_cast<SampleCommon&>(s1) = D->sa;
            s1.vocab = D->sa.vocab; s1.fault_period = D->sa.fault_period;
            for (int k = 0; k < 8; ++k) { s1.off[k] = D->sa.off[k]; s1.n[k] = D->sa.n[k]; s1.temp[k] = D->sa.temp[k]; s1.p[k] = D->sa.p[k]; }
            if (D->force_dev) {
                ForcedSampleArgs<false> sf{};
                static_cast<SampleArgs<false>&>(sf) = s1;
                sf.force = D->force_dev;
                if (D->wide) hipLaunchKernelGGL((dec_sample_kernel<false, true, SMP_KW>), dim3(1), dim3(512), smp_lds_bytes(SMP_KW), st, sf);
                else hipLaunchKernelGGL((dec_sample_kernel<false, true>), dim3(1), dim3(512), 0, st, sf);
            } else {
                if (D->wide) hipLaunchKernelGGL((dec_sample_kernel<false, false, SMP_KW>), dim3(1), dim3(512), smp_lds_bytes(SMP_KW), st, s1);
                else hipLaunchKernelGGL((dec_sample_kernel<false, false>), dim3(1), dim3(512), 0, st, s1);
            }
        }
        PB_LAUNCH_CHECK(); ++n;
    }
    D->launches = n;
    return 0;
}

// ntok == 0: one host-sampled step (B == 1: tok_host goes up, the logits row comes down to logits_host); ntok > 0: ntok device-sampled steps
static int issue(Decoder* D, int ntok) {
    if (ntok == 0) PB_CHECK_HIP(hipMemcpyAsync(D->tok_dev, D->tok_host, 16, hipMemcpyHostToDevice, D->stream));
    for (int k = 0; k < (ntok ? ntok : 1); ++k)
        if (D->B == 1 ? step_issue<false>(D, ntok > 0) : step_issue<true>(D, ntok > 0)) return -1;
    if (ntok == 0)
        PB_CHECK_HIP(hipMemcpyAsync(D->logits_host, D->bp.plan.logits, sizeof(float) * (size_t)D->bp.plan.vocab, hipMemcpyDeviceToHost, D->stream));
    return 0;
}

// issue(D, ntok) captured as graph g (a single linear stream of kernels and copies: no parallel branches); false = capture unavailable
static bool capture(Decoder* D, int g, int ntok) {
    if (hipStreamSynchronize(D->stream) != hipSuccess || hipStreamBeginCapture(D->stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const int rc = issue(D, ntok);
    const hipError_t e = hipStreamEndCapture(D->stream, &D->graph[g]);
    if (rc || e != hipSuccess || !D->graph[g] || hipGraphInstantiate(&D->exec[g], D->graph[g], nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (D->graph[g]) { (void)hipGraphDestroy(D->graph[g]); D->graph[g] = nullptr; }
        D->exec[g] = nullptr;
        return false;
    }
    return true;
}

// keys per cross-attention split of a row with s_enc visible keys: <= ns_cross splits of >= 64 keys
static int cross_chunk(const Decoder* D, int s_enc) {
    const int ck = (s_enc + D->ns_cross - 1) / D->ns_cross;
    return ck < 64 ? 64 : (ck + 15) & ~15;
}

// the rows' geometry as the plan has it (row b: s_enc[b], its own slice b), into the host mirror and, in stream order, into BState
static int geom_reset(Decoder* D) {
    for (int b = 0; b < BMAX; ++b) {
        const int se = b < D->B ? D->bp.s_enc[b] : 1;
        D->geo.s_enc[b] = se; D->geo.ck[b] = cross_chunk(D, se); D->geo.kv_row[b] = b < D->B ? b : 0;
        if (b < D->B) D->ck_cross[b] = D->geo.ck[b];
    }
    hipLaunchKernelGGL(dec_geom_kernel, dim3(1), dim3(64), 0, D->stream, D->st, D->geo);
    PB_LAUNCH_CHECK();
    return 0;
}

static void drop_graphs(Decoder* D) {
    for (int g = 0; g < N_GRAPHS; ++g) {
        if (D->exec[g]) (void)hipGraphExecDestroy(D->exec[g]);
        if (D->graph[g]) (void)hipGraphDestroy(D->graph[g]);
        D->exec[g] = nullptr; D->graph[g] = nullptr;
    }
}

}  // namespace

extern "C" int pb_batch_decoder_create(const pb_decode_batch* bp, void** out) {
    PB_REQUIRE(bp && out, "pb_batch_decoder_create: null argument");
    *out = nullptr;
    const pb_decode_plan* plan = &bp->plan;
    const int d = plan->d, H = plan->H, hd = H > 0 ? d / H : 0;
    // the shapes the fused kernels cover (return 1 = declined, not an error: pb_decode_step or the per-prompt loop), 1 <= B <= 16, every
    // row with a visible encoder extent
    if (plan->dtype != PB_BF16 || H <= 0 || d % H != 0 || (hd != 64 && hd != 128) || d % 256 != 0 || d > 1024 || !plan->attn_part ||
        plan->n_layers <= 0 || plan->n_layers > PB_DECODE_MAX_LAYERS || plan->ffn % 8 != 0 || plan->ffn > 8192 || plan->S <= 0 ||
        bp->B < 1 || bp->B > BMAX) return 1;
    for (int b = 0; b < bp->B; ++b)
        if (bp->s_enc[b] <= 0 || bp->s_enc[b] > plan->S) return 1;
    Decoder* D = new Decoder();
    D->bp = *bp;
    D->B = bp->B;
    if (hipStreamCreateWithFlags(&D->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&D->ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&D->ev_fence, hipEventDisableTiming) != hipSuccess ||
        hipMalloc(&D->st, sizeof(BState)) != hipSuccess || hipMalloc(&D->tok_dev, 16 * BMAX) != hipSuccess ||
        hipHostMalloc(&D->tok_host, 16 * BMAX, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&D->logits_host, sizeof(float) * (size_t)plan->vocab, hipHostMallocDefault) != hipSuccess) {
        pb_set_error("pb_batch_decoder_create: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        pb_batch_decoder_destroy(D);
        return -1;
    }
    // Every (head, split) workgroup projects q of its head itself (hd rows of W_q: 98 KB at cfg 2), so the split count trades K / V rows
    // per workgroup against re-reads of W_q: PB_DECODE_SPLITS_SELF / _CROSS (2 .. 16; developer A/B, profiles/r06_decode_splits_ab.txt).
    // Cross-attention: splits of >= 64 keys over each row's visible encoder positions (fixed for the prompt).
    auto env_splits = [](const char* name, int dflt) { const char* e = getenv(name); int v = e ? atoi(e) : dflt; return v < 2 ? 2 : (v > PB_DECODE_MAX_SPLITS ? PB_DECODE_MAX_SPLITS : v); };
    D->ns_self = env_splits("PB_DECODE_SPLITS_SELF", PB_DECODE_MAX_SPLITS);
    D->ns_cross = env_splits("PB_DECODE_SPLITS_CROSS", PB_DECODE_MAX_SPLITS);
    int ck_max = 0;
    for (int b = 0; b < D->B; ++b) {
        const int ck = cross_chunk(D, bp->s_enc[b]);
        D->ck_cross[b] = ck;
        ck_max = ck > ck_max ? ck : ck_max;
    }
    int ck_self = (plan->S + D->ns_self - 2) / (D->ns_self - 1);
    ck_self = ck_self < 64 ? 64 : (ck_self + 15) & ~15;
    D->lds_attn = sizeof(float) * (size_t)(5 * hd + (ck_max > ck_self ? ck_max : ck_self) + 16);
    if (geom_reset(D)) { pb_batch_decoder_destroy(D); return -1; }     // BState's geometry fields are never read uninitialised
    *out = D;
    return 0;
}

extern "C" int pb_batch_decoder_destroy(void* dec) {
    Decoder* D = (Decoder*)dec;
    if (!D) return 0;
    if (D->stream) (void)hipStreamSynchronize(D->stream);
    drop_graphs(D);
    for (int i = 0; i < SPEC_EVENTS; ++i) if (D->evs[i]) (void)hipEventDestroy(D->evs[i]);
    if (D->u_dev) (void)hipFree(D->u_dev);
    if (D->force_dev) (void)hipFree(D->force_dev);
    if (D->allow_dev) (void)hipFree(D->allow_dev);
    if (D->sched_dev) (void)hipFree(D->sched_dev);
    if (D->anchor_dev) (void)hipFree(D->anchor_dev);
    if (D->log_logits) (void)hipHostFree(D->log_logits);
    if (D->log_tok) (void)hipHostFree(D->log_tok);
    for (int i = 0; i < N_STAGE; ++i) if (D->stage_ev[i]) (void)hipEventDestroy(D->stage_ev[i]);
    if (D->stage) (void)hipHostFree(D->stage);
    if (D->ev_fence) (void)hipEventDestroy(D->ev_fence);
    if (D->ev) (void)hipEventDestroy(D->ev);
    if (D->st) (void)hipFree(D->st);
    if (D->tok_dev) (void)hipFree(D->tok_dev);
    if (D->tok_host) (void)hipHostFree(D->tok_host);
    if (D->logits_host) (void)hipHostFree(D->logits_host);
    if (D->stream) (void)hipStreamDestroy(D->stream);
    delete D;
    return 0;
}

// Rows that share their prompt share its cross K|V (see the header). The map is validated whole before anything changes.
extern "C" int pb_batch_decoder_share_cross(void* dec, int32_t n_groups, const int32_t* kv_row) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && kv_row, "pb_batch_decoder_share_cross: null argument");
    PB_REQUIRE(!D->issued, "pb_batch_decoder_share_cross: a step was already issued; the cross-cache layout is fixed for this decoder");
    PB_REQUIRE(!D->dynamic, "pb_batch_decoder_share_cross: the decoder is dynamic (pb_batch_decoder_dynamic): its rows change slices one by one");
    const int B = D->B;
    PB_REQUIRE(n_groups >= 1 && n_groups <= B, "pb_batch_decoder_share_cross: %d groups for %d rows", n_groups, B);
    int count[BMAX] = {}, s_enc[BMAX] = {};
    for (int b = 0; b < B; ++b) {
        const int g = kv_row[b];
        PB_REQUIRE(g >= 0 && g < n_groups, "pb_batch_decoder_share_cross: row %d names slice %d of %d", b, g, n_groups);
        if (count[g]++ == 0) s_enc[g] = D->bp.s_enc[b];
        PB_REQUIRE(D->bp.s_enc[b] == s_enc[g], "pb_batch_decoder_share_cross: rows of slice %d differ in s_enc (%d, %d): they are not one prompt",
                   g, s_enc[g], D->bp.s_enc[b]);
    }
    for (int g = 0; g < n_groups; ++g) PB_REQUIRE(count[g] > 0, "pb_batch_decoder_share_cross: no row names slice %d", g);
    D->n_groups = n_groups;
    for (int b = 0; b < B; ++b) D->kv_row[b] = kv_row[b];
    // The grouped kernel where rows really share a slice; PB_DECODE_CROSS_GROUPED=0 keeps the per-row kernel reading through kv_row (developer A/B
    // and the fallback), PB_DECODE_GROUP_TILE = 2 / 4 / 8 rows per workgroup.
    const char* eg = getenv("PB_DECODE_CROSS_GROUPED");
    const char* et = getenv("PB_DECODE_GROUP_TILE");
    int rt = et ? atoi(et) : 4;
    rt = rt <= 2 ? 2 : (rt <= 4 ? 4 : 8);
    D->group_rt = 0;
    if (B > 1 && n_groups < B && !(eg && atoi(eg) == 0)) {
        const int d = D->bp.plan.d, hd = d / D->bp.plan.H;
        int ck_max = 0, nt = 0, at = 0;
        for (int b = 0; b < B; ++b) ck_max = D->ck_cross[b] > ck_max ? D->ck_cross[b] : ck_max;
        for (int g = 0; g < n_groups; ++g) {                 // rows in slice order, each slice cut into even tiles of <= rt rows
            const int tiles = (count[g] + rt - 1) / rt;
            int left = count[g], f = at;
            for (int b = 0; b < B; ++b) if (kv_row[b] == g) D->rows_by_group[at++] = b;
            for (int k = 0; k < tiles; ++k) {
                const int n = (left + (tiles - k) - 1) / (tiles - k);
                D->tile_first[nt] = f; D->tile_n[nt] = n; ++nt;
                f += n; left -= n;
            }
        }
        D->n_tiles = nt;
        D->lds_group = (size_t)rt * (sizeof(float) * (size_t)(5 * hd + ((ck_max + 3) & ~3)) + 2 * (size_t)d);
        if (D->lds_group <= 64 * 1024) D->group_rt = rt;   // else: the per-row kernel through kv_row
    }
    return 0;
}

// Start of a prompt / batch: every row at position -1 and live (pos = -1: 0xff bytes, done = 0), ordered behind everything enqueued on the
// caller's stream (encoder passes, cross K/V projections). use_graph = 0 issues the launches of every step directly (A/B, debugging).
extern "C" int pb_batch_decoder_reset(void* dec, void* caller_stream, int32_t use_graph) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D, "pb_batch_decoder_reset: null decoder");
    PB_CHECK_HIP(hipEventRecord(D->ev, (hipStream_t)caller_stream));
    PB_CHECK_HIP(hipStreamWaitEvent(D->stream, D->ev, 0));
    PB_CHECK_HIP(hipMemsetAsync(D->st->pos, 0xff, sizeof(int) * BMAX, D->stream));
    PB_CHECK_HIP(hipMemsetAsync(D->st->done, 0, sizeof(int) * BMAX, D->stream));
    if (D->dynamic && geom_reset(D)) return -1;                        // every slot back to the plan's prompt and its own slice
    for (int b = 0; b < BMAX; ++b) D->live[b] = b < D->B;
    D->steps = 0;
    D->use_graph = use_graph;
    return 0;
}

// One host-sampled step (B == 1): tok8 (the decoder input of this position, 8 ids) goes up, the (vocab) f32 logits row of the position
// comes back into logits_out (host memory). Blocks until the row has landed.
extern "C" int pb_batch_decoder_step(void* dec, const int16_t* tok8, float* logits_out) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->B == 1 && tok8 && logits_out, "pb_batch_decoder_step: null argument or B > 1");
    PB_REQUIRE(D->steps < D->bp.plan.S, "pb_batch_decoder_step: position %d is outside the K/V caches and the position table (S = %d): call "
               "pb_batch_decoder_reset for a new prompt", D->steps, D->bp.plan.S);
    ++D->steps;
    for (int k = 0; k < 8; ++k) D->tok_host[k] = tok8[k];
    if (D->use_graph && !D->exec[G_STEP] && !capture(D, G_STEP, 0)) D->use_graph = 0;     // capture unavailable: direct launches
    if (D->use_graph) PB_CHECK_HIP(hipGraphLaunch(D->exec[G_STEP], D->stream));
    else if (issue(D, 0)) return -1;
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));
    for (int k = 0; k < D->bp.plan.vocab; ++k) logits_out[k] = D->logits_host[k];
    return 0;
}

// ---- device-sampled decode: the sampler's constants and the uniform draws of the whole batch go up once; steps are then enqueued in
// runs (pb_batch_decoder_launch: SPEC_K steps = one graph replay) without waiting for the host; the host follows behind through the pinned
// logs (pb_batch_decoder_wait + pb_batch_decoder_logs), and pb_batch_decoder_seek rewinds a row after a position where it disagrees with
// the device's choice.
extern "C" int pb_batch_decoder_sampler_init(void* dec, const float* temps8, const float* p8, const int32_t* n8, const int32_t* off8, const int32_t* pad8,
                                             const double* u, int64_t n_u, int32_t limit, int32_t fault_row, int32_t fault_period) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && temps8 && p8 && n8 && off8 && pad8 && u, "pb_batch_decoder_sampler_init: null argument");
    const size_t S = (size_t)D->bp.plan.S, B = (size_t)D->B, vocab = (size_t)D->bp.plan.vocab;
    PB_REQUIRE(n_u >= (int64_t)(B * S * 8), "pb_batch_decoder_sampler_init: %lld draws for %d rows x %d positions x 8 heads", (long long)n_u, D->B, (int)S);
    PB_REQUIRE(limit >= 0 && limit <= (int)S, "pb_batch_decoder_sampler_init: limit %d outside 0..%d", limit, (int)S);
    bool wide = false;
    for (int h = 0; h < 8; ++h) {
        wide = wide || n8[h] > SMP_W;
        PB_REQUIRE(n8[h] > 0 && n8[h] <= 64 * SMP_KW && off8[h] >= 0 && off8[h] + n8[h] <= (int)vocab && temps8[h] > 0.f,
                   "pb_batch_decoder_sampler_init: head %d (n %d, offset %d, temperature %g)", h, n8[h], off8[h], (double)temps8[h]);
        D->sa.n[h] = n8[h]; D->sa.off[h] = off8[h]; D->sa.temp[h] = temps8[h]; D->sa.p[h] = p8[h]; D->sa.pad[h] = pad8[h];
    }
    int sorted = 0;
    for (int h = 0; h < 8; ++h) if (p8[h] < 1.0f) sorted += n8[h];
    wide = wide || sorted > 512;                                        // the narrow form ranks with one thread per class under a head with p < 1: 512 of them; the wide form takes rounds
    if (wide) {                                                         // ~104 KB of dynamic LDS: over the default limit, so every wide instantiation opts in
        const int lds = (int)smp_lds_bytes(SMP_KW);
        PB_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_sample_kernel<true, true, SMP_KW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        PB_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_sample_kernel<true, false, SMP_KW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        PB_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_sample_kernel<false, true, SMP_KW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        PB_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dec_sample_kernel<false, false, SMP_KW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    }
    D->wide = wide;
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
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)D->st->limit, limit, BMAX, D->stream));    // every row; pb_batch_decoder_start may set them one by one
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)D->st->stop, pad8[0], BMAX, D->stream));   // no row stops at a bar until pb_batch_decoder_stop says so
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)D->st->rule, -1, 4 * BMAX, D->stream));    // every row is sampled freely, from every class, in every bar, until pb_batch_decoder_order / _allow / _schedule say otherwise
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->opad[0], pad8[0], 1, D->stream));
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->opad[1], pad8[1], 1, D->stream));
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));                     // `u` may be pageable: the copy is done when we return
    D->limit = limit;
    for (int b = 0; b < BMAX; ++b) { D->stop.stop[b] = pad8[0]; D->admit_stop[b] = -1; D->order.order[b] = -1; D->admit_order[b] = -1; }
    for (int b = 0; b < BMAX; ++b) { D->allow.allow[b] = -1; D->admit_allow[b] = -1; }
    D->n_allow = 0;                                                     // the previous run's table (if any) stays allocated and unread: no row points into it
    for (int b = 0; b < BMAX; ++b) { D->sched.sched[b] = -1; D->admit_sched[b] = -1; }
    D->n_sched = 0;                                                     // likewise
    for (int b = 0; b < BMAX; ++b) { D->anchor.base[b] = -1; D->anchor.cnt[b] = 0; D->admit_anchor[b] = -1; D->admit_nanchor[b] = 0; }
    D->n_anchor = 0;                                                    // likewise (the memset of `rule` above cleared the rows' slots)
    D->sa.logits = D->bp.plan.logits; D->sa.u = D->u_dev; D->sa.st = D->st; D->sa.tok_dev = D->tok_dev;
    D->sa.log_logits = D->log_logits; D->sa.log_tok = D->log_tok; D->sa.vocab = (int)vocab; D->sa.S = (int)S;
    D->sa.fault_row = fault_row; D->sa.fault_period = (D->B == 1 && fault_row != 0) ? 0 : fault_period;    // the single-row sampler corrupts row 0
    drop_graphs(D);                                                     // captured with the previous constants
    D->sampler = true;
    return 0;
}

// Which sampler the decoder's steps end with (behind sampler_init): 0 = narrow (every head <= 272 classes and at most 512 classes under the
// heads with p < 1), 1 = wide.
extern "C" int32_t pb_batch_decoder_sampler_form(void* dec) {
    Decoder* D = (Decoder*)dec;
    return (D && D->sampler && D->wide) ? 1 : 0;
}

// Forced tokens (see the header): the (B, S, 8) table of given ids goes up once, into memory the decoder owns. Every value is checked on
// the host against the n8 / S of sampler_init before anything changes; the graphs are captured afterwards, with the FORCED sampler node.
extern "C" int pb_batch_decoder_force(void* dec, const int16_t* forced) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && forced, "pb_batch_decoder_force: null argument");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_force: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(!D->issued, "pb_batch_decoder_force: a step was already issued; the sampler kernel is fixed for this decoder");
    PB_REQUIRE(!D->n_anchor, "pb_batch_decoder_force: the decoder carries anchors (pb_batch_decoder_anchor): position-indexed and time-indexed givens do not combine");
    const size_t n = (size_t)D->B * (size_t)D->bp.plan.S * 8;
    for (size_t k = 0; k < n; ++k) {
        const int v = forced[k], h = (int)(k & 7);
        PB_REQUIRE(v == -1 || (v >= 0 && v < D->sa.n[h]), "pb_batch_decoder_force: row %d, position %d, head %d: id %d is neither -1 nor inside the "
                   "head's table (%d ids)", (int)(k / 8 / (size_t)D->bp.plan.S), (int)(k / 8 % (size_t)D->bp.plan.S), h, v, D->sa.n[h]);
    }
    int16_t* tab = nullptr;
    if (hipMalloc(&tab, sizeof(int16_t) * n) != hipSuccess) {
        pb_set_error("pb_batch_decoder_force: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return -1;
    }
    if (hipMemcpyAsync(tab, forced, sizeof(int16_t) * n, hipMemcpyHostToDevice, D->stream) != hipSuccess ||
        hipStreamSynchronize(D->stream) != hipSuccess) {         // `forced` may be pageable: the copy is done when we return
        pb_set_error("pb_batch_decoder_force: upload failed: %s", hipGetErrorString(hipGetLastError()));
        (void)hipFree(tab);
        return -1;
    }
    if (D->force_dev) (void)hipFree(D->force_dev);
    D->force_dev = tab;
    return 0;
}

// Stop at a bar (see the header): one bar id per row, checked whole on the host before anything changes, then stored in decoder-stream
// order by a small kernel that takes the values by kernarg (as dec_geom_kernel does), so nothing of the caller's has to outlive the call.
extern "C" int pb_batch_decoder_stop(void* dec, const int32_t* stop_bar) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && stop_bar, "pb_batch_decoder_stop: null argument");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_stop: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(!D->issued, "pb_batch_decoder_stop: a step was already issued; the rows' stop bars are set before the run's first step");
    for (int b = 0; b < D->B; ++b)
        PB_REQUIRE(stop_bar[b] >= 0 && stop_bar[b] <= D->sa.pad[0], "pb_batch_decoder_stop: row %d: bar %d outside 0..%d (%d = no stop)", b, stop_bar[b],
                   D->sa.pad[0], D->sa.pad[0]);
    StopArgs g = D->stop;
    for (int b = 0; b < D->B; ++b) g.stop[b] = stop_bar[b];
    if (D->B == 1) {                                                   // the single-row kernels have no done flag: the host ends the run. No device work;
        D->stop = g;                                                   // the mirror keeps the bar for an anchored row's rule (pb_batch_decoder_anchor, _start)
        return 0;
    }
    hipLaunchKernelGGL(dec_stop_kernel, dim3(1), dim3(64), 0, D->stream, D->st, g);
    PB_LAUNCH_CHECK();
    D->stop = g;
    return 0;
}

// Time-ordered sampling (see the header): one bar floor per row (-1: a free row), checked whole on the host before anything changes, then
// stored in decoder-stream order by a small kernel that takes the values by kernarg, as the stop bars are. Unlike them it reaches the
// single-row sampler too: a B = 1 run samples on the device, and a kernel that did not know the constraint would be rewound wherever it bites.
extern "C" int pb_batch_decoder_order(void* dec, const int32_t* floor) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && floor, "pb_batch_decoder_order: null argument");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_order: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(!D->issued, "pb_batch_decoder_order: a step was already issued; the rows' bar floors are set before the run's first step");
    for (int b = 0; b < D->B; ++b)
        PB_REQUIRE(floor[b] >= -1 && floor[b] < D->sa.pad[0], "pb_batch_decoder_order: row %d: floor %d outside -1..%d (-1 = not ordered)", b, floor[b],
                   D->sa.pad[0] - 1);
    OrderArgs g = D->order;
    for (int b = 0; b < D->B; ++b) g.order[b] = floor[b];
    hipLaunchKernelGGL(dec_order_kernel, dim3(1), dim3(64), 0, D->stream, D->st, g);
    PB_LAUNCH_CHECK();
    D->order = g;
    return 0;
}

// Allowed classes (see the header): the table of distinct masks goes up once, into memory the decoder owns, and one index per row is stored
// beside the rows' bar floors in decoder-stream order by a small kernel that takes them by kernarg. Everything is checked on the host
// before anything changes. Like the bar floors it reaches the single-row sampler too.
extern "C" int pb_batch_decoder_allow(void* dec, const uint32_t* masks, int32_t n_masks, int32_t words, const int32_t* row_mask) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && masks && row_mask, "pb_batch_decoder_allow: null argument");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_allow: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(!D->issued, "pb_batch_decoder_allow: a step was already issued; the rows' allow masks are set before the run's first step");
    PB_REQUIRE(!D->n_sched, "pb_batch_decoder_allow: a bar schedule points into the table in place; upload the masks before pb_batch_decoder_schedule");
    PB_REQUIRE(n_masks > 0 && n_masks <= 65536, "pb_batch_decoder_allow: %d masks (1 .. 65536)", n_masks);
    PB_REQUIRE(words == (D->sa.vocab + 31) / 32, "pb_batch_decoder_allow: %d words per mask for %d vocabulary columns (%d)", words, D->sa.vocab,
               (D->sa.vocab + 31) / 32);
    for (int b = 0; b < D->B; ++b)
        PB_REQUIRE(row_mask[b] >= -1 && row_mask[b] < n_masks, "pb_batch_decoder_allow: row %d: mask index %d outside -1..%d (-1 = every class allowed)", b,
                   row_mask[b], n_masks - 1);
    const size_t bytes = sizeof(uint32_t) * (size_t)n_masks * (size_t)words;
    uint32_t* tab = nullptr;
    if (hipMalloc(&tab, bytes) != hipSuccess) {
        pb_set_error("pb_batch_decoder_allow: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return -1;
    }
    if (hipMemcpyAsync(tab, masks, bytes, hipMemcpyHostToDevice, D->stream) != hipSuccess ||
        hipStreamSynchronize(D->stream) != hipSuccess) {         // `masks` may be pageable: the copy is done when we return
        pb_set_error("pb_batch_decoder_allow: upload failed: %s", hipGetErrorString(hipGetLastError()));
        (void)hipFree(tab);
        return -1;
    }
    AllowArgs g = D->allow;
    for (int b = 0; b < D->B; ++b) g.allow[b] = row_mask[b];
    g.words = words; g.table = tab;
    hipLaunchKernelGGL(dec_allow_kernel, dim3(1), dim3(64), 0, D->stream, D->st, g);
    if (hipGetLastError() != hipSuccess) {
        pb_set_error("pb_batch_decoder_allow: launch failed");
        (void)hipFree(tab);
        return -1;
    }
    if (D->allow_dev) (void)hipFree(D->allow_dev);               // the previous table: no row has pointed into it since sampler_init (hipFree drains the device)
    D->allow_dev = tab; D->n_allow = n_masks;
    D->allow = g;
    return 0;
}

// Bar schedules (see the header): the table of distinct schedules goes up once, into memory the decoder owns, and one index per row is
// stored beside the rows' allow masks in decoder-stream order by a small kernel. Its entries index the masks pb_batch_decoder_allow
// uploaded, so that call comes first. Everything is checked on the host before anything changes.
extern "C" int pb_batch_decoder_schedule(void* dec, const int32_t* table, int32_t n_sched, int32_t nbar, const int32_t* row_sched) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && table && row_sched, "pb_batch_decoder_schedule: null argument");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_schedule: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(!D->issued, "pb_batch_decoder_schedule: a step was already issued; the rows' bar schedules are set before the run's first step");
    PB_REQUIRE(n_sched > 0 && n_sched <= 65536, "pb_batch_decoder_schedule: %d schedules (1 .. 65536)", n_sched);
    PB_REQUIRE(nbar == D->sa.pad[0], "pb_batch_decoder_schedule: %d entries per schedule for %d ordinary bar ids (pad[0])", nbar, D->sa.pad[0]);
    for (size_t i = 0; i < (size_t)n_sched * (size_t)nbar; ++i)
        PB_REQUIRE(table[i] >= -1 && table[i] < D->n_allow, "pb_batch_decoder_schedule: schedule %d, bar %d: mask index %d outside -1..%d (-1 = the row's own "
                   "mask; the table is pb_batch_decoder_allow's)", (int)(i / nbar), (int)(i % nbar), table[i], D->n_allow - 1);
    for (int b = 0; b < D->B; ++b)
        PB_REQUIRE(row_sched[b] >= -1 && row_sched[b] < n_sched, "pb_batch_decoder_schedule: row %d: schedule index %d outside -1..%d (-1 = no schedule)", b,
                   row_sched[b], n_sched - 1);
    const size_t bytes = sizeof(int) * (size_t)n_sched * (size_t)nbar;
    int* tab = nullptr;
    if (hipMalloc(&tab, bytes) != hipSuccess) {
        pb_set_error("pb_batch_decoder_schedule: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return -1;
    }
    if (hipMemcpyAsync(tab, table, bytes, hipMemcpyHostToDevice, D->stream) != hipSuccess ||
        hipStreamSynchronize(D->stream) != hipSuccess) {         // `table` may be pageable: the copy is done when we return
        pb_set_error("pb_batch_decoder_schedule: upload failed: %s", hipGetErrorString(hipGetLastError()));
        (void)hipFree(tab);
        return -1;
    }
    SchedArgs g = D->sched;
    for (int b = 0; b < D->B; ++b) g.sched[b] = row_sched[b];
    g.nbar = nbar; g.table = tab;
    hipLaunchKernelGGL(dec_sched_kernel, dim3(1), dim3(64), 0, D->stream, D->st, g);
    if (hipGetLastError() != hipSuccess) {
        pb_set_error("pb_batch_decoder_schedule: launch failed");
        (void)hipFree(tab);
        return -1;
    }
    if (D->sched_dev) (void)hipFree(D->sched_dev);               // the previous table: no row has pointed into it since sampler_init (hipFree drains the device)
    D->sched_dev = tab; D->n_sched = n_sched;
    D->sched = g;
    return 0;
}

// Enqueue `ntok` steps; first_tok ((B, 8) host ids, may be NULL) is copied up in front as the rows' decoder inputs. Row form: a row stops
// by itself at the limit; B == 1: the steps must stay within it. Returns a ticket >= 0 for pb_batch_decoder_wait, < 0 on error.
extern "C" int pb_batch_decoder_launch(void* dec, int32_t ntok, const int16_t* first_tok) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->sampler, "pb_batch_decoder_launch: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(ntok > 0, "pb_batch_decoder_launch: %d steps", ntok);
    PB_REQUIRE(D->B > 1 || D->steps + ntok <= D->limit, "pb_batch_decoder_launch: %d steps from position %d pass the limit %d", ntok, D->steps, D->limit);
    if (first_tok) {
        PB_CHECK_HIP(hipStreamSynchronize(D->stream));                 // tok_host is about to be rewritten: no copy of it may be in flight
        for (int k = 0; k < 8 * D->B; ++k) D->tok_host[k] = first_tok[k];
        PB_CHECK_HIP(hipMemcpyAsync(D->tok_dev, D->tok_host, 16 * (size_t)D->B, hipMemcpyHostToDevice, D->stream));
    }
    if (D->use_graph && !D->exec[G_ONE] && (!capture(D, G_ONE, 1) || !capture(D, G_RUN, SPEC_K))) D->use_graph = 0;
    int left = ntok;
    while (left > 0) {
        if (D->use_graph && left >= SPEC_K) { PB_CHECK_HIP(hipGraphLaunch(D->exec[G_RUN], D->stream)); left -= SPEC_K; }
        else if (D->use_graph) { PB_CHECK_HIP(hipGraphLaunch(D->exec[G_ONE], D->stream)); left -= 1; }
        else { if (issue(D, 1)) return -1; left -= 1; }
    }
    D->steps += ntok;
    const int tk = D->next_ev;
    D->next_ev = (D->next_ev + 1) % SPEC_EVENTS;
    PB_CHECK_HIP(hipEventRecord(D->evs[tk], D->stream));
    return tk;
}
extern "C" int pb_batch_decoder_wait(void* dec, int32_t ticket) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->sampler && ticket >= 0 && ticket < SPEC_EVENTS, "pb_batch_decoder_wait: bad ticket %d", ticket);
    PB_CHECK_HIP(hipEventSynchronize(D->evs[ticket]));
    return 0;
}
extern "C" int pb_batch_decoder_logs(void* dec, float** logits_rows, int16_t** tok_rows) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->sampler && logits_rows && tok_rows, "pb_batch_decoder_logs: no sampler");
    *logits_rows = D->log_logits; *tok_rows = D->log_tok;
    return 0;
}
// Rewind one row (tok8 != NULL): drain what is enqueued, then row's last decoded position = pos, its next input = tok8, live again. The
// other rows keep their positions, inputs and flags. tok8 == NULL: the row is done from the next enqueued step on (no drain).
extern "C" int pb_batch_decoder_seek(void* dec, int32_t row, int32_t pos, const int16_t* tok8) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && row >= 0 && row < D->B, "pb_batch_decoder_seek: row %d", row);
    if (!tok8) {
        PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->done[row], 1, 1, D->stream));
        D->live[row] = false;
        return 0;
    }
    PB_REQUIRE(pos >= -1 && pos < D->bp.plan.S, "pb_batch_decoder_seek: position %d", pos);
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));
    for (int k = 0; k < 8; ++k) D->tok_host[row * 8 + k] = tok8[k];
    PB_CHECK_HIP(hipMemcpyAsync(D->tok_dev + row * 8, D->tok_host + row * 8, 16, hipMemcpyHostToDevice, D->stream));
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->pos[row], pos, 1, D->stream));
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->done[row], 0, 1, D->stream));
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));
    D->steps = pos + 1;
    D->live[row] = true;
    return 0;
}

// Primed start (after reset, and after sampler_init where there is one): every row at its own last decoded position last_pos[b] (-1 = none,
// up to S - 1: the prefix rows' K|V are in the self-attention cache), with next_tok[b] as its next decoder input and limit[b] (NULL: the
// sampler's limit, S without a sampler) as the position it stops before. The whole row state goes up in one copy. B == 1: the host bound
// of the single-row kernels follows (steps = last_pos[0] + 1, limit = limit[0]).
extern "C" int pb_batch_decoder_start(void* dec, const int32_t* last_pos, const int16_t* next_tok, const int32_t* limit) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && last_pos && next_tok, "pb_batch_decoder_start: null argument");
    const int S = D->bp.plan.S, B = D->B, dflt = D->sampler ? D->limit : S;
    BState h{};
    for (int b = 0; b < BMAX; ++b) {
        h.pos[b] = -1; h.done[b] = 0; h.limit[b] = dflt;
        h.s_enc[b] = D->geo.s_enc[b]; h.ck[b] = D->geo.ck[b]; h.kv_row[b] = D->geo.kv_row[b];
        h.stop[b] = D->stop.stop[b];                                  // as sampler_init / pb_batch_decoder_stop left it (unread without a sampler)
        h.rule[b].order = D->sampler ? D->order.order[b] : -1;        // ... / pb_batch_decoder_order
        h.rule[b].allow = D->sampler ? D->allow.allow[b] : -1;        // ... / pb_batch_decoder_allow
        h.rule[b].sched = D->sampler ? D->sched.sched[b] : -1;        // ... / pb_batch_decoder_schedule
        const bool anchored = D->sampler && D->n_anchor && D->anchor.cnt[b] > 0;
        h.rule[b].reserved = anchored ? D->anchor.base[b] : -1;      // ... / pb_batch_decoder_anchor
        h.acnt[b] = anchored ? D->anchor.cnt[b] : 0; h.aplaced[b] = 0; // a start is the row's first position: no anchor placed
    }
    for (int k = 0; k < 8; ++k) h.apad[k] = D->sa.pad[k];
    h.atab = D->n_anchor ? D->anchor_dev : nullptr;
    h.opad[0] = D->sa.pad[0]; h.opad[1] = D->sa.pad[1];
    h.awords = D->allow.words; h.amask = D->n_allow ? D->allow_dev : nullptr;
    h.nbar = D->sched.nbar; h.stab = D->n_sched ? D->sched_dev : nullptr;
    for (int b = 0; b < B; ++b) {
        PB_REQUIRE(last_pos[b] >= -1 && last_pos[b] < S, "pb_batch_decoder_start: row %d at position %d (S = %d)", b, last_pos[b], S);
        PB_REQUIRE(!limit || (limit[b] >= 0 && limit[b] <= S), "pb_batch_decoder_start: row %d limit %d outside 0..%d", b, limit[b], S);
        h.pos[b] = last_pos[b];
        if (limit) h.limit[b] = limit[b];
    }
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));                     // tok_host may still be read by an enqueued copy
    for (int k = 0; k < 8 * B; ++k) D->tok_host[k] = next_tok[k];
    PB_CHECK_HIP(hipMemcpyAsync(D->tok_dev, D->tok_host, 16 * (size_t)B, hipMemcpyHostToDevice, D->stream));
    PB_CHECK_HIP(hipMemcpyAsync(D->st, &h, sizeof(BState), hipMemcpyHostToDevice, D->stream));
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));                     // `h` lives on this stack
    D->steps = h.pos[0] + 1;
    D->limit = h.limit[0];
    for (int b = 0; b < BMAX; ++b) D->live[b] = b < B;
    return 0;
}

// Refill (see the header): from here on the rows' cross-attention geometry is read from BState, so pb_batch_decoder_admit can hand a
// slot to another prompt between two replays of the captured graphs. The LDS of the cross-attention launch is sized for the largest
// keys-per-split any s_enc <= S gives.
extern "C" int pb_batch_decoder_dynamic(void* dec, int32_t n_slices) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D, "pb_batch_decoder_dynamic: null decoder");
    PB_REQUIRE(!D->issued, "pb_batch_decoder_dynamic: a step was already issued; the cross-attention kernel is fixed for this decoder");
    PB_REQUIRE(D->B > 1, "pb_batch_decoder_dynamic: a B = 1 decoder runs the single-row kernels");
    PB_REQUIRE(!D->n_groups, "pb_batch_decoder_dynamic: the decoder shares cross slices (pb_batch_decoder_share_cross)");
    PB_REQUIRE(!D->dynamic, "pb_batch_decoder_dynamic: the decoder is already dynamic");
    PB_REQUIRE(n_slices >= D->B && n_slices <= 2 * BMAX, "pb_batch_decoder_dynamic: %d slices for %d rows (B .. %d)", n_slices, D->B, 2 * BMAX);
    const int S = D->bp.plan.S, hd = D->bp.plan.d / D->bp.plan.H;
    const size_t bytes = ((size_t)S * (8 * sizeof(double) + 8 * sizeof(int16_t) + sizeof(float)) + 63) & ~(size_t)63;
    char* stage = nullptr;
    if (hipHostMalloc(&stage, bytes * N_STAGE, hipHostMallocDefault) != hipSuccess) {
        pb_set_error("pb_batch_decoder_dynamic: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return -1;
    }
    for (int i = 0; i < N_STAGE; ++i)
        if (hipEventCreateWithFlags(&D->stage_ev[i], hipEventDisableTiming) != hipSuccess) {
            pb_set_error("pb_batch_decoder_dynamic: event creation failed: %s", hipGetErrorString(hipGetLastError()));
            for (int k = 0; k <= i; ++k) if (D->stage_ev[k]) { (void)hipEventDestroy(D->stage_ev[k]); D->stage_ev[k] = nullptr; }
            (void)hipHostFree(stage);
            return -1;
        }
    D->stage = stage; D->stage_bytes = bytes;
    int ck_self = (S + D->ns_self - 2) / (D->ns_self - 1);
    ck_self = ck_self < 64 ? 64 : (ck_self + 15) & ~15;
    const int ck_max = cross_chunk(D, S);                              // ck grows with s_enc
    D->lds_attn = sizeof(float) * (size_t)(5 * hd + (ck_max > ck_self ? ck_max : ck_self) + 16);
    D->dynamic = n_slices;
    return 0;
}

// The hand-over of a slot. Everything is checked on the host first; then, in decoder-stream order behind an event on the caller's stream:
// the row's draws, forced entries and mask (out of a pinned staging entry: the caller's arrays are free when we return) and one small
// kernel that replaces the row's state. No synchronize and no host wait: the other rows run on.
extern "C" int pb_batch_decoder_admit(void* dec, int32_t row, int32_t slice, int32_t s_enc, int32_t last_pos, const int16_t* next_tok8, int32_t limit,
                                      const double* u_row, const int16_t* forced_row, const float* mask_row, void* caller_stream) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->dynamic, "pb_batch_decoder_admit: not a dynamic decoder (pb_batch_decoder_dynamic)");
    PB_REQUIRE(D->sampler && D->u_dev, "pb_batch_decoder_admit: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(next_tok8 && u_row, "pb_batch_decoder_admit: null argument");
    const int S = D->bp.plan.S;
    PB_REQUIRE(row >= 0 && row < D->B, "pb_batch_decoder_admit: row %d of %d", row, D->B);
    PB_REQUIRE(!D->live[row], "pb_batch_decoder_admit: row %d is live; end it first (pb_batch_decoder_seek with tok8 = NULL)", row);
    PB_REQUIRE(slice >= 0 && slice < D->dynamic, "pb_batch_decoder_admit: slice %d of %d", slice, D->dynamic);
    for (int b = 0; b < D->B; ++b)
        PB_REQUIRE(!(D->live[b] && D->geo.kv_row[b] == slice), "pb_batch_decoder_admit: slice %d is being read by the live row %d", slice, b);
    PB_REQUIRE(s_enc > 0 && s_enc <= S, "pb_batch_decoder_admit: s_enc %d outside 1..%d", s_enc, S);
    PB_REQUIRE(last_pos >= -1 && last_pos < limit && limit <= S, "pb_batch_decoder_admit: position %d, limit %d (-1 <= position < limit <= %d)", last_pos, limit, S);
    PB_REQUIRE(!forced_row || D->force_dev, "pb_batch_decoder_admit: a forced row needs the decoder's force table (pb_batch_decoder_force before the first step; "
               "an all -1 table will do)");
    PB_REQUIRE((mask_row != nullptr) == (D->bp.plan.enc_mask != nullptr), "pb_batch_decoder_admit: the plan has %s encoder mask", D->bp.plan.enc_mask ? "an" : "no");
    for (int h = 0; h < 8; ++h)
        PB_REQUIRE(next_tok8[h] >= 0 && next_tok8[h] < D->sa.n[h], "pb_batch_decoder_admit: input id %d of head %d is outside its table (%d ids)",
                   next_tok8[h], h, D->sa.n[h]);
    if (forced_row)
        for (size_t k = 0; k < (size_t)S * 8; ++k) {
            const int v = forced_row[k], h = (int)(k & 7);
            PB_REQUIRE(v == -1 || (v >= 0 && v < D->sa.n[h]), "pb_batch_decoder_admit: position %d, head %d: id %d is neither -1 nor inside the head's table "
                       "(%d ids)", (int)(k / 8), h, v, D->sa.n[h]);
        }
    const int e = D->next_stage;
    if (D->stage_used[e] && hipEventQuery(D->stage_ev[e]) != hipSuccess) {
        (void)hipGetLastError();
        pb_set_error("pb_batch_decoder_admit: %d admissions are still in flight; wait for a launch ticket first", N_STAGE);
        return -1;
    }
    char* sg = D->stage + (size_t)e * D->stage_bytes;
    double* su = (double*)sg;
    int16_t* sf = (int16_t*)(su + (size_t)S * 8);
    float* sm = (float*)(sf + (size_t)S * 8);
    for (size_t k = 0; k < (size_t)S * 8; ++k) su[k] = u_row[k];
    if (forced_row) for (size_t k = 0; k < (size_t)S * 8; ++k) sf[k] = forced_row[k];
    if (mask_row) for (int k = 0; k < S; ++k) sm[k] = mask_row[k];
    AdmitArgs a{};
    a.st = D->st; a.tok_dev = D->tok_dev; a.row = row; a.s_enc = s_enc; a.ck = cross_chunk(D, s_enc); a.slice = slice; a.pos = last_pos; a.limit = limit;
    a.stop = D->admit_stop[row] >= 0 ? D->admit_stop[row] : D->sa.pad[0];    // never the previous occupant's
    a.order = D->admit_order[row];                                           // -1 unless staged: nor its bar floor
    a.allow = D->admit_allow[row];                                           // ... nor its allow mask
    a.sched = D->admit_sched[row];                                           // ... nor its bar schedule
    a.anchor = D->admit_nanchor[row] > 0 ? D->admit_anchor[row] : -1;        // ... nor its anchors
    a.n_anchor = D->admit_nanchor[row];
    for (int h = 0; h < 8; ++h) a.tok[h] = next_tok8[h];
    PB_CHECK_HIP(hipEventRecord(D->ev, (hipStream_t)caller_stream));
    PB_CHECK_HIP(hipStreamWaitEvent(D->stream, D->ev, 0));
    D->stage_used[e] = true;
    D->next_stage = (e + 1) % N_STAGE;
    PB_CHECK_HIP(hipMemcpyAsync(D->u_dev + (size_t)row * S * 8, su, sizeof(double) * (size_t)S * 8, hipMemcpyHostToDevice, D->stream));
    if (D->force_dev) {
        int16_t* fr = D->force_dev + (size_t)row * S * 8;
        if (forced_row) PB_CHECK_HIP(hipMemcpyAsync(fr, sf, sizeof(int16_t) * (size_t)S * 8, hipMemcpyHostToDevice, D->stream));
        else PB_CHECK_HIP(hipMemsetAsync(fr, 0xff, sizeof(int16_t) * (size_t)S * 8, D->stream));       // -1 everywhere: all free
    }
    if (mask_row)
        PB_CHECK_HIP(hipMemcpyAsync(const_cast<float*>(D->bp.plan.enc_mask) + (size_t)row * S, sm, sizeof(float) * (size_t)S, hipMemcpyHostToDevice, D->stream));
    hipLaunchKernelGGL(dec_admit_kernel, dim3(1), dim3(64), 0, D->stream, a);
    PB_LAUNCH_CHECK();
    PB_CHECK_HIP(hipEventRecord(D->stage_ev[e], D->stream));
    D->geo.s_enc[row] = s_enc; D->geo.ck[row] = a.ck; D->geo.kv_row[row] = slice; D->ck_cross[row] = a.ck;
    D->stop.stop[row] = a.stop; D->admit_stop[row] = -1;
    D->order.order[row] = a.order; D->admit_order[row] = -1;
    D->allow.allow[row] = a.allow; D->admit_allow[row] = -1;
    D->sched.sched[row] = a.sched; D->admit_sched[row] = -1;
    D->anchor.base[row] = a.anchor; D->anchor.cnt[row] = a.n_anchor; D->admit_anchor[row] = -1; D->admit_nanchor[row] = 0;
    D->live[row] = true;
    return 0;
}

// The stop bar of the prompt the next pb_batch_decoder_admit puts into `row` (see the header). Host state only: the store is the admit's.
extern "C" int pb_batch_decoder_admit_stop(void* dec, int32_t row, int32_t stop_bar) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->dynamic, "pb_batch_decoder_admit_stop: not a dynamic decoder (pb_batch_decoder_dynamic)");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_admit_stop: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(row >= 0 && row < D->B, "pb_batch_decoder_admit_stop: row %d of %d", row, D->B);
    PB_REQUIRE(stop_bar >= 0 && stop_bar <= D->sa.pad[0], "pb_batch_decoder_admit_stop: row %d: bar %d outside 0..%d (%d = no stop)", row, stop_bar,
               D->sa.pad[0], D->sa.pad[0]);
    D->admit_stop[row] = stop_bar;
    return 0;
}

// The bar floor of the prompt the next pb_batch_decoder_admit puts into `row` (see the header). Host state only: the store is the admit's.
extern "C" int pb_batch_decoder_admit_order(void* dec, int32_t row, int32_t floor) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->dynamic, "pb_batch_decoder_admit_order: not a dynamic decoder (pb_batch_decoder_dynamic)");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_admit_order: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(row >= 0 && row < D->B, "pb_batch_decoder_admit_order: row %d of %d", row, D->B);
    PB_REQUIRE(floor >= -1 && floor < D->sa.pad[0], "pb_batch_decoder_admit_order: row %d: floor %d outside -1..%d (-1 = not ordered)", row, floor,
               D->sa.pad[0] - 1);
    D->admit_order[row] = floor;
    return 0;
}

// The allow mask (an index into pb_batch_decoder_allow's table) of the prompt the next pb_batch_decoder_admit puts into `row` (see the
// header). Host state only: the store is the admit's.
extern "C" int pb_batch_decoder_admit_allow(void* dec, int32_t row, int32_t mask_index) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->dynamic, "pb_batch_decoder_admit_allow: not a dynamic decoder (pb_batch_decoder_dynamic)");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_admit_allow: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(row >= 0 && row < D->B, "pb_batch_decoder_admit_allow: row %d of %d", row, D->B);
    PB_REQUIRE(mask_index >= -1 && mask_index < D->n_allow, "pb_batch_decoder_admit_allow: row %d: mask index %d outside -1..%d (-1 = every class allowed; the "
               "table is pb_batch_decoder_allow's)", row, mask_index, D->n_allow - 1);
    D->admit_allow[row] = mask_index;
    return 0;
}

// The bar schedule (an index into pb_batch_decoder_schedule's table) of the prompt the next pb_batch_decoder_admit puts into `row` (see the
// header). Host state only: the store is the admit's.
extern "C" int pb_batch_decoder_admit_schedule(void* dec, int32_t row, int32_t sched_index) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->dynamic, "pb_batch_decoder_admit_schedule: not a dynamic decoder (pb_batch_decoder_dynamic)");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_admit_schedule: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(row >= 0 && row < D->B, "pb_batch_decoder_admit_schedule: row %d of %d", row, D->B);
    PB_REQUIRE(sched_index >= -1 && sched_index < D->n_sched, "pb_batch_decoder_admit_schedule: row %d: schedule index %d outside -1..%d (-1 = no schedule; the "
               "table is pb_batch_decoder_schedule's)", row, sched_index, D->n_sched - 1);
    D->admit_sched[row] = sched_index;
    return 0;
}

// Anchored notes (see the header). anchor_check: `cnt` rows of 8 ids at `a` are ordinary ids in non-decreasing (bar, position) order
// with every bar in floor .. stop - 1; the message names `who`.
static int anchor_check(const Decoder* D, const int16_t* a, int cnt, int floor, int stop, const char* who, int row) {
    for (int i = 0; i < cnt; ++i) {
        for (int h = 0; h < 8; ++h)
            PB_REQUIRE(a[i * 8 + h] >= 0 && a[i * 8 + h] < D->sa.pad[h], "%s: row %d, anchor %d, head %d: id %d is not an ordinary id 0..%d", who, row, i, h,
                       (int)a[i * 8 + h], D->sa.pad[h] - 1);
        PB_REQUIRE(i == 0 || a[i * 8] > a[i * 8 - 8] || (a[i * 8] == a[i * 8 - 8] && a[i * 8 + 1] >= a[i * 8 - 7]),
                   "%s: row %d, anchor %d at (bar %d, position %d) lies in front of anchor %d at (%d, %d): anchors come in time order", who, row, i,
                   (int)a[i * 8], (int)a[i * 8 + 1], i - 1, (int)a[i * 8 - 8], (int)a[i * 8 - 7]);
        PB_REQUIRE(a[i * 8] >= floor && a[i * 8] < stop, "%s: row %d, anchor %d: bar %d outside the row's bars %d..%d (its floor and its stop bar)", who, row, i,
                   (int)a[i * 8], floor, stop - 1);
    }
    return 0;
}

// The table of the anchors of ALL rows of the call goes up once, into memory the decoder owns; each row's base and count are stored, with
// a counter of 0, in decoder-stream order by a small kernel that takes them by kernarg. Behind pb_batch_decoder_stop / _order (the rows'
// bars are checked against them). Everything is checked on the host before anything changes. It reaches the single-row sampler too.
extern "C" int pb_batch_decoder_anchor(void* dec, const int16_t* rows, int32_t n_rows, const int32_t* row_base, const int32_t* row_cnt) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && rows && row_base && row_cnt, "pb_batch_decoder_anchor: null argument");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_anchor: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(!D->issued, "pb_batch_decoder_anchor: a step was already issued; the rows' anchors are set before the run's first step");
    PB_REQUIRE(!D->force_dev, "pb_batch_decoder_anchor: the decoder has a force table (pb_batch_decoder_force): position-indexed and time-indexed givens do "
               "not combine");
    PB_REQUIRE(n_rows > 0 && n_rows <= (1 << 20), "pb_batch_decoder_anchor: %d anchor rows (1 .. %d)", n_rows, 1 << 20);
    for (int b = 0; b < D->B; ++b) {
        PB_REQUIRE(row_cnt[b] >= 0 && row_base[b] >= 0 && (long long)row_base[b] + row_cnt[b] <= n_rows,
                   "pb_batch_decoder_anchor: row %d: anchors %d .. %d + %d outside the table's %d rows", b, row_base[b], row_base[b], row_cnt[b], n_rows);
        PB_REQUIRE(row_cnt[b] <= D->bp.plan.S, "pb_batch_decoder_anchor: row %d: %d anchors for a window of %d positions", b, row_cnt[b], D->bp.plan.S);
    }
    for (int i = 0; i < n_rows; ++i)
        for (int h = 0; h < 8; ++h)
            PB_REQUIRE(rows[i * 8 + h] >= 0 && rows[i * 8 + h] < D->sa.pad[h], "pb_batch_decoder_anchor: table row %d, head %d: id %d is not an ordinary id 0..%d", i,
                       h, (int)rows[i * 8 + h], D->sa.pad[h] - 1);
    for (int b = 0; b < D->B; ++b)
        if (anchor_check(D, rows + (size_t)row_base[b] * 8, row_cnt[b], D->order.order[b] > 0 ? D->order.order[b] : 0, D->stop.stop[b], "pb_batch_decoder_anchor", b))
            return -1;
    const size_t bytes = sizeof(int16_t) * 8 * (size_t)n_rows;
    int16_t* tab = nullptr;
    if (hipMalloc(&tab, bytes) != hipSuccess) {
        pb_set_error("pb_batch_decoder_anchor: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        return -1;
    }
    if (hipMemcpyAsync(tab, rows, bytes, hipMemcpyHostToDevice, D->stream) != hipSuccess ||
        hipStreamSynchronize(D->stream) != hipSuccess) {         // `rows` may be pageable: the copy is done when we return
        pb_set_error("pb_batch_decoder_anchor: upload failed: %s", hipGetErrorString(hipGetLastError()));
        (void)hipFree(tab);
        return -1;
    }
    AnchorArgs g = D->anchor;
    for (int b = 0; b < D->B; ++b) { g.base[b] = row_cnt[b] > 0 ? row_base[b] : -1; g.cnt[b] = row_cnt[b]; }
    for (int h = 0; h < 8; ++h) g.pad[h] = D->sa.pad[h];
    g.table = tab;
    hipLaunchKernelGGL(dec_anchor_kernel, dim3(1), dim3(64), 0, D->stream, D->st, g);
    if (hipGetLastError() != hipSuccess) {
        pb_set_error("pb_batch_decoder_anchor: launch failed");
        (void)hipFree(tab);
        return -1;
    }
    if (D->anchor_dev) (void)hipFree(D->anchor_dev);             // the previous table: no row has pointed into it since sampler_init (hipFree drains the device)
    D->anchor_dev = tab; D->n_anchor = n_rows;
    D->anchor_host.assign(rows, rows + (size_t)n_rows * 8);
    D->anchor = g;
    return 0;
}

// The anchors (rows base .. base + cnt - 1 of pb_batch_decoder_anchor's table) of the prompt the next pb_batch_decoder_admit puts into
// `row` (see the header); behind the row's pb_batch_decoder_admit_stop / _admit_order, against which the bars are checked. Host state only.
extern "C" int pb_batch_decoder_admit_anchor(void* dec, int32_t row, int32_t base, int32_t cnt) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->dynamic, "pb_batch_decoder_admit_anchor: not a dynamic decoder (pb_batch_decoder_dynamic)");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_admit_anchor: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(row >= 0 && row < D->B, "pb_batch_decoder_admit_anchor: row %d of %d", row, D->B);
    PB_REQUIRE(cnt >= 0 && base >= 0 && (long long)base + cnt <= D->n_anchor && cnt <= D->bp.plan.S,
               "pb_batch_decoder_admit_anchor: row %d: anchors %d .. %d + %d outside the table's %d rows (the table is pb_batch_decoder_anchor's)", row, base, base,
               cnt, D->n_anchor);
    if (cnt && anchor_check(D, D->anchor_host.data() + (size_t)base * 8, cnt, D->admit_order[row] > 0 ? D->admit_order[row] : 0,
                            D->admit_stop[row] >= 0 ? D->admit_stop[row] : D->sa.pad[0], "pb_batch_decoder_admit_anchor", row)) return -1;
    D->admit_anchor[row] = cnt > 0 ? base : -1; D->admit_nanchor[row] = cnt;
    return 0;
}

// The counter of a rewound row: with the pb_batch_decoder_seek that moved it back, the number of anchors the HOST has placed up to the
// position it seeks to. In decoder-stream order behind that seek's stores; the steps enqueued next read it.
extern "C" int pb_batch_decoder_seek_anchor(void* dec, int32_t row, int32_t placed) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && D->sampler, "pb_batch_decoder_seek_anchor: pb_batch_decoder_sampler_init first");
    PB_REQUIRE(row >= 0 && row < D->B, "pb_batch_decoder_seek_anchor: row %d of %d", row, D->B);
    PB_REQUIRE(placed >= 0 && placed <= D->anchor.cnt[row], "pb_batch_decoder_seek_anchor: row %d: %d anchors placed of %d", row, placed, D->anchor.cnt[row]);
    PB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)&D->st->aplaced[row], placed, 1, D->stream));
    return 0;
}

// The rows' counters after draining what is enqueued: out = B host ints.
extern "C" int pb_batch_decoder_anchors_placed(void* dec, int32_t* out) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D && out, "pb_batch_decoder_anchors_placed: null argument");
    PB_REQUIRE(D->sampler, "pb_batch_decoder_anchors_placed: pb_batch_decoder_sampler_init first");
    PB_CHECK_HIP(hipStreamSynchronize(D->stream));
    int got[BMAX];
    PB_CHECK_HIP(hipMemcpy(got, D->st->aplaced, sizeof(int) * BMAX, hipMemcpyDeviceToHost));
    for (int b = 0; b < D->B; ++b) out[b] = D->anchor.cnt[b] > 0 ? got[b] : 0;
    return 0;
}

// `caller_stream` waits for everything enqueued on the decoder's stream so far (an event; the host does not wait).
extern "C" int pb_batch_decoder_fence(void* dec, void* caller_stream) {
    Decoder* D = (Decoder*)dec;
    PB_REQUIRE(D, "pb_batch_decoder_fence: null decoder");
    PB_CHECK_HIP(hipEventRecord(D->ev_fence, D->stream));
    PB_CHECK_HIP(hipStreamWaitEvent((hipStream_t)caller_stream, D->ev_fence, 0));
    return 0;
}

extern "C" int pb_batch_decoder_launches(void* dec) { return dec ? ((Decoder*)dec)->launches : 0; }
extern "C" int pb_batch_decoder_graph(void* dec) {
    const Decoder* D = (const Decoder*)dec;
    return D && D->use_graph && (D->exec[G_STEP] || D->exec[G_RUN]) ? 1 : 0;
}
