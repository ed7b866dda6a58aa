// K18: checkpoint merging on flat f32 parameter vectors (average, task arithmetic, TIES, magnitude / random masking of task vectors):
// the reference's model_merging_methods/merging_methods.py + mask_weights_utils.py as streaming passes. Three kernel families:
//   kth_hist_kernel / kth_pick_kernel   exact k-th smallest magnitude: radix select over the magnitude's bit pattern, 4 x 8 bits
//   tally_kernel                        TIES pass 1: 64-bit counts of the positive and negative summed signs
//   apply_kernel<METHOD>                one fused pass from the pre-trained vector and up to 8 model vectors to the merged vector
// All HBM-bound, f32x4 per lane, grid-stride, <= 2048 workgroups (adamw_kernel's shape). Pointers may be segments of flat buffers: the
// elements in front of the first 16-byte boundary and behind the last whole vector are done by scalar accesses of workgroup 0.
//
// Bit parity with the reference's CPU tensors needs every operation rounded once, in the reference's order. The build contracts
// (-ffp-contract=fast): the backend then fuses a * b + c whatever the source says -- `#pragma clang fp contract(off)` does not reach it, and
// clang's __fadd_rn / __fmul_rn are plain operators -- so build.py compiles THIS file with -ffp-contract=off (FILE_FLAGS), and
// tests/test_merge_cpu.py looks for fused multiply-adds in its code. Masks are applied as the reference applies them, by a
// MULTIPLICATION with 0 or 1 (x * 0 keeps x's sign: a masked -1.5 is -0.0, and -0.0 survives a sum of masked values), never by a select.
#include "pb_common.h"
#include "pb_api_internal.h"
#include "pb_merge_select.h"
#include <algorithm>

namespace {

constexpr int MG_BLOCKS = 2048, MG_THREADS = 256, MG_MAX = PB_MERGE_MAX_MODELS;

__device__ __forceinline__ uint32_t mag_bits(float v) { return pb_sel_mag(__float_as_uint(v)); }

// ---- radix select --------------------------------------------------------------------------------------------------------------
struct KthState {
    unsigned long long hist[4][256];     // pass p counts the elements whose bits above its digit equal the prefix, by digit
    PbSelState sel;
};

__global__ void kth_init_kernel(KthState* st, unsigned long long k) {
    for (int i = threadIdx.x; i < 4 * 256; i += blockDim.x) (&st->hist[0][0])[i] = 0ull;
    if (threadIdx.x == 0) { st->sel.k_rem = k; st->sel.prefix = 0u; st->sel.mask = 0u; }
}

// one element's bin into the workgroup's LDS histogram; the four elements of a lane are merged first (equal digits are the rule in the top pass)
__device__ __forceinline__ void hist_add4(uint32_t* bins, const int (&b)[4]) {
    int c[4] = {b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (c[j] < 0) continue;
        uint32_t cnt = 1;
#pragma unroll
        for (int l = j + 1; l < 4; ++l) if (c[l] == c[j]) { ++cnt; c[l] = -1; }
        atomicAdd(&bins[c[j]], cnt);
    }
}

template <bool VEC>
__global__ __launch_bounds__(MG_THREADS) void kth_hist_kernel(const float* __restrict__ x, const float* __restrict__ base, long n, long head, long n4,
                                                              int pass, KthState* __restrict__ st, int32_t* __restrict__ flags) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t prefix = st->sel.prefix, mask = st->sel.mask;
    bool bad = false;
    auto bin_of = [&](float xv, float bv) -> int {
        const uint32_t u = mag_bits(base ? xv - bv : xv);
        bad |= pb_sel_nonfinite(u);
        return pb_sel_bin(u, prefix, mask, pass);
    };
    const long tid = (long)blockIdx.x * MG_THREADS + threadIdx.x, stride = (long)gridDim.x * MG_THREADS;
    const float* xs = x + head;
    const float* bs = base ? base + head : nullptr;
    if (VEC) {
        for (long i = tid; i < n4; i += stride) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + 4 * i);
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (bs) bv = *reinterpret_cast<const f32x4*>(bs + 4 * i);
            const int b[4] = {bin_of(xv[0], bv[0]), bin_of(xv[1], bv[1]), bin_of(xv[2], bv[2]), bin_of(xv[3], bv[3])};
            // a wave whose 256 elements all fall into one bin (constant tensors, the exponent pass of narrow distributions) adds once
            const int first = __builtin_amdgcn_readfirstlane(b[0]);
            if (first >= 0 && __all(b[0] == first && b[1] == first && b[2] == first && b[3] == first)) {
                const unsigned long long act = __ballot(1);
                if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(&bins[first], 4u * (uint32_t)__popcll(act));
            } else {
                hist_add4(bins, b);
            }
        }
    } else {
        for (long i = tid; i < 4 * n4; i += stride) {
            const int b = bin_of(xs[i], bs ? bs[i] : 0.f);
            if (b >= 0) atomicAdd(&bins[b], 1u);
        }
    }
    if (blockIdx.x == 0) {
        const long body_end = head + 4 * n4;
        long i = -1;
        if ((long)threadIdx.x < head) i = threadIdx.x;                                             // head: lanes 0 .. 2
        else if (threadIdx.x >= 64 && body_end + (threadIdx.x - 64) < n) i = body_end + (threadIdx.x - 64);    // tail: lanes 64 .. 66
        if (i >= 0) {
            const int b = bin_of(x[i], base ? base[i] : 0.f);
            if (b >= 0) atomicAdd(&bins[b], 1u);
        }
    }
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(&st->hist[pass][threadIdx.x], (unsigned long long)bins[threadIdx.x]);
    if (bad && pass == 0) atomicOr(flags, 1);
}

// one workgroup of 256: the first bin whose running count reaches k_rem holds the wanted element
__global__ __launch_bounds__(256) void kth_pick_kernel(KthState* __restrict__ st, int pass, float* __restrict__ kth_out) {
    __shared__ unsigned long long scan[256];
    const int t = threadIdx.x;
    const unsigned long long mine = st->hist[pass][t];
    PbSelState sel = st->sel;
    scan[t] = mine;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned long long add = t >= o ? scan[t - o] : 0ull;
        __syncthreads();
        scan[t] += add;
        __syncthreads();
    }
    if (pb_sel_pick(scan[t], mine, t, pass, sel)) {    // exactly one thread
        st->sel = sel;
        if (pass == 3) *kth_out = __uint_as_float(sel.prefix);
    }
}

// ---- the per-element arithmetic --------------------------------------------------------------------------------------------------
struct MergeArgs {
    const float* pre; float* out;
    const float* model[MG_MAX];
    const float* thresh[MG_MAX];
    const long long* tally;
    long n, head, n4, g0;
    uint32_t seed_lo, seed_hi;
    unsigned long long drop_thresh[MG_MAX];
    float rescale[MG_MAX];
    int mask_kind[MG_MAX];
    int n_models, format, model_base;
    float lambda;
};

__device__ __forceinline__ uint32_t pick_word(const uint4& r, int w) { return w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w; }

// the mask words of elements g .. g + 3 of model m (g need not be a multiple of 4: then two draws)
__device__ __forceinline__ void mask_words4(const MergeArgs& a, int m, long g, uint32_t (&w)[4]) {
    const uint32_t c = (uint32_t)(g >> 2);
    const int r = (int)(g & 3);                        // the same for every vector of a launch
    const uint4 lo = philox4x32(c, (uint32_t)(a.model_base + m), 0x4D455247u, 0u, a.seed_lo, a.seed_hi);
    if (r == 0) { w[0] = lo.x; w[1] = lo.y; w[2] = lo.z; w[3] = lo.w; return; }
    const uint4 hi = philox4x32(c + 1u, (uint32_t)(a.model_base + m), 0x4D455247u, 0u, a.seed_lo, a.seed_hi);
    if (r == 1) { w[0] = lo.y; w[1] = lo.z; w[2] = lo.w; w[3] = hi.x; }
    else if (r == 2) { w[0] = lo.z; w[1] = lo.w; w[2] = hi.x; w[3] = hi.y; }
    else { w[0] = lo.w; w[1] = hi.x; w[2] = hi.y; w[3] = hi.z; }
}
__device__ __forceinline__ uint32_t mask_word1(const MergeArgs& a, int m, long g) {
    return pick_word(philox4x32((uint32_t)(g >> 2), (uint32_t)(a.model_base + m), 0x4D455247u, 0u, a.seed_lo, a.seed_hi), (int)(g & 3));
}

// W_m: the model's value after its mask (see pb_merge_apply in the header)
__device__ __forceinline__ float masked_value(const MergeArgs& a, int m, float p, float f, float thr, uint32_t word) {
    const int kind = a.mask_kind[m];
    if (kind == PB_MERGE_MASK_NONE) return f;
    float x = a.format == PB_MERGE_DELTA ? f - p : f;
    const bool drop = kind == PB_MERGE_MASK_MAGNITUDE ? mag_bits(x) <= __float_as_uint(thr) : (unsigned long long)word < a.drop_thresh[m];
    x = x * (drop ? 0.0f : 1.0f);
    if (a.rescale[m] != 1.0f) x = x / a.rescale[m];
    return a.format == PB_MERGE_DELTA ? p + x : x;
}

// T_m of TIES and the summed sign's class: +1, -1 or 0
__device__ __forceinline__ int ties_trim(const MergeArgs& a, float p, const float (&w)[MG_MAX], const float (&thr)[MG_MAX], float (&t)[MG_MAX]) {
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < MG_MAX; ++m) {
        if (m < a.n_models) {
            const float d = w[m] - p;
            t[m] = d * (mag_bits(d) >= __float_as_uint(thr[m]) ? 1.0f : 0.0f);
            s = s + t[m];
        }
    }
    return (s > 0.f) - (s < 0.f);
}

template <int METHOD>
__device__ __forceinline__ float merge_one(const MergeArgs& a, float p, const float (&f)[MG_MAX], const float (&thr)[MG_MAX], const uint32_t (&word)[MG_MAX], int majority) {
    float w[MG_MAX];
#pragma unroll
    for (int m = 0; m < MG_MAX; ++m) if (m < a.n_models) w[m] = METHOD == PB_MERGE_TIES ? f[m] : masked_value(a, m, p, f[m], thr[m], word[m]);
    if (METHOD == PB_MERGE_MASKED) return w[0];
    if (METHOD == PB_MERGE_AVERAGE) {
        float s = 0.0f;                                // torch's sum starts its accumulator at +0: values that are all -0.0 average to +0.0
#pragma unroll
        for (int m = 0; m < MG_MAX; ++m) if (m < a.n_models) s = s + w[m];
        return s / (float)a.n_models;
    }
    if (METHOD == PB_MERGE_TASK) {
        float s = w[0] - p;
#pragma unroll
        for (int m = 1; m < MG_MAX; ++m) if (m < a.n_models) s = s + (w[m] - p);
        return p + a.lambda * s;
    }
    float t[MG_MAX];
    int sg = ties_trim(a, p, w, thr, t);
    if (sg == 0) sg = majority;
    float s = 0.f;
    int cnt = 0;
#pragma unroll
    for (int m = 0; m < MG_MAX; ++m) {
        if (m < a.n_models) {
            const bool keep = (sg > 0 && t[m] > 0.f) || (sg < 0 && t[m] < 0.f);
            const float kv = t[m] * (keep ? 1.0f : 0.0f);
            cnt += kv != 0.f;
            s = s + kv;
        }
    }
    return p + a.lambda * (s / (float)max(cnt, 1));
}

// the device thresholds of the launch: bit pattern 0 (every magnitude >= it; a magnitude mask never uses a NULL threshold)
__device__ __forceinline__ void load_thresh(const MergeArgs& a, float (&thr)[MG_MAX]) {
#pragma unroll
    for (int m = 0; m < MG_MAX; ++m) thr[m] = (m < a.n_models && a.thresh[m]) ? a.thresh[m][0] : 0.f;
}

template <int METHOD, bool VEC>
__global__ __launch_bounds__(MG_THREADS) void apply_kernel(const MergeArgs a) {
    float thr[MG_MAX];
    load_thresh(a, thr);
    int majority = 0;
    if (METHOD == PB_MERGE_TIES) { const long long d = a.tally[0] - a.tally[1]; majority = (d > 0) - (d < 0); }
    const long tid = (long)blockIdx.x * MG_THREADS + threadIdx.x, stride = (long)gridDim.x * MG_THREADS;
    if (VEC) {
        for (long i = tid; i < a.n4; i += stride) {
            const long e = a.head + 4 * i;
            const f32x4 pv = *reinterpret_cast<const f32x4*>(a.pre + e);
            f32x4 fv[MG_MAX];
            uint32_t wd[MG_MAX][4];
#pragma unroll
            for (int m = 0; m < MG_MAX; ++m) {
                if (m < a.n_models) {
                    fv[m] = *reinterpret_cast<const f32x4*>(a.model[m] + e);
                    if (METHOD != PB_MERGE_TIES && a.mask_kind[m] == PB_MERGE_MASK_RANDOM) mask_words4(a, m, a.g0 + e, wd[m]);
                    else { wd[m][0] = wd[m][1] = wd[m][2] = wd[m][3] = 0u; }
                }
            }
            f32x4 ov;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float f[MG_MAX];
                uint32_t word[MG_MAX];
#pragma unroll
                for (int m = 0; m < MG_MAX; ++m) { f[m] = m < a.n_models ? fv[m][j] : 0.f; word[m] = m < a.n_models ? wd[m][j] : 0u; }
                ov[j] = merge_one<METHOD>(a, pv[j], f, thr, word, majority);
            }
            *reinterpret_cast<f32x4*>(a.out + e) = ov;
        }
    }
    // scalar elements: the whole body when the pointers are offset differently, else head and tail (workgroup 0)
    auto scalar = [&](long e) {
        float f[MG_MAX];
        uint32_t word[MG_MAX];
#pragma unroll
        for (int m = 0; m < MG_MAX; ++m) {
            f[m] = 0.f; word[m] = 0u;
            if (m < a.n_models) {
                f[m] = a.model[m][e];
                if (METHOD != PB_MERGE_TIES && a.mask_kind[m] == PB_MERGE_MASK_RANDOM) word[m] = mask_word1(a, m, a.g0 + e);
            }
        }
        a.out[e] = merge_one<METHOD>(a, a.pre[e], f, thr, word, majority);
    };
    if (!VEC) for (long i = tid; i < 4 * a.n4; i += stride) scalar(a.head + i);
    if (blockIdx.x == 0) {
        const long body_end = a.head + 4 * a.n4;
        if ((long)threadIdx.x < a.head) scalar(threadIdx.x);
        else if (threadIdx.x >= 64 && body_end + (threadIdx.x - 64) < a.n) scalar(body_end + (threadIdx.x - 64));
    }
}

template <bool VEC>
__global__ __launch_bounds__(MG_THREADS) void tally_kernel(const MergeArgs a, unsigned long long* __restrict__ tally) {
    __shared__ unsigned int red[2];
    if (threadIdx.x < 2) red[threadIdx.x] = 0u;
    __syncthreads();
    float thr[MG_MAX];
    load_thresh(a, thr);
    unsigned int pos = 0, neg = 0;                      // a lane sees < 2^32 elements
    auto one = [&](float p, const float (&f)[MG_MAX]) {
        float t[MG_MAX];
        const int sg = ties_trim(a, p, f, thr, t);
        pos += sg > 0; neg += sg < 0;
    };
    auto scalar = [&](long e) {
        float f[MG_MAX];
#pragma unroll
        for (int m = 0; m < MG_MAX; ++m) f[m] = m < a.n_models ? a.model[m][e] : 0.f;
        one(a.pre[e], f);
    };
    const long tid = (long)blockIdx.x * MG_THREADS + threadIdx.x, stride = (long)gridDim.x * MG_THREADS;
    if (VEC) {
        for (long i = tid; i < a.n4; i += stride) {
            const long e = a.head + 4 * i;
            const f32x4 pv = *reinterpret_cast<const f32x4*>(a.pre + e);
            f32x4 fv[MG_MAX];
#pragma unroll
            for (int m = 0; m < MG_MAX; ++m) if (m < a.n_models) fv[m] = *reinterpret_cast<const f32x4*>(a.model[m] + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float f[MG_MAX];
#pragma unroll
                for (int m = 0; m < MG_MAX; ++m) f[m] = m < a.n_models ? fv[m][j] : 0.f;
                one(pv[j], f);
            }
        }
    } else {
        for (long i = tid; i < 4 * a.n4; i += stride) scalar(a.head + i);
    }
    if (blockIdx.x == 0) {
        const long body_end = a.head + 4 * a.n4;
        if ((long)threadIdx.x < a.head) scalar(threadIdx.x);
        else if (threadIdx.x >= 64 && body_end + (threadIdx.x - 64) < a.n) scalar(body_end + (threadIdx.x - 64));
    }
    if (pos) atomicAdd(&red[0], pos);                   // 32 bits hold a workgroup's share: n <= 2^34 over 2048 workgroups
    if (neg) atomicAdd(&red[1], neg);
    __syncthreads();
    if (threadIdx.x < 2 && red[threadIdx.x]) atomicAdd(&tally[threadIdx.x], (unsigned long long)red[threadIdx.x]);
}

// [0, head) scalar | n4 vectors | tail scalar: head = elements in front of `lead`'s first 16-byte boundary; vec = every other pointer reaches one there too
void split_range(const void* lead, long n, long& head, long& n4) {
    head = std::min<long>(n, (long)(((16 - ((uintptr_t)lead & 15)) & 15) / 4));
    n4 = (n - head) >> 2;
}
bool aligned_at(const float* p, long head) { return (((uintptr_t)(p + head)) & 15) == 0; }
int grid_for(long items) { return (int)std::max(1L, std::min((long)MG_BLOCKS, (items + MG_THREADS - 1) / MG_THREADS)); }

// checks the descriptor fields both entry points read and fills the kernel's arguments; returns 0, or < 0 with the error set
int fill_args(const pb_merge_desc* d, const char* who, bool tally_only, MergeArgs& a, bool& vec) {
    PB_REQUIRE(d, "%s: NULL descriptor", who);
    PB_REQUIRE(d->n >= 0 && d->g0 >= 0 && d->n + d->g0 <= (1ll << 34), "%s: n = %lld, g0 = %lld out of range (the mask counter is element >> 2 in 32 bits)", who,
               (long long)d->n, (long long)d->g0);
    const int lo = (!tally_only && d->method == PB_MERGE_MASKED) ? 1 : 2, hi = lo == 1 ? 1 : MG_MAX;
    PB_REQUIRE(d->n_models >= lo && d->n_models <= hi, "%s: n_models = %d (this method takes %d .. %d models)", who, (int)d->n_models, lo, hi);
    PB_REQUIRE(d->pre && ((uintptr_t)d->pre % 4 == 0), "%s: pre must be a non-NULL f32 pointer", who);
    PB_REQUIRE(d->model_base >= 0 && d->model_base + d->n_models <= MG_MAX, "%s: model_base = %d with %d models", who, (int)d->model_base, (int)d->n_models);
    a = MergeArgs{};
    a.pre = d->pre; a.out = d->out; a.tally = (const long long*)d->tally;
    a.n = (long)d->n; a.g0 = (long)d->g0;
    a.seed_lo = (uint32_t)(d->seed & 0xffffffffu); a.seed_hi = (uint32_t)(d->seed >> 32);
    a.n_models = d->n_models; a.format = d->format; a.lambda = d->lambda; a.model_base = d->model_base;
    split_range(tally_only ? (const void*)d->pre : (const void*)d->out, a.n, a.head, a.n4);
    vec = aligned_at(d->pre, a.head);
    for (int m = 0; m < d->n_models; ++m) {
        PB_REQUIRE(d->model[m] && ((uintptr_t)d->model[m] % 4 == 0), "%s: model[%d] must be a non-NULL f32 pointer", who, m);
        PB_REQUIRE(tally_only || d->model[m] != d->out, "%s: out aliases model[%d]", who, m);
        a.model[m] = d->model[m]; a.thresh[m] = d->thresh[m];
        a.drop_thresh[m] = d->drop_thresh[m]; a.rescale[m] = d->rescale[m]; a.mask_kind[m] = d->mask_kind[m];
        vec = vec && aligned_at(d->model[m], a.head);
    }
    return 0;
}

}  // namespace

extern "C" int64_t pb_merge_desc_bytes(void) { return (int64_t)sizeof(pb_merge_desc); }
extern "C" int64_t pb_merge_kth_ws_bytes(void) { return (int64_t)sizeof(KthState); }

extern "C" int pb_merge_kth_abs(const float* x, const float* base, int64_t n, int64_t k, float* kth_out, int32_t* flags_out, void* ws, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    PB_REQUIRE(x && kth_out && flags_out && ws, "pb_merge_kth_abs: x, kth_out, flags_out and ws are required");
    PB_REQUIRE(((uintptr_t)x % 4 == 0) && ((uintptr_t)base % 4 == 0) && ((uintptr_t)ws % 8 == 0), "pb_merge_kth_abs: x / base need 4-byte, ws 8-byte alignment");
    PB_REQUIRE(n >= 1 && k >= 1 && k <= n, "pb_merge_kth_abs: need 1 <= k <= n (got k = %lld, n = %lld)", (long long)k, (long long)n);
    KthState* st = (KthState*)ws;
    long head, n4;
    split_range(x, (long)n, head, n4);
    const bool vec = !base || aligned_at(base, head);
    const int grid = grid_for(vec ? n4 : 4 * n4);
    hipLaunchKernelGGL(kth_init_kernel, dim3(1), dim3(256), 0, stream, st, (unsigned long long)k);
    PB_LAUNCH_CHECK();
    for (int pass = 0; pass < 4; ++pass) {
        if (vec) hipLaunchKernelGGL(kth_hist_kernel<true>, dim3(grid), dim3(MG_THREADS), 0, stream, x, base, (long)n, head, n4, pass, st, flags_out);
        else hipLaunchKernelGGL(kth_hist_kernel<false>, dim3(grid), dim3(MG_THREADS), 0, stream, x, base, (long)n, head, n4, pass, st, flags_out);
        PB_LAUNCH_CHECK();
        hipLaunchKernelGGL(kth_pick_kernel, dim3(1), dim3(256), 0, stream, st, pass, kth_out);
        PB_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int pb_merge_sign_tally(const pb_merge_desc* d, void* stream_) {
    MergeArgs a;
    bool vec;
    if (int rc = fill_args(d, "pb_merge_sign_tally", true, a, vec)) return rc;
    PB_REQUIRE(d->tally && ((uintptr_t)d->tally % 8 == 0), "pb_merge_sign_tally: tally must be a device int64[2]");
    if (a.n == 0) return 0;
    const int grid = grid_for(vec ? a.n4 : 4 * a.n4);
    if (vec) hipLaunchKernelGGL(tally_kernel<true>, dim3(grid), dim3(MG_THREADS), 0, (hipStream_t)stream_, a, (unsigned long long*)d->tally);
    else hipLaunchKernelGGL(tally_kernel<false>, dim3(grid), dim3(MG_THREADS), 0, (hipStream_t)stream_, a, (unsigned long long*)d->tally);
    PB_LAUNCH_CHECK();
    return 0;
}

template <int METHOD>
static int launch_apply(const MergeArgs& a, bool vec, hipStream_t stream) {
    const int grid = grid_for(vec ? a.n4 : 4 * a.n4);
    if (vec) hipLaunchKernelGGL((apply_kernel<METHOD, true>), dim3(grid), dim3(MG_THREADS), 0, stream, a);
    else hipLaunchKernelGGL((apply_kernel<METHOD, false>), dim3(grid), dim3(MG_THREADS), 0, stream, a);
    PB_LAUNCH_CHECK();
    return 0;
}

extern "C" int pb_merge_apply(const pb_merge_desc* d, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    MergeArgs a;
    bool vec;
    PB_REQUIRE(d && d->method >= PB_MERGE_AVERAGE && d->method <= PB_MERGE_MASKED, "pb_merge_apply: unknown method %d", d ? (int)d->method : -1);
    if (int rc = fill_args(d, "pb_merge_apply", false, a, vec)) return rc;
    PB_REQUIRE(d->out && ((uintptr_t)d->out % 4 == 0) && d->out != d->pre, "pb_merge_apply: out must be a non-NULL f32 pointer that is not pre");
    PB_REQUIRE(d->format == PB_MERGE_DELTA || d->format == PB_MERGE_FINETUNED, "pb_merge_apply: unknown format %d", (int)d->format);
    for (int m = 0; m < d->n_models; ++m) {
        const int kind = d->mask_kind[m];
        PB_REQUIRE(kind >= PB_MERGE_MASK_NONE && kind <= PB_MERGE_MASK_RANDOM, "pb_merge_apply: unknown mask kind %d of model %d", kind, m);
        PB_REQUIRE(d->method != PB_MERGE_TIES || kind == PB_MERGE_MASK_NONE, "pb_merge_apply: PB_MERGE_TIES takes unmasked models (model %d has mask kind %d)", m, kind);
        PB_REQUIRE(kind != PB_MERGE_MASK_MAGNITUDE || d->thresh[m], "pb_merge_apply: model %d has a magnitude mask without a threshold", m);
        PB_REQUIRE(kind == PB_MERGE_MASK_NONE || d->rescale[m] > 0.f, "pb_merge_apply: rescale[%d] must be > 0 (1 = none)", m);
        if (kind == PB_MERGE_MASK_NONE) a.rescale[m] = 1.0f;
    }
    PB_REQUIRE(d->method != PB_MERGE_TIES || (d->tally && ((uintptr_t)d->tally % 8 == 0)), "pb_merge_apply: PB_MERGE_TIES needs the tally of pb_merge_sign_tally");
    if (a.n == 0) return 0;
    switch (d->method) {
        case PB_MERGE_AVERAGE: return launch_apply<PB_MERGE_AVERAGE>(a, vec, stream);
        case PB_MERGE_TASK: return launch_apply<PB_MERGE_TASK>(a, vec, stream);
        case PB_MERGE_TIES: return launch_apply<PB_MERGE_TIES>(a, vec, stream);
        default: return launch_apply<PB_MERGE_MASKED>(a, vec, stream);
    }
}
