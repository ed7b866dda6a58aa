// K17: gradient accumulation over micro-batches (Engine.loss_and_grads(micro=(i, K))): dst = src or dst += src over a flat f32 range.
// Pure streaming (12 bytes per element in add mode: two reads and a write), f32x4 per lane, 64-bit indexing, grid-stride, grid sized
// from n and capped like the optimizer's row kernels. No atomics: every element is written by exactly one lane, one f32 addition per
// element, so equal inputs give equal bits.
// The engine calls it on whole flat buffers and on slot ranges [lo, hi) of them, whose offsets need not be multiples of 4 elements: the
// elements in front of dst's first 16-byte boundary and the (< 4) behind the last whole vector are done by scalar accesses; when src
// does not reach a 16-byte boundary at the same element (the two pointers are offset differently) the whole range goes scalar.
#include "pb_common.h"
#include "pb_api_internal.h"
#include <algorithm>

namespace {

constexpr int ACC_BLOCKS = 2048, ACC_THREADS = 256;

// [0, head) scalar | [head, head + 4 n4) as n4 vectors (VEC) or scalars | [head + 4 n4, n) scalar
template <bool ADD, bool VEC>
__global__ __launch_bounds__(ACC_THREADS) void accum_kernel(float* __restrict__ dst, const float* __restrict__ src, long n, long head, long n4) {
    const long tid = (long)blockIdx.x * ACC_THREADS + threadIdx.x, stride = (long)gridDim.x * ACC_THREADS;
    float* d = dst + head;
    const float* s = src + head;
    if (VEC) {
        for (long i = tid; i < n4; i += stride) {
            f32x4 v = *reinterpret_cast<const f32x4*>(s + 4 * i);
            if (ADD) v = *reinterpret_cast<const f32x4*>(d + 4 * i) + v;
            *reinterpret_cast<f32x4*>(d + 4 * i) = v;
        }
    } else {
        for (long i = tid; i < 4 * n4; i += stride) d[i] = ADD ? d[i] + s[i] : s[i];
    }
    if (blockIdx.x == 0) {
        const long body_end = head + 4 * n4;
        long i = -1;
        if ((long)threadIdx.x < head) i = threadIdx.x;                                             // head: lanes 0 .. 2
        else if (threadIdx.x >= 64 && body_end + (threadIdx.x - 64) < n) i = body_end + (threadIdx.x - 64);    // tail: lanes 64 .. 66
        if (i >= 0) dst[i] = ADD ? dst[i] + src[i] : src[i];
    }
}

}  // namespace

extern "C" int pb_accum_f32(float* dst, const float* src, int64_t n, int32_t add, void* stream_) {
    if (n <= 0) return 0;
    PB_REQUIRE(dst && src && ((uintptr_t)dst % 4 == 0) && ((uintptr_t)src % 4 == 0), "pb_accum_f32: dst and src must be non-NULL f32 pointers");
    PB_REQUIRE(add == 0 || add == 1, "pb_accum_f32: add must be 0 or 1 (got %d)", (int)add);
    const long head = std::min<long>((long)n, (long)(((16 - ((uintptr_t)dst & 15)) & 15) / 4));
    const long n4 = ((long)n - head) >> 2;
    const bool vec = ((uintptr_t)(src + head) & 15) == 0;
    const long items = vec ? n4 : 4 * n4;
    const int grid = (int)std::max(1L, std::min((long)ACC_BLOCKS, (items + ACC_THREADS - 1) / ACC_THREADS));
    hipStream_t stream = (hipStream_t)stream_;
    if (add) {
        if (vec) hipLaunchKernelGGL((accum_kernel<true, true>), dim3(grid), dim3(ACC_THREADS), 0, stream, dst, src, (long)n, head, n4);
        else hipLaunchKernelGGL((accum_kernel<true, false>), dim3(grid), dim3(ACC_THREADS), 0, stream, dst, src, (long)n, head, n4);
    } else {
        if (vec) hipLaunchKernelGGL((accum_kernel<false, true>), dim3(grid), dim3(ACC_THREADS), 0, stream, dst, src, (long)n, head, n4);
        else hipLaunchKernelGGL((accum_kernel<false, false>), dim3(grid), dim3(ACC_THREADS), 0, stream, dst, src, (long)n, head, n4);
    }
    PB_LAUNCH_CHECK();
    return 0;
}
