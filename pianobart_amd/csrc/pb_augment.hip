// On-device Octuple augmentation in front of the corruption: every piece of a batch is shifted AS A WHOLE along up to three
// axes -- a = 0 pitch (head 3, semitones), a = 1 velocity (head 5, bins), a = 2 tempo (head 7, bins) -- by one amount per axis, drawn
// uniformly from the request [lo, hi] clamped by the piece's own extremes and the axis bounds, so that no note is clipped or wrapped.
// An axis is described by two host-built tables: coord[a][id] = the id's coordinate (>= 0) or -1 (specials, percussion pitches: never
// touched) and its inverse id_at[a][c]. Integer work only; equal inputs and seed give equal bytes.
//
// One 256-thread workgroup per piece. The six tables (at most 13 KB) are staged once in LDS. Pass 1 reads the piece's 16-byte rows and
// reduces (max c, max -c) per axis: registers, then the wave butterfly of pb_common.h on integers, then 4 partials through LDS. One
// thread clamps and draws the three axes (Philox counter (0, piece, axis, 0xA06)); a barrier; pass 2 re-reads the rows (the piece is at most
// 1 MB and was just read: it sits in L2), maps the three heads through LDS and stores. A row is read and written by the same lane in
// pass 2, after every lane's pass-1 reads, so out == ids is allowed. Plain vector loads and stores; no atomics.
#include "pb_common.h"
#include "pb_api_internal.h"

namespace {

constexpr int AT = 256, HMAX = 1088, TAB = 3 * HMAX;          // threads, ids of the widest head (ops.HEAD_MAX), int16 of one table set
constexpr int NONE = -(1 << 20);                              // "no shiftable id seen" in a max reduction
struct AugAxis { int lo, hi, blo, bhi, ncoord; uint32_t thresh; };
struct AugArgs {
    const int16_t* ids; int16_t* out; int32_t* shifts; const int16_t* coord; const int16_t* id_at;
    int B, S; uint32_t seed_lo, seed_hi; AugAxis ax[3];
};

#define PB_DPP_I(v, ctrl) __builtin_amdgcn_update_dpp(0, (v), (ctrl), 0xf, 0xf, true)
__device__ __forceinline__ int wave_max_i(int v) {          // wave_max of pb_common.h on int32
    v = max(v, PB_DPP_I(v, 0xb1));
    v = max(v, PB_DPP_I(v, 0x4e));
    v = max(v, PB_DPP_I(v, 0x141));
    v = max(v, PB_DPP_I(v, 0x140));
    auto a = __builtin_amdgcn_permlane16_swap((uint32_t)v, (uint32_t)v, false, false);
    v = max((int)a[0], (int)a[1]);
    auto b = __builtin_amdgcn_permlane32_swap((uint32_t)v, (uint32_t)v, false, false);
    return max((int)b[0], (int)b[1]);
}

// the ids of heads 3, 5 and 7 are the high halves of words 1, 2 and 3 of a row
__device__ __forceinline__ uint32_t axis_id(const uint4& r, int a) { return (a == 0 ? r.y : a == 1 ? r.z : r.w) >> 16; }

__global__ __launch_bounds__(AT) void augment_kernel(const AugArgs p) {
    __shared__ __attribute__((aligned(16))) int16_t coord[TAB];
    __shared__ __attribute__((aligned(16))) int16_t id_at[TAB];
    __shared__ int part[AT / PB_WAVE][6];
    __shared__ int shift[3];
    const int b = blockIdx.x, t = threadIdx.x, S = p.S;
    const int16_t* in = p.ids + (size_t)b * S * 8;
    int16_t* out = p.out + (size_t)b * S * 8;
    for (int i = t; i < TAB / 8; i += AT) {
        reinterpret_cast<uint4*>(coord)[i] = reinterpret_cast<const uint4*>(p.coord)[i];
        reinterpret_cast<uint4*>(id_at)[i] = reinterpret_cast<const uint4*>(p.id_at)[i];
    }
    __syncthreads();
    // coordinate of an id on axis a, or -1: ids and coordinates outside the tables are "not shiftable" (the tables are the caller's)
    auto coord_of = [&](int a, uint32_t id) {
        const int c = id < (uint32_t)HMAX ? (int)coord[a * HMAX + id] : -1;
        return c < p.ax[a].ncoord ? c : -1;
    };

    // ---- pass 1: the piece's extremes per axis
    int hi[3] = {NONE, NONE, NONE}, nlo[3] = {NONE, NONE, NONE};      // max c and max -c
#pragma unroll 4
    for (int i = t; i < S; i += AT) {
        const uint4 r = *reinterpret_cast<const uint4*>(in + (size_t)i * 8);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int c = coord_of(a, axis_id(r, a));
            if (c >= 0) { hi[a] = max(hi[a], c); nlo[a] = max(nlo[a], -c); }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { hi[a] = wave_max_i(hi[a]); nlo[a] = wave_max_i(nlo[a]); }
    if ((t & (PB_WAVE - 1)) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[t / PB_WAVE][2 * a] = hi[a]; part[t / PB_WAVE][2 * a + 1] = nlo[a]; }
    }
    __syncthreads();

    // ---- the draw: one thread decides the three axes
    if (t == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const AugAxis ax = p.ax[a];
            int cmax = NONE, ncmin = NONE;
            for (int w = 0; w < AT / PB_WAVE; ++w) { cmax = max(cmax, part[w][2 * a]); ncmin = max(ncmin, part[w][2 * a + 1]); }
            int s = 0;
            if (cmax >= 0) {
                const int flo = max(ax.lo, ax.blo + ncmin), fhi = min(ax.hi, ax.bhi - cmax);
                if (flo <= 0 && fhi >= 0) {                       // else the piece lies outside the bounds, or fills them
                    const uint4 r = philox4x32(0u, (uint32_t)b, (uint32_t)a, 0xA06u, p.seed_lo, p.seed_hi);
                    s = flo + (int)__umulhi(r.x, (uint32_t)(fhi - flo + 1));
                    if (ax.thresh != 0xFFFFFFFFu && r.y >= ax.thresh) s = 0;
                }
            }
            shift[a] = s;
            p.shifts[b * 3 + a] = s;
        }
    }
    __syncthreads();

    // ---- pass 2: apply
    const int s0 = shift[0], s1 = shift[1], s2 = shift[2];
#pragma unroll 4
    for (int i = t; i < S; i += AT) {
        uint4 r = *reinterpret_cast<const uint4*>(in + (size_t)i * 8);
        const int c0 = coord_of(0, r.y >> 16), c1 = coord_of(1, r.z >> 16), c2 = coord_of(2, r.w >> 16);
        if (c0 >= 0) r.y = (r.y & 0xffffu) | ((uint32_t)(uint16_t)id_at[c0 + s0] << 16);
        if (c1 >= 0) r.z = (r.z & 0xffffu) | ((uint32_t)(uint16_t)id_at[HMAX + c1 + s1] << 16);
        if (c2 >= 0) r.w = (r.w & 0xffffu) | ((uint32_t)(uint16_t)id_at[2 * HMAX + c2 + s2] << 16);
        *reinterpret_cast<uint4*>(out + (size_t)i * 8) = r;
    }
}

}  // namespace

extern "C" int pb_augment(const int16_t* ids, int16_t* out, int32_t* shifts, int32_t B, int32_t S, const int16_t* coord, const int16_t* id_at,
                          const int32_t* plan, uint64_t seed, void* stream_) {
    PB_REQUIRE(ids && out && shifts && coord && id_at && plan, "pb_augment: NULL argument");
    PB_REQUIRE(B >= 1 && B <= 65535, "pb_augment: B=%d out of range (1..65535)", B);
    PB_REQUIRE(S >= 1 && S <= 65536, "pb_augment: S=%d out of range (1..65536)", S);
    PB_REQUIRE((((uintptr_t)ids | (uintptr_t)out | (uintptr_t)coord | (uintptr_t)id_at) & 15) == 0,
               "pb_augment: ids, out, coord and id_at must be 16-byte aligned");
    const char *i0 = (const char*)ids, *o0 = (const char*)out;
    const size_t bytes = (size_t)B * S * 16;
    PB_REQUIRE(i0 == o0 || i0 + bytes <= o0 || o0 + bytes <= i0, "pb_augment: out overlaps ids partially (out == ids, in place, is allowed)");
    static const char* const axis[3] = {"pitch", "velocity", "tempo"};
    AugArgs a;
    for (int k = 0; k < 3; ++k) {
        const int32_t* q = plan + 6 * k;
        PB_REQUIRE(q[0] <= 0 && q[1] >= 0, "pb_augment: %s: the request %d .. %d must hold lo <= 0 <= hi", axis[k], q[0], q[1]);
        PB_REQUIRE(q[4] >= 1 && q[4] <= HMAX, "pb_augment: %s: ncoord=%d out of range (1..%d)", axis[k], q[4], HMAX);
        PB_REQUIRE(q[2] >= 0 && q[2] <= q[3] && q[3] < q[4], "pb_augment: %s: the bounds %d .. %d must lie in 0 .. ncoord-1 = %d", axis[k], q[2], q[3],
                   q[4] - 1);
        // a request wider than the axis draws what the axis allows: the clamp would cut it anyway (and lo, hi stay far from overflow)
        a.ax[k].lo = q[0] < -HMAX ? -HMAX : q[0]; a.ax[k].hi = q[1] > HMAX ? HMAX : q[1];
        a.ax[k].blo = q[2]; a.ax[k].bhi = q[3]; a.ax[k].ncoord = q[4]; a.ax[k].thresh = (uint32_t)q[5];
    }
    a.ids = ids; a.out = out; a.shifts = shifts; a.coord = coord; a.id_at = id_at; a.B = B; a.S = S;
    a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(augment_kernel, dim3(B), dim3(AT), 0, (hipStream_t)stream_, a);
    PB_LAUNCH_CHECK();
    return 0;
}
