// The scalar logic of pb_merge.hip's radix select, shared by the kernels and by tools/merge_select_check.cpp (a stand-alone host program that
// runs the four passes serially over edge-case inputs under -fsanitize=address,undefined and compares with a sort).
// A magnitude is a float's bit pattern without its sign: non-negative floats order as unsigned integers. Pass p (0 .. 3) looks at bits
// 31 - 8p .. 24 - 8p of the magnitudes whose higher bits equal `prefix` (under `mask`).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define PB_SEL_FN __host__ __device__ __forceinline__
#else
#define PB_SEL_FN inline
#endif

struct PbSelState {
    unsigned long long k_rem;            // rank of the wanted element among the elements under the prefix (1-based)
    uint32_t prefix, mask;               // bits decided so far and which bits those are
};

PB_SEL_FN uint32_t pb_sel_mag(uint32_t float_bits) { return float_bits & 0x7fffffffu; }
PB_SEL_FN bool pb_sel_nonfinite(uint32_t mag) { return (mag & 0x7f800000u) == 0x7f800000u; }
PB_SEL_FN int pb_sel_shift(int pass) { return 24 - 8 * pass; }
// the bin of pass `pass` that a magnitude falls into, or -1 when its higher bits are not the prefix
PB_SEL_FN int pb_sel_bin(uint32_t mag, uint32_t prefix, uint32_t mask, int pass) {
    return (mag & mask) == prefix ? (int)((mag >> pb_sel_shift(pass)) & 0xffu) : -1;
}
// Bin t holds `mine` elements and the bins 0 .. t hold `incl`: true (for exactly one t while 1 <= k_rem <= the elements under the prefix)
// when the wanted element is in bin t; st then becomes the state of the next pass and st.prefix after pass 3 is the answer's bit pattern.
PB_SEL_FN bool pb_sel_pick(unsigned long long incl, unsigned long long mine, int t, int pass, PbSelState& st) {
    const unsigned long long excl = incl - mine;
    if (!(excl < st.k_rem && st.k_rem <= incl)) return false;
    st.k_rem -= excl;
    st.prefix |= (uint32_t)t << pb_sel_shift(pass);
    st.mask |= 0xffu << pb_sel_shift(pass);
    return true;
}
