// Stand-alone host check of the radix select of csrc/pb_merge.hip: the scalar logic the kernels share (csrc/pb_merge_select.h: bin of a
// magnitude, the pick that narrows the prefix) run serially -- four histogram passes of 256 64-bit bins, the inclusive scan, the pick --
// over the edge-case inputs of tests/test_merge_gpu.py, against std::sort. Built with -fsanitize=address,undefined and run on the CPU
// (tests/test_merge_cpu.py); no GPU code is involved. Prints one line per input kind; exit status 1 on the first mismatch.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../pianobart_amd/csrc/pb_merge_select.h"

static uint32_t bits_of(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }
static float float_of(uint32_t u) { float v; std::memcpy(&v, &u, 4); return v; }

// the k-th smallest magnitude's bit pattern as the kernels find it; *nonfinite as their flag
static uint32_t select_kth(const std::vector<float>& x, unsigned long long k, bool* nonfinite) {
    PbSelState st = {k, 0u, 0u};
    *nonfinite = false;
    for (int pass = 0; pass < 4; ++pass) {
        std::vector<unsigned long long> hist(256, 0ull);
        for (float v : x) {
            const uint32_t mag = pb_sel_mag(bits_of(v));
            if (pass == 0 && pb_sel_nonfinite(mag)) *nonfinite = true;
            const int b = pb_sel_bin(mag, st.prefix, st.mask, pass);
            if (b >= 0) ++hist[(size_t)b];
        }
        unsigned long long incl = 0;
        int picked = 0;
        const PbSelState before = st;
        for (int t = 0; t < 256; ++t) {            // every "thread" starts from the state before the pass, as in the kernel
            incl += hist[(size_t)t];
            PbSelState mine = before;
            if (pb_sel_pick(incl, hist[(size_t)t], t, pass, mine)) { st = mine; ++picked; }
        }
        if (picked != 1) { std::printf("pass %d: %d bins picked\n", pass, picked); return 0xffffffffu; }
    }
    return st.prefix;
}

static std::vector<float> make(const std::string& kind, size_t n, std::mt19937& rng) {
    std::vector<float> x(n);
    std::normal_distribution<float> normal(0.f, 1.f);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t sign = (rng() & 1u) << 31;
        if (kind == "normal") x[i] = 0.02f * normal(rng);
        else if (kind == "equal") x[i] = 0.375f;
        else if (kind == "zeros") x[i] = i % 4 == 0 ? -0.0f : i % 2 == 0 ? 0.0f : normal(rng);
        else if (kind == "pairs") x[i] = i % 2 == 0 ? normal(rng) : -x[i - 1];
        else if (kind == "denormal") x[i] = float_of((1u + rng() % ((1u << 23) - 1u)) | sign);
        else x[i] = float_of(0x3C123400u | (rng() & 0xffu) | sign);          // top24: the fourth pass decides
    }
    return x;
}

int main() {
    std::mt19937 rng(15);
    const size_t sizes[] = {1, 3, 255, 256, 257, 4099, (1u << 16) + 5};
    const char* kinds[] = {"normal", "equal", "zeros", "pairs", "denormal", "top24"};
    for (const char* kind : kinds) {
        size_t checked = 0;
        for (size_t n : sizes) {
            const std::vector<float> x = make(kind, n, rng);
            std::vector<uint32_t> mags(n);
            for (size_t i = 0; i < n; ++i) mags[i] = pb_sel_mag(bits_of(x[i]));
            std::sort(mags.begin(), mags.end());
            const unsigned long long ks[] = {1ull, std::max<unsigned long long>(1ull, (unsigned long long)(0.8 * (double)n)), (unsigned long long)n};
            for (unsigned long long k : ks) {
                bool nonfinite;
                const uint32_t got = select_kth(x, k, &nonfinite);
                if (got != mags[(size_t)k - 1] || nonfinite) {
                    std::printf("%s n=%zu k=%llu: got %08x want %08x nonfinite=%d\n", kind, n, k, got, mags[(size_t)k - 1], (int)nonfinite);
                    return 1;
                }
                ++checked;
            }
        }
        std::printf("%s: %zu selections equal the sort\n", kind, checked);
    }
    std::vector<float> bad = make("normal", 257, rng);
    bool nonfinite;
    bad[200] = INFINITY;
    select_kth(bad, 7, &nonfinite);
    if (!nonfinite) { std::printf("inf not flagged\n"); return 1; }
    bad[200] = NAN;
    select_kth(bad, 7, &nonfinite);
    if (!nonfinite) { std::printf("nan not flagged\n"); return 1; }
    std::printf("inf / nan flagged\nok\n");
    return 0;
}
