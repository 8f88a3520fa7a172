// Host check of fast_ray_tracer_amd/csrc/frt_cam_index.hpp (compiled and run by tests/test_cam_index.py): the
// multiply-shift quotient and remainder against / and %, and the rule that admits a batch to the 32-bit index math.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "frt_cam_index.hpp"

static long long g_checked = 0;

static bool check(uint32_t n, uint32_t d) {
    const frt::DivMagic m = frt::div_magic(d);
    const uint32_t q = frt::magic_div(n, m.magic, m.shift), r = frt::magic_rem(n, q, d);
    ++g_checked;
    if (q == n / d && r == n % d) return true;
    std::printf("FAIL %u / %u: got %u rem %u, want %u rem %u (magic %u shift %u)\n", n, d, q, r, n / d, n % d, m.magic,
                m.shift);
    return false;
}

int main() {
    const uint32_t divisors[] = {1u, 2u, 3u, 9u, 63u, 64u, 65u, 1919u, 1920u, 0x7FFFFFFFu};
    bool ok = true;
    for (const uint32_t d : divisors) {
        // 0, 2^32 - 1, and around every 2^k, k <= 32, the multiples of d next to it, each with its neighbours
        std::vector<uint64_t> ns = {0ull, 0xFFFFFFFFull};
        for (int k = 0; k <= 32; ++k) {
            const uint64_t p = 1ull << k, below = p / d * d;
            for (const uint64_t mult : {below - (below >= d ? d : 0), below, below + d})
                for (int e = -1; e <= 1; ++e) ns.push_back(mult + (uint64_t)(int64_t)e);
        }
        for (const uint64_t n : ns)
            if (n <= 0xFFFFFFFFull) ok = check((uint32_t)n, d) && ok;  // (0 - 1 wraps to 2^64 - 1: out of range)
    }
    // the rule: samples and pixel_begin + pixels within 32 bits unsigned, spp, hsize and the rows below 2^31
    const int64_t two32 = 1ll << 32, two31 = 1ll << 31;
    struct Case {
        int64_t ns, p0, np, spp, hs, r0, rs;
        bool want;
    } cases[] = {
        {64 * 1920 * 1080, 0, 1920 * 1080, 64, 1920, 0, 1, true},  // the headline frame in one batch
        {9, two32 - 2, 1, 9, 1920, 0, 1, true},                    // last pixel index 2^32 - 2
        {9, two32 - 1, 1, 9, 1920, 0, 1, false},                   // last pixel index 2^32 - 1: the sum is 2^32
        {9, two32, 1, 9, 1920, 0, 1, false},                       // last pixel index 2^32
        {18, two32 - 1, 2, 9, 1920, 0, 1, false},                  // last pixel index 2^32, begun below it
        {two32, 0, two32 / 4, 4, 1920, 0, 1, false},               // 2^32 samples
        {two32 - 4, 0, two32 / 4 - 1, 4, 1920, 0, 1, true},
        {two31, 0, 1, two31, 1920, 0, 1, false},                   // spp 2^31
        {8, 0, 8, 1, two31, 0, 1, false},                          // hsize 2^31
        {8, 0, 8, 1, two31 - 1, 0, 1, true},
        {8, 16, 8, 1, 8, two31 - 3, 1, true},                      // last row 2^31 - 1
        {8, 16, 8, 1, 8, two31 - 2, 1, false},                     // last row 2^31
        {8, 0, 8, 1, 8, -1, 1, false},
    };
    for (const Case& c : cases) {
        const bool got = frt::cam_index_fits32(c.ns, c.p0, c.np, c.spp, c.hs, c.r0, c.rs);
        ++g_checked;
        if (got != c.want) {
            std::printf("FAIL rule: samples %lld pixels [%lld, +%lld) spp %lld hsize %lld rows %lld by %lld: got %d\n",
                        (long long)c.ns, (long long)c.p0, (long long)c.np, (long long)c.spp, (long long)c.hs,
                        (long long)c.r0, (long long)c.rs, (int)got);
            ok = false;
        }
    }
    std::printf("%s %lld checks\n", ok ? "OK" : "FAILED", g_checked);
    return ok ? 0 : 1;
}
