// Stand-alone host program for tests/test_mcmc_cpu.py: csrc/philox.hpp compiled by plain g++ (the header includes nothing from
// HIP then), printing the published known answers, and the words and normals of a few (seed, call, purpose, index) for the
// numpy restatement to be compared with.
#include <cinttypes>
#include <cstdio>

#include "../r2_gaussian_amd/csrc/philox.hpp"

int main()
{
    using namespace r2;
    const uint32_t kat[3][6] = {
        { 0u, 0u, 0u, 0u, 0u, 0u },
        { 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu },
        { 0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u },
    };
    for (const auto &k : kat) {
        const Philox4 p = philox4x32_10(k[0], k[1], k[2], k[3], k[4], k[5]);
        std::printf("kat %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", p.w[0], p.w[1], p.w[2], p.w[3]);
    }
    const uint64_t seed = 0x0123456789abcdefull, call = (1ull << 40) + 3ull;
    for (uint32_t purpose = 0; purpose < 3; ++purpose)
        for (uint32_t index = 0; index < 100; ++index) {
            const uint32_t at = index * 40503u;   // indices spread over the 32 bits
            const Philox4 p = philox_words(seed, call, purpose, at);
            float e[3];
            philox_normal3(seed, call, purpose, at, e);
            std::printf("draw %" PRIu32 " %" PRIu32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %a %a %a\n", purpose, at,
                        p.w[0], p.w[1], p.w[2], p.w[3], (double)e[0], (double)e[1], (double)e[2]);
        }
    std::printf("philox ok\n");
    return 0;
}
