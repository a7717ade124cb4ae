// Stand-alone host program for tests/test_cloud_model_cpu.py: the arithmetic half of csrc/cloud_model.hpp compiled by plain g++
// (the header includes nothing from HIP then).  Reads lines "f r x y z" / "d r x y z" / "a x" of hexadecimal floats and prints
// the bit patterns of quat_rot<float>, of quat_rot<double>, and of the activations' branches at x.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../r2_gaussian_amd/csrc/cloud_model.hpp"

static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, sizeof u); return u; }
static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, sizeof u); return u; }

int main()
{
    using namespace r2;
    char kind;
    double q[4];
    while (std::scanf(" %c", &kind) == 1) {
        const int want = kind == 'a' ? 1 : 4;
        for (int k = 0; k < want; ++k)
            if (std::scanf("%la", &q[k]) != 1) return 2;
        if (kind == 'f') {
            float R[3][3];
            quat_rot((float)q[0], (float)q[1], (float)q[2], (float)q[3], R);
            std::printf("f");
            for (const auto &row : R)
                for (float v : row) std::printf(" %08" PRIx32, bits(v));
        } else if (kind == 'd') {
            double R[3][3];
            quat_rot(q[0], q[1], q[2], q[3], R);
            std::printf("d");
            for (const auto &row : R)
                for (double v : row) std::printf(" %016" PRIx64, bits(v));
        } else if (kind == 'a') {   // x, softplus_f, inv_softplus_rounded, the unbounded scale_act (a range and lo it must ignore), expf
            const float x = (float)q[0];
            std::printf("a %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32, bits(x), bits(softplus_f(x)),
                        bits(inv_softplus_rounded(x)), bits(scale_act(x, false, 0.299f, 0.001f)), bits(expf(x)));
        } else {
            return 3;
        }
        std::printf("\n");
    }
    std::printf("cloud model ok\n");
    return 0;
}
