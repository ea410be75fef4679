// tests/test_shade_predicates_host.py: the host twins of pt_device.h's mask-arithmetic range predicates
// (coord_ok_m, dir_ok_m, ray_fast_m) against the '&&' / '||' forms (coord_ok, dir_ok, ray_fast, and the same chains
// spelled out here) over an edge grid.  Prints one summary line; exits 1 on a mismatch.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "pt_device.h"

static bool coord_ok_ref(float v)
{
    const float a = std::fabs(v);
    return a == 0.0f || (a >= 0x1p-50f && a <= 0x1p20f);
}
static bool dir_ok_ref(float v)
{
    const float a = std::fabs(v);
    return a == 0.0f || (a >= 0x1p-100f && a <= 0x1p45f);
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    // 0, +-2^-101, +-2^-100, +-2^-51, +-2^-50, +-2^20 and the float above, +-2^45 and the float above, inf, NaN
    std::vector<float> g = {0.0f, -0.0f};
    for (float m : {0x1p-101f, 0x1p-100f, 0x1p-51f, 0x1p-50f, 0x1p20f, std::nextafterf(0x1p20f, inf), 0x1p45f,
                    std::nextafterf(0x1p45f, inf), inf, std::numeric_limits<float>::quiet_NaN(),
                    // (and the neighbours below each bound, a denormal, 1)
                    std::nextafterf(0x1p-100f, 0.0f), std::nextafterf(0x1p-50f, 0.0f), std::nextafterf(0x1p20f, 0.0f),
                    std::nextafterf(0x1p45f, 0.0f), 0x1p-149f, 1.0f}) {
        g.push_back(m);
        g.push_back(-m);
    }
    int bad = 0, n1 = 0, n6 = 0;
    for (float v : g) {
        ++n1;
        if ((ptd::coord_ok_m(v) != 0) != coord_ok_ref(v) || ptd::coord_ok(v) != coord_ok_ref(v)) { printf("coord_ok(%a)\n", v); ++bad; }
        if ((ptd::dir_ok_m(v) != 0) != dir_ok_ref(v) || ptd::dir_ok(v) != dir_ok_ref(v)) { printf("dir_ok(%a)\n", v); ++bad; }
    }
    // ray_fast: every pair of grid values in every component and its neighbour, the other four at in-range values
    for (int k = 0; k < 6; ++k)
        for (float v : g)
            for (float w : g) {
                float c[6] = {1.0f, -2.0f, 0.0f, 0.5f, -0.0f, -0.25f};
                c[k] = v;
                c[(k + 5) % 6] = w;
                const bool ref = coord_ok_ref(c[0]) && coord_ok_ref(c[1]) && coord_ok_ref(c[2]) && dir_ok_ref(c[3]) &&
                                 dir_ok_ref(c[4]) && dir_ok_ref(c[5]);
                const ptd::V3 o = ptd::v3(c[0], c[1], c[2]), d = ptd::v3(c[3], c[4], c[5]);
                ++n6;
                if (ptd::ray_fast_m(o, d) != ref || ptd::ray_fast(o, d) != ref) { printf("ray_fast %d %a %a\n", k, v, w); ++bad; }
            }
    printf("coord_ok/dir_ok %d values, ray_fast %d rays: %d mismatches\n", n1, n6, bad);
    return bad ? 1 : 0;
}
