// The host stages of the quantile MCSE (csrc/kmc_quantile_host.hpp) in a program of their own, for the host sanitizers
// (tests/test_quantile_mcse_cpu.py builds it with -fsanitize=address,undefined and runs it): the Beta quantile and the index rule over
// the grid of the tests, and the indicator moments at the ends of their range.  One line per case; every line is printed twice from two
// evaluations, so that a difference between equal calls shows.
#include <cstdio>

#include "kmc_quantile_host.hpp"

using namespace kmc_quantile_host;

int main()
{
    const double ess[5] = {1.5, 10.0, 1e3, 1e6, 2e9}, p[5] = {0.001, 0.05, 0.5, 0.95, 0.999};
    const int64_t S = 100000;
    int bad = 0;
    for (int e = 0; e < 5; ++e)
        for (int k = 0; k < 5; ++k) {
            double a[2], b[2];
            int64_t i1[2], i2[2];
            for (int r = 0; r < 2; ++r)
                if (!quantile_mcse_ranks(S, p[k], ess[e], &a[r], &b[r], &i1[r], &i2[r])) ++bad;
            if (a[0] != a[1] || b[0] != b[1] || i1[0] != i1[1] || i2[0] != i2[1]) ++bad;
            if (!(a[0] > 0.0 && a[0] < b[0] && b[0] < 1.0) || i1[0] < 0 || i2[0] >= S || i1[0] > i2[0]) ++bad;
            std::printf("ess %.17g p %.17g a %.17g b %.17g i1 %lld i2 %lld\n", ess[e], p[k], a[0], b[0], (long long)i1[0], (long long)i2[0]);
        }
    {   // the ends of the parameter range, and an ess that gives no interval
        double x = 0.0, a, b;
        int64_t i1, i2;
        if (!beta_quantile(kPhiMinus1, 1.0, 1.0, &x)) ++bad;
        std::printf("uniform %.17g\n", x);
        if (!beta_quantile(kPhiPlus1, 2147483649.0, 1.0, &x)) ++bad;
        std::printf("edge %.17g\n", x);
        if (!beta_quantile(kPhiMinus1, 1.0, 2147483649.0, &x)) ++bad;
        std::printf("edge %.17g\n", x);
        if (!quantile_mcse_ranks(S, 0.5, std::numeric_limits<double>::quiet_NaN(), &a, &b, &i1, &i2) || a == a || i1 != -1 || i2 != -1) ++bad;
        if (!quantile_mcse_ranks(S, 0.5, 0.0, &a, &b, &i1, &i2) || a == a || i1 != -1) ++bad;
        if (!quantile_mcse_ranks(1, 0.5, 1.0, &a, &b, &i1, &i2) || i1 != 0 || i2 != 0) ++bad;
    }
    const int64_t hk[4][2] = {{4, 0}, {4, 4}, {5, 2}, {2147483647, 1073741823}};
    for (int i = 0; i < 4; ++i) {
        double mu, s2;
        indicator_moments(hk[i][0], hk[i][1], &mu, &s2);
        std::printf("h %lld k %lld mu %.17g s2 %.17g\n", (long long)hk[i][0], (long long)hk[i][1], mu, s2);
    }
    std::printf("bad %d\n", bad);
    return bad ? 1 : 0;
}
