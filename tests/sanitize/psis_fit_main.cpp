// Stand-alone harness of the PSIS fit (kmc_psis_fit.hpp) for a host sanitizer build: the header's arithmetic with the host context over
// tails of every size class -- empty, below the fit, the smallest fit, ragged against the 256 lanes, the 4 096 limit (where the grid
// scratch is full: 30 + 64 entries) -- and over degenerate ones (all equal, a huge spread).  Prints one line per tail; the test that
// builds it (tests/test_psis_loo_cpu.py) compares two of them with the library.  No device, no library: only the header.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kmc_psis_fit.hpp"

int main()
{
    using namespace kmc_psis;
    const int sizes[] = {0, 1, 4, 5, 6, 255, 256, 257, 1000, kMaxTail};
    unsigned long long state = 88172645463325252ull;
    auto uniform = [&]() {                                   // xorshift64: the same tails on every machine
        state ^= state << 13; state ^= state >> 7; state ^= state << 17;
        return (double)(state >> 11) * (1.0 / 9007199254740992.0);
    };
    for (int shape = 0; shape < 3; ++shape)
        for (int nt : sizes) {
            const double xc = -12.0;
            std::vector<double> x((size_t)nt), s((size_t)nt);
            for (int t = 0; t < nt; ++t) {
                const double u = uniform();
                const double r = shape == 0 ? 0.3 * expm1(-0.5 * log1p(-u)) / 0.5 : shape == 1 ? 1.0 : 1e4 * u;
                x[(size_t)t] = xc + log1p(r);
            }
            for (int a = 1; a < nt; ++a)                     // insertion sort: ascending
                for (int b = a; b > 0 && x[(size_t)b] < x[(size_t)b - 1]; --b) { const double v = x[(size_t)b]; x[(size_t)b] = x[(size_t)b - 1]; x[(size_t)b - 1] = v; }
            std::vector<double> grid(3 * (size_t)kMaxGrid);
            HostCtx ctx;
            const FitScratch sc{grid.data(), grid.data() + kMaxGrid, grid.data() + 2 * kMaxGrid};
            const FitResult r = psis_fit(ctx, x.data(), s.data(), nt, xc, sc);
            std::printf("shape %d nt %d k %.17g sigma %.17g w_tail %.17g n_tail %.17g elpd %.17g\n", shape, nt, r.k, r.sigma, r.w_tail, r.n_tail,
                        psis_elpd(-3.0, 100.0, 5000 + nt, nt, r));
        }
    return 0;
}
