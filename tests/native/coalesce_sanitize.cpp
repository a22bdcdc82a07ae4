// The greedy pass of coalescing_basins (csrc/ceg_coalesce.h) as a program of its own, for -fsanitize=address,undefined on the host:
// hand-made rankings that take each branch, then random ones with many basins coming, merging and going.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "ceg_coalesce.h"

static int run(const std::vector<int32_t>& lin, const std::vector<double>& sm, const std::vector<double>& val, const int32_t dims[3],
               const double* mat, bool ortho, double safemin, double maxdist, double atol, double maxbasins)
{
    const std::vector<CegBasin> ret = ceg_coalesce_greedy(lin.data(), sm.data(), val.data(), (int64_t)lin.size(), dims, mat, ortho, safemin,
                                                          maxdist, atol, maxbasins);
    double tot = 0;
    for (const CegBasin& b : ret) tot += b.val + b.c[0] + b.c[1] + b.c[2];
    std::printf("%zu basins, checksum %.17g\n", ret.size(), tot);
    return (int)ret.size();
}

int main()
{
    const int32_t dims[3] = {12, 10, 14};
    const double ortho_mat[9] = {11.5, 0, 0, 0, 11.0, 0, 0, 0, 12.5};
    const double skew_mat[9] = {12.0, 0, 0, -2.8470095, 10.62518409, 0, -1.13302466, 2.03346665, 12.78988931};      // column-major
    auto L = [&](int i, int j, int k) { return (int32_t)(i + dims[0] * (j + dims[1] * k)); };
    int bad = 0;
    for (int skew = 0; skew < 2; ++skew) {
        const double* m = skew ? skew_mat : ortho_mat;
        const double safemin = skew ? 5.0 : 5.5;
        // new basins, absorbed neighbours, several in range, a low value, a lone low value, a zero, maxbasins
        bad += run({L(1, 1, 1), L(7, 5, 8), L(1, 6, 12)}, {0.9, 0.8, 0.7}, {0.5, 0.25, 0.125}, dims, m, !skew, safemin, 1.5, 0.1, INFINITY) != 3;
        bad += run({L(5, 5, 5), L(6, 5, 5), L(5, 4, 5), L(4, 5, 6)}, {0.9, 0.8, 0.7, 0.6}, {0.4, 0.3, 0.2, 0.1}, dims, m, !skew, safemin, 2.5, 0.1,
                   INFINITY) != 1;
        bad += run({L(3, 5, 5), L(7, 5, 5), L(5, 5, 5), L(4, 5, 5)}, {0.9, 0.8, 0.7, 0.6}, {0.4, 0.3, 0.05, 0.1}, dims, m, !skew, safemin, 2.2, 0.1,
                   INFINITY) != 2;
        bad += run({L(1, 1, 1), L(7, 5, 8), L(1, 6, 12), L(8, 1, 3)}, {0.9, 0.05, 0.04, 0.03}, {0.5, 0.3, 0.0, 0.07}, dims, m, !skew, safemin, 1.5,
                   0.1, INFINITY) != 3;
        bad += run({L(1, 1, 1), L(7, 5, 8), L(1, 6, 12)}, {0.9, 0.8, 0.7}, {0.5, 0.25, 0.125}, dims, m, !skew, safemin, 1.5, 0.1, 2) != 2;
        bad += run({}, {}, {}, dims, m, !skew, safemin, 1.5, 0.1, INFINITY) != 0;
        std::mt19937_64 rng(12345 + skew);
        const int n = dims[0] * dims[1] * dims[2];
        for (int round = 0; round < 4; ++round) {
            std::vector<int32_t> lin(n);
            for (int x = 0; x < n; ++x) lin[x] = x;
            std::shuffle(lin.begin(), lin.end(), rng);
            lin.resize(n / (1 + round));
            std::vector<double> sm(lin.size()), val(lin.size());
            for (size_t q = 0; q < lin.size(); ++q) {
                sm[q] = (double)(rng() % 16) / 64.0;
                val[q] = (double)(rng() % 9) / 64.0;
            }
            run(lin, sm, val, dims, m, !skew, safemin, 0.8 + round, 0.1, round == 3 ? 5.0 : INFINITY);
        }
    }
    if (bad) {
        std::printf("%d hand-made rankings gave another number of basins\n", bad);
        return 1;
    }
    std::printf("coalesce ok\n");
    return 0;
}
