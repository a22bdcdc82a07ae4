// cluster_closer_than! and the two updates of the nearest-basin rule (csrc/ceg_coalesce.h) as a program of its own, for
// -fsanitize=address,undefined on the host: lists that merge into chains, that hit the cap, that are empty; and the rule built from
// ceg_coalesce_lone / ceg_coalesce_absorb against the bytes of the line-by-line loop on random rankings.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "ceg_coalesce.h"

static int64_t cluster(std::vector<double> rho, std::vector<double> pos, const double* mat, bool ortho, double safemin, double maxdist)
{
    const int64_t kept = ceg_cluster_closer_than_inplace(rho.data(), pos.data(), (int64_t)rho.size(), mat, ortho, safemin, maxdist);
    double tot = 0;
    for (int64_t q = 0; q < kept; ++q) tot += rho[(size_t)q] + pos[3 * (size_t)q] + pos[3 * (size_t)q + 1] + pos[3 * (size_t)q + 2];
    std::printf("%lld of %zu entries kept, checksum %.17g\n", (long long)kept, rho.size(), tot);
    return kept;
}

// the loop as the device runs it: the nearest basin in range, then one of the two updates
static std::vector<CegBasin> rule(const std::vector<int32_t>& lin, const std::vector<double>& sm, const std::vector<double>& val,
                                  const int32_t dims[3], const double* mat, bool ortho, double safemin, double maxdist, double atol,
                                  double maxbasins)
{
    std::vector<CegBasin> ret;
    const int64_t a = dims[0], b = dims[1], c = dims[2];
    for (size_t r = 0; r < lin.size(); ++r) {
        const int64_t x = lin[r];
        const double pos[3] = {(double)(x % a + 1) / (double)a, (double)((x / a) % b + 1) / (double)b, (double)(x / (a * b) + 1) / (double)c};
        int64_t bi = -1;
        double bd = 0, bofs[3] = {0, 0, 0};
        for (size_t idx = 0; idx < ret.size(); ++idx) {
            double buffer[3] = {pos[0] - ret[idx].c[0], pos[1] - ret[idx].c[1], pos[2] - ret[idx].c[2]};
            double ofs[3];
            const double d = ceg_pdwo(mat, ortho, safemin, buffer, ofs);
            if (d > maxdist) continue;
            if (bi < 0 || ceg_nearer(d, (int64_t)idx, bd, bi)) {
                bd = d;
                bi = (int64_t)idx;
                std::memcpy(bofs, ofs, sizeof bofs);
            }
        }
        if (bi < 0) {
            if (sm[r] >= atol) {
                ret.push_back(CegBasin{val[r], {pos[0], pos[1], pos[2]}});
                if ((double)ret.size() >= maxbasins) break;
            } else if (!(val[r] == 0)) {
                ret.push_back(ceg_coalesce_lone(val[r], pos));
            }
        } else {
            ceg_coalesce_absorb(ret[(size_t)bi], val[r], pos, bofs);
        }
    }
    return ret;
}

int main()
{
    const double ortho_mat[9] = {11.5, 0, 0, 0, 11.0, 0, 0, 0, 12.5};
    const double skew_mat[9] = {12.0, 0, 0, -2.8470095, 10.62518409, 0, -1.13302466, 2.03346665, 12.78988931};      // column-major
    int bad = 0;
    for (int skew = 0; skew < 2; ++skew) {
        const double* m = skew ? skew_mat : ortho_mat;
        const double safemin = skew ? 5.0 : 5.5;
        bad += cluster({}, {}, m, !skew, safemin, 2.0) != 0;
        bad += cluster({0.3}, {0.1, 0.2, 0.3}, m, !skew, safemin, 2.0) != 1;
        bad += cluster({0.3, 0.2}, {0.1, 0.2, 0.3, 0.98, 0.2, 0.31}, m, !skew, safemin, 3.0) != 1;                    // across the cell boundary
        bad += cluster({0.6, 0.5, 0.3}, {0.5, 0.5, 0.5, 0.52, 0.5, 0.5, 0.5, 0.52, 0.5}, m, !skew, safemin, 2.0) != 2;   // 0.6 + 0.5 > 1 stays apart
        std::vector<double> rho, pos;
        for (int q = 0; q < 12; ++q) {                                                                               // a chain into one entry
            rho.push_back(0.05);
            pos.push_back(0.1 + 0.02 * q);
            pos.push_back(0.3);
            pos.push_back(0.3);
        }
        bad += cluster(rho, pos, m, !skew, safemin, 8.0) != 1;
        std::mt19937_64 rng(777 + skew);
        std::uniform_real_distribution<double> u(-0.2, 1.2), w(0.01, 0.3);
        rho.clear();
        pos.clear();
        for (int q = 0; q < 400; ++q) {
            rho.push_back(w(rng));
            for (int r = 0; r < 3; ++r) pos.push_back(u(rng));
        }
        cluster(rho, pos, m, !skew, safemin, 2.0);
        // the rule from the two helpers against the loop as written
        const int32_t dims[3] = {12, 10, 14};
        const int n = dims[0] * dims[1] * dims[2];
        for (int round = 0; round < 4; ++round) {
            std::vector<int32_t> lin(n);
            for (int x = 0; x < n; ++x) lin[x] = x;
            std::shuffle(lin.begin(), lin.end(), rng);
            lin.resize(n / (1 + round));
            std::vector<double> sm(lin.size()), val(lin.size());
            for (size_t q = 0; q < lin.size(); ++q) {
                sm[q] = (double)(rng() % 16) / 64.0;
                val[q] = ((double)(rng() % 9) - 1.0) / 64.0;                      // zeros and negative values among them
            }
            const double maxdist = 0.8 + round, maxbasins = round == 3 ? 5.0 : INFINITY;
            const std::vector<CegBasin> want = ceg_coalesce_greedy(lin.data(), sm.data(), val.data(), (int64_t)lin.size(), dims, m, !skew,
                                                                   safemin, maxdist, 0.1, maxbasins);
            const std::vector<CegBasin> got = rule(lin, sm, val, dims, m, !skew, safemin, maxdist, 0.1, maxbasins);
            const bool same = got.size() == want.size() && (got.empty() || std::memcmp(got.data(), want.data(), sizeof(CegBasin) * got.size()) == 0);
            std::printf("rule: %zu basins, %s\n", got.size(), same ? "the bytes of the loop" : "DIFFERENT");
            bad += !same;
        }
    }
    if (bad) {
        std::printf("%d checks failed\n", bad);
        return 1;
    }
    std::printf("cluster ok\n");
    return 0;
}
