// ceg_coalesce.h -- the two pieces of the site extraction that are plain sequential FP64 and are shared by the host and the device:
//   ceg_pdwo            periodic_distance_with_ofs!, utils.jl:257-280, operation by operation
//   ceg_coalesce_greedy the greedy pass of coalescing_basins, basins.jl:677-719, line by line
// No HIP in here: the file also compiles as ordinary C++ (tests/native/coalesce_sanitize.cpp does so under the sanitizers).
#ifndef CEG_COALESCE_H
#define CEG_COALESCE_H

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define CEG_HD __host__ __device__
#else
#define CEG_HD
#endif

// every expression below is the reference's, in its order: no contraction into fma
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

// norm(mat*b): mat 3x3 column-major, rows summed left to right, then sqrt(x*x + y*y + z*z) with a correctly rounded square root
CEG_HD inline double ceg_norm_matvec(const double* m, const double (&b)[3])
{
    const double x = m[0] * b[0] + m[3] * b[1] + m[6] * b[2];
    const double y = m[1] * b[0] + m[4] * b[1] + m[7] * b[2];
    const double z = m[2] * b[0] + m[5] * b[1] + m[8] * b[2];
    return sqrt(x * x + y * y + z * z);
}

// utils.jl:257-280.  b: the fractional difference, wrapped in place; ofs: the cell offset (an integer, held as O)
template <typename O>
CEG_HD inline double ceg_pdwo(const double* m, bool ortho, double safemin, double (&b)[3], O (&ofs)[3])
{
#pragma unroll
    for (int q = 0; q < 3; ++q) {                                    // :258-261
        const double diff = b[q] + 0.5;
        const double fl = floor(diff);
        ofs[q] = (O)fl;
        b[q] = diff - fl - 0.5;
    }
    const double ref = ceg_norm_matvec(m, b);                        // :262
    if (ortho || ref <= safemin) return ref;                         // :263
#pragma unroll
    for (int q = 0; q < 3; ++q) {                                    // :264-278, first improvement
        b[q] += 1;
        double nn = ceg_norm_matvec(m, b);
        if (nn < ref) {
            ofs[q] -= 1;
            return nn;
        }
        b[q] -= 2;
        nn = ceg_norm_matvec(m, b);
        if (nn < ref) {
            ofs[q] += 1;
            return nn;
        }
        b[q] += 1;
    }
    return ref;
}

struct CegBasin {
    double val;
    double c[3];
};

// basins.jl:677-719 over a ranking that is already cut at the crop (:679).  lin: 0-based linear indices; smoothed / values: the smoothed
// and the unsmoothed grid at them.  -> the basins, in the order the reference's `ret` holds them when the loop ends
inline std::vector<CegBasin> ceg_coalesce_greedy(const int32_t* lin, const double* smoothed, const double* values, int64_t nranked,
                                                 const int32_t dims[3], const double* mat, bool ortho, double safemin, double maxdist,
                                                 double atol, double maxbasins)
{
    struct InDist {
        int64_t idx;
        double ofs[3];
        double d;
    };
    std::vector<CegBasin> ret;
    std::vector<InDist> in_distance;
    std::vector<int64_t> js;
    const int64_t a = dims[0], b = dims[1], c = dims[2];
    for (int64_t r = 0; r < nranked; ++r) {
        const double smval = smoothed[r], val = values[r];
        const int64_t x = lin[r];
        const int64_t i = x % a + 1, j = (x / a) % b + 1, k = x / (a * b) + 1;                 // :681-682, 1-based
        const double pos[3] = {(double)i / (double)a, (double)j / (double)b, (double)k / (double)c};      // :683
        in_distance.clear();
        for (size_t idx = 0; idx < ret.size(); ++idx) {                                       // :685-690
            double buffer[3] = {pos[0] - ret[idx].c[0], pos[1] - ret[idx].c[1], pos[2] - ret[idx].c[2]};
            double ofs[3];
            const double d = ceg_pdwo(mat, ortho, safemin, buffer, ofs);
            if (d > maxdist) continue;
            in_distance.push_back(InDist{(int64_t)idx, {ofs[0], ofs[1], ofs[2]}, d});
        }
        if (in_distance.empty() && smval >= atol) {                                           // :691-693
            ret.push_back(CegBasin{val, {pos[0], pos[1], pos[2]}});
            if ((double)ret.size() >= maxbasins) break;
            continue;
        }
        if (in_distance.size() > 1) {                                                         // :695-699
            std::stable_sort(in_distance.begin(), in_distance.end(), [](const InDist& p, const InDist& q) {
                return p.d < q.d || (q.d != q.d && p.d == p.d);                               // isless: a NaN sorts last
            });
            size_t submid = 1;
            if (!(val < atol)) {
                for (size_t q = 0; q < in_distance.size(); ++q)
                    if (in_distance[q].d < maxdist / 2) {
                        submid = q + 1;
                        break;
                    }
            }
            in_distance.resize(submid);
        }
        double newcenter[3] = {pos[0] * val, pos[1] * val, pos[2] * val};                     // :700-706
        double newval = val;
        for (const InDist& e : in_distance) {
            const CegBasin& o = ret[(size_t)e.idx];
            for (int q = 0; q < 3; ++q) newcenter[q] += (o.c[q] + e.ofs[q]) * o.val;
            newval += o.val;
        }
        if (newval == 0) continue;                                                            // :707
        for (int q = 0; q < 3; ++q) newcenter[q] /= newval;                                   // :708
        const CegBasin merged{newval, {newcenter[0], newcenter[1], newcenter[2]}};
        if (in_distance.size() == 1) {                                                        // :709-710
            ret[(size_t)in_distance[0].idx] = merged;
        } else {                                                                              // :712-716
            js.clear();
            for (const InDist& e : in_distance) js.push_back(e.idx);
            std::sort(js.begin(), js.end());
            for (size_t q = js.size(); q-- > 0;) ret.erase(ret.begin() + js[q]);
            ret.push_back(merged);
        }
    }
    return ret;
}

#endif  // CEG_COALESCE_H
