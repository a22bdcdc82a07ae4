// ceg_coalesce.h -- the pieces of the site extraction that are plain sequential FP64 and are shared by the host and the device:
//   ceg_pdwo            periodic_distance_with_ofs!, utils.jl:257-280, operation by operation
//   ceg_coalesce_greedy the greedy pass of coalescing_basins, basins.jl:677-719, line by line
//   ceg_nearer, ceg_coalesce_lone, ceg_coalesce_absorb   the order and the two updates of that pass as the nearest-basin rule the device
//                       follows (ceg_grid_coalesce.hip); tests/native/cluster_sanitize.cpp holds them against the loop above
//   ceg_cluster_closer_than_inplace   cluster_closer_than!, basins.jl:613-642, line by line (host)
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

// As :695-699 are written the in-distance list keeps one entry, the nearest basin (isless on d, a NaN last, the lowest index among
// equals), so the loop body has two updates; both are :700-708 in the reference's operation order, ofs held as double.
// isless(d1, d2) with the index as the second key: the order of the stable sort of :696
CEG_HD inline bool ceg_isless(double p, double q) { return p < q || (q != q && p == p); }

CEG_HD inline bool ceg_nearer(double d1, int64_t i1, double d2, int64_t i2)
{
    return ceg_isless(d1, d2) || (!ceg_isless(d2, d1) && i1 < i2);
}

// nothing in range and smval < atol: (val, pos*val/val) -- not pos.  The caller skips val == 0 (:707)
CEG_HD inline CegBasin ceg_coalesce_lone(double val, const double (&pos)[3])
{
    CegBasin o;
    o.val = val;
#pragma unroll
    for (int q = 0; q < 3; ++q) o.c[q] = pos[q] * val / val;
    return o;
}

// one basin in range: it becomes (val + v2, (pos*val + (c + ofs)*v2) / (val + v2)); false, and nothing changed, where val + v2 == 0
CEG_HD inline bool ceg_coalesce_absorb(CegBasin& o, double val, const double (&pos)[3], const double (&ofs)[3])
{
    const double newval = val + o.val;
    if (newval == 0) return false;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        double nc = pos[q] * val;
        nc += (o.c[q] + ofs[q]) * o.val;
        o.c[q] = nc / newval;
    }
    o.val = newval;
    return true;
}

// cluster_closer_than!, basins.jl:613-642, line by line, in place: rho[n], pos[n][3].  -> the number of entries kept, moved to the front
inline int64_t ceg_cluster_closer_than_inplace(double* rho, double* pos, int64_t n, const double* mat, bool ortho, double safemin,
                                               double maxdist)
{
    std::vector<char> todelete((size_t)n, 0);
    for (int64_t i1 = 0; i1 < n; ++i1) {
        if (todelete[(size_t)i1]) continue;                                                   // :619
        double rho1 = rho[i1], pos1[3] = {pos[3 * i1], pos[3 * i1 + 1], pos[3 * i1 + 2]};
        for (int64_t i2 = i1 + 1; i2 < n; ++i2) {
            if (todelete[(size_t)i2]) continue;                                               // :622
            const double rho2 = rho[i2];
            const double* pos2 = pos + 3 * i2;
            const double r = rho1 + rho2;
            if (r > 1) continue;                                                              // :625
            double buffer[3] = {pos1[0] - pos2[0], pos1[1] - pos2[1], pos1[2] - pos2[2]};
            double ofs[3];
            const double d = ceg_pdwo(mat, ortho, safemin, buffer, ofs);
            if (d >= maxdist) continue;                                                       // :633
            todelete[(size_t)i2] = 1;
            for (int q = 0; q < 3; ++q) pos1[q] = (rho1 * pos1[q] + rho2 * (pos2[q] + ofs[q])) / r;      // :635
            rho1 = r;
            rho[i1] = rho1;                                                                   // :637
            for (int q = 0; q < 3; ++q) pos[3 * i1 + q] = pos1[q];
        }
    }
    int64_t kept = 0;
    for (int64_t i = 0; i < n; ++i) {                                                         // :640
        if (todelete[(size_t)i]) continue;
        rho[kept] = rho[i];
        for (int q = 0; q < 3; ++q) pos[3 * kept + q] = pos[3 * i + q];
        ++kept;
    }
    return kept;
}

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
