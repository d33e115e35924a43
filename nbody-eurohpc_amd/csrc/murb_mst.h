// The pure functions of the minimum-spanning-tree read-out (include/murbmst.h has the definition): one Boruvka round over the
// foreign-nearest sweep's result, the single-linkage cut of a tree, and an edge's fp64 length.  Host code that g++ compiles
// without a device, so that tests/test_mst_host.py checks it through murbmst_round and murbmst_cut; murbmst_of (murbhip.hip)
// calls the same inline functions.  Integers and compares only, but for the length: fp64, one operation per line, none
// contracted.
#ifndef MURB_MST_H_
#define MURB_MST_H_

#include <algorithm>
#include <cmath>
#include <vector>

#define MURB_MST_ROUNDS_MAX 40   // the guard of murbmst_of: Boruvka halves the components each round, so 31 rounds serve any int n

struct MurbMstEdge {
    float r2;
    int i, j;   // i < j
};

// the total order on unordered pairs: (r2, min(i, j), max(i, j)).  r2 is never NaN here (a NaN never wins the sweep)
inline bool murb_mst_before(const MurbMstEdge& a, const MurbMstEdge& b)
{
    if (a.r2 != b.r2) return a.r2 < b.r2;
    if (a.i != b.i) return a.i < b.i;
    return a.j < b.j;
}

inline bool murb_mst_same(const MurbMstEdge& a, const MurbMstEdge& b) { return a.i == b.i && a.j == b.j; }

inline int murb_mst_find(std::vector<int>& up, int v)
{
    while (up[v] != v) {
        up[v] = up[up[v]];   // path halving
        v = up[v];
    }
    return v;
}

// the length of an edge from the fp32 coordinates (include/murbmst.h): d = (double)q_j - (double)q_i, sqrt((dx dx + dy dy) + dz dz)
inline double murb_mst_length(const float xi, const float yi, const float zi, const float xj, const float yj, const float zj)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double dx = (double)xj - (double)xi;
    const double dy = (double)yj - (double)yi;
    const double dz = (double)zj - (double)zi;
    const double xx = dx * dx;
    const double yy = dy * dy;
    const double zz = dz * dz;
    const double xy = xx + yy;
    const double s = xy + zz;
    return std::sqrt(s);
}

// One Boruvka round (include/murbmst.h).  label: n entries, >= 0 a component, < 0 outside; partner, r2: n entries, read at the
// bodies with label >= 0 (partner -1: none).  chosen: the round's edges, ascending by the key, the edge two components choose
// mutually once.  false: the input is not what the foreign-nearest rule gives for these labels (a partner outside [0, n),
// outside the mask or of the body's own label, or an edge that would close a cycle); nothing is changed then.  On success
// label holds the merged components, each under its smallest body index.
inline bool murb_mst_round(const unsigned long n, int* label, const int* partner, const float* r2, std::vector<MurbMstEdge>& chosen)
{
    chosen.clear();
    // the components as dense ids: the distinct labels, ascending
    std::vector<int> ids;
    ids.reserve(n);
    for (unsigned long i = 0; i < n; ++i)
        if (label[i] >= 0) ids.push_back(label[i]);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const auto id_of = [&](int l) { return (int)(std::lower_bound(ids.begin(), ids.end(), l) - ids.begin()); };
    std::vector<int> comp(n, -1);
    for (unsigned long i = 0; i < n; ++i)
        if (label[i] >= 0) comp[i] = id_of(label[i]);
    // per component the minimum, by the key, over its bodies' (i, partner[i], r2[i])
    std::vector<MurbMstEdge> best(ids.size());
    std::vector<char> has(ids.size(), 0);
    for (unsigned long i = 0; i < n; ++i) {
        if (comp[i] < 0 || partner[i] == -1) continue;
        const long p = partner[i];
        if (p < 0 || p >= (long)n || comp[p] < 0 || comp[p] == comp[i]) return false;
        const MurbMstEdge e{r2[i], (int)std::min<long>((long)i, p), (int)std::max<long>((long)i, p)};
        if (!has[comp[i]] || murb_mst_before(e, best[comp[i]])) {
            best[comp[i]] = e;
            has[comp[i]] = 1;
        }
    }
    for (size_t k = 0; k < ids.size(); ++k)
        if (has[k]) chosen.push_back(best[k]);
    std::sort(chosen.begin(), chosen.end(), murb_mst_before);
    chosen.erase(std::unique(chosen.begin(), chosen.end(), murb_mst_same), chosen.end());
    // the union over the components; an edge inside one set would close a cycle
    std::vector<int> up(ids.size());
    for (size_t k = 0; k < ids.size(); ++k) up[k] = (int)k;
    for (const MurbMstEdge& e : chosen) {
        const int a = murb_mst_find(up, comp[e.i]), b = murb_mst_find(up, comp[e.j]);
        if (a == b) {
            chosen.clear();
            return false;
        }
        up[std::max(a, b)] = std::min(a, b);
    }
    // bodies rise, so the first body of a set is its smallest index
    std::vector<int> lowest(ids.size(), -1);
    for (unsigned long i = 0; i < n; ++i) {
        if (comp[i] < 0) continue;
        const int root = murb_mst_find(up, comp[i]);
        if (lowest[root] < 0) lowest[root] = (int)i;
        label[i] = lowest[root];
    }
    return true;
}

// Single-linkage groups (include/murbmst.h): the components under the edges with r2 <= thr, each labelled by its smallest body
// index; bodies on no edge label themselves.  false: an edge index outside [0, n).
inline bool murb_mst_cut(const unsigned long n, const unsigned long edges, const int* ei, const int* ej, const float* er2, const float thr,
                         int* label)
{
    for (unsigned long e = 0; e < edges; ++e)
        if (ei[e] < 0 || ej[e] < 0 || (long)ei[e] >= (long)n || (long)ej[e] >= (long)n) return false;
    std::vector<int> up(n);
    for (unsigned long i = 0; i < n; ++i) up[i] = (int)i;
    for (unsigned long e = 0; e < edges; ++e) {
        if (!(er2[e] <= thr)) continue;
        const int a = murb_mst_find(up, ei[e]), b = murb_mst_find(up, ej[e]);
        if (a != b) up[std::max(a, b)] = std::min(a, b);   // the root is the set's smallest index
    }
    for (unsigned long i = 0; i < n; ++i) label[i] = murb_mst_find(up, (int)i);
    return true;
}

#endif
