// Mesh decimation (inference.py:128-129, the reference's decimate_mesh(v, f, 100000): pymeshlab's quadric edge collapse
// with optimal placement, utils/meshutils.py:63-115) as rules D0-D10 of include/primx_hip.h: edge collapse in rounds of
// pairwise independent edges, float64 throughout, no FMA contraction, no square root.
//
// Every sum whose order matters is taken by one work-item in a fixed order (a vertex's quadric over its sorted corner
// list); atomics are integer only and used where the result does not depend on arrival order (edge face counts, class
// bits, 64-bit minima of unique keys, one collapse counter per wave).  The collapses of a round touch pairwise disjoint
// faces and vertices (D7), so the collapse kernel needs no ordering between its work-items.  Output order is fixed
// (faces and vertices by index, block-prefix compaction): every output is bitwise deterministic.
//
//   edges:     faces per edge, vertex classes (boundary / locked), the range of every vertex in the sorted corner list.
//   quadrics:  one work-item per vertex over its corners in ascending face order (D1).
//   costs:     one work-item per edge: the 3 x 3 solve by cofactors, placement, cost, key, structural validity (D3, D4).
//   select:    one work-item per candidate walks the fans of both endpoints (D6); m1 by 64-bit atomicMin; a candidate
//              takes m2 of its endpoints from their fans and compares (D7).
//   collapse:  prefix of the faces the selected edges remove (D8), the collapses (D9), compaction of the live faces.
//   finish:    referenced vertices in input order, fp32 positions, re-indexed faces, vmap (D10).
//   normals:   per vertex the normalised sum of its faces' g in ascending face order (not part of the bit-exact rules).
#include <algorithm>
#include <climits>
#include <cstring>

#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_common.h"

constexpr int CLS_BOUNDARY = 1, CLS_LOCKED = 2;
constexpr long long KEY_NONE = LLONG_MAX;

// ------------------------------------------------------------------ small float64 helpers (the order is the rule's)

__device__ __forceinline__ void ld3(const double* __restrict__ p, int i, double o[3]) {
    o[0] = p[3 * (size_t)i];
    o[1] = p[3 * (size_t)i + 1];
    o[2] = p[3 * (size_t)i + 2];
}
__device__ __forceinline__ double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void sub3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[0] - b[0];
    o[1] = a[1] - b[1];
    o[2] = a[2] - b[2];
}
__device__ __forceinline__ void cross3(const double a[3], const double b[3], double o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// g = (p1 - p0) x (p2 - p0)
__device__ __forceinline__ void face_g(const double p0[3], const double p1[3], const double p2[3], double g[3]) {
    double e1[3], e2[3];
    sub3(p1, p0, e1);
    sub3(p2, p0, e2);
    cross3(e1, e2, g);
}
// acc += the quadric of the plane (n, d): (a00, a01, a02, a11, a12, a22, q0, q1, q2, c); weighted: each coefficient
// (x y) w
__device__ __forceinline__ void add_plane(double acc[10], const double n[3], double d, double w, bool weighted) {
    const double c[10] = {n[0] * n[0], n[0] * n[1], n[0] * n[2], n[1] * n[1], n[1] * n[2], n[2] * n[2],
                          n[0] * d,    n[1] * d,    n[2] * d,    d * d};
    for (int k = 0; k < 10; ++k) acc[k] = acc[k] + (weighted ? c[k] * w : c[k]);
}

__device__ __forceinline__ bool load_face(const int* __restrict__ f, int t, int V, int idx[3]) {
    for (int k = 0; k < 3; ++k) {
        idx[k] = f[3 * (size_t)t + k];
        if (idx[k] < 0 || idx[k] >= V) return false;
    }
    return true;
}

// ------------------------------------------------------------------ edges (D2)

__global__ __launch_bounds__(THREADS) void md_corner_init_kernel(const int* __restrict__ f, int n, int V, int* __restrict__ vcls) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int x = f[c];
    if (x >= 0 && x < V) vcls[x] = 0;
}

__global__ __launch_bounds__(THREADS) void md_edge_count_kernel(const int* __restrict__ node, int n, int U, int* __restrict__ ecnt) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int e = node[c];
    if (e >= 0 && e < U) atomicAdd(ecnt + e, 1);
}

// sv = the corners' vertices in ascending order: [first, last) of every vertex that occurs
__global__ __launch_bounds__(THREADS) void md_ranges_kernel(const int* __restrict__ sv, int n, int V, int* __restrict__ first,
                                                            int* __restrict__ last) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int x = sv[i];
    if (x < 0 || x >= V) return;
    if (i == 0 || sv[i - 1] != x) first[x] = i;
    if (i == n - 1 || sv[i + 1] != x) last[x] = i + 1;
}

__global__ __launch_bounds__(THREADS) void md_class_kernel(const int* __restrict__ f, const int* __restrict__ node, int n, int V,
                                                           int U, const int* __restrict__ ecnt, int* __restrict__ vcls) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int t = c / 3, k = c - 3 * t;
    const int e = node[c];
    if (e < 0 || e >= U) return;
    const int cnt = ecnt[e];
    const int bits = cnt == 1 ? CLS_BOUNDARY : (cnt > 2 ? CLS_LOCKED : 0);
    if (!bits) return;
    const int a = f[c], b = f[3 * (size_t)t + (k + 1) % 3];
    if (a >= 0 && a < V) atomicOr(vcls + a, bits);
    if (b >= 0 && b < V) atomicOr(vcls + b, bits);
}

// ------------------------------------------------------------------ quadrics (D1)

__global__ __launch_bounds__(THREADS) void md_quadric_kernel(const float* __restrict__ v, const int* __restrict__ f,
                                                             const int* __restrict__ node, const int* __restrict__ order,
                                                             const int* __restrict__ first, const int* __restrict__ last,
                                                             const int* __restrict__ ecnt, int V, int F, int U,
                                                             double* __restrict__ p, double* __restrict__ Q) {
    const int x = blockIdx.x * THREADS + threadIdx.x;
    if (x >= V) return;
    for (int k = 0; k < 3; ++k) p[3 * (size_t)x + k] = (double)v[3 * (size_t)x + k];
    double acc[10];
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    const int lo = max(first[x], 0), hi = min(last[x], 3 * F);
    for (int j = lo; j < hi; ++j) {
        const int c = order[j];
        if (c < 0 || c >= 3 * F) continue;
        const int t = c / 3, kc = c - 3 * t;
        int idx[3];
        if (!load_face(f, t, V, idx)) continue;
        double q[3][3];
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) q[k][a] = (double)v[3 * (size_t)idx[k] + a];
        double g[3];
        face_g(q[0], q[1], q[2], g);
        add_plane(acc, g, -dot3(g, q[0]), 1.0, false);
        for (int ke = 0; ke < 3; ++ke) {                     // the face's boundary edges in corner order
            const int kn = (ke + 1) % 3;
            if (ke != kc && kn != kc) continue;
            const int e = node[3 * (size_t)t + ke];
            if (e < 0 || e >= U || ecnt[e] != 1) continue;
            double d[3], m[3];
            sub3(q[kn], q[ke], d);
            const double l2 = dot3(d, d);
            if (l2 == 0.0) continue;
            cross3(d, g, m);
            add_plane(acc, m, -dot3(m, q[ke]), 1.0 / l2, true);
        }
    }
    for (int k = 0; k < 10; ++k) Q[10 * (size_t)x + k] = acc[k];
}

// ------------------------------------------------------------------ costs (D3, D4)

__device__ __forceinline__ double quadric_cost(const double q[10], const double y[3]) {
    const double a0 = (q[0] * y[0] + q[1] * y[1]) + q[2] * y[2];
    const double a1 = (q[1] * y[0] + q[3] * y[1]) + q[4] * y[2];
    const double a2 = (q[2] * y[0] + q[4] * y[1]) + q[5] * y[2];
    const double yAy = (y[0] * a0 + y[1] * a1) + y[2] * a2;
    const double qy = (q[6] * y[0] + q[7] * y[1]) + q[8] * y[2];
    const double c = (yAy + 2.0 * qy) + q[9];
    return c > 0.0 ? c : 0.0;
}

__global__ __launch_bounds__(THREADS) void md_cost_kernel(const double* __restrict__ p, const double* __restrict__ Q,
                                                          const long long* __restrict__ ukeys, const int* __restrict__ ecnt,
                                                          const int* __restrict__ vcls, int V, int U, int optimal,
                                                          double* __restrict__ xo, double* __restrict__ cost,
                                                          long long* __restrict__ key, int* __restrict__ valid) {
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= U) return;
    const long long uk = ukeys[e];
    const long long a64 = uk / V, b64 = uk % V;
    if (uk < 0 || a64 >= V || a64 >= b64) {                  // not an edge key: never a candidate, sorts last
        for (int k = 0; k < 3; ++k) xo[3 * (size_t)e + k] = 0.0;
        cost[e] = 0.0;
        key[e] = (long long)(0x7fffffffULL << 32) | (long long)e;
        valid[e] = 0;
        return;
    }
    const int a = (int)a64, b = (int)b64;
    double q[10], pa[3], pb[3], mid[3], d[3];
    for (int k = 0; k < 10; ++k) q[k] = Q[10 * (size_t)a + k] + Q[10 * (size_t)b + k];
    ld3(p, a, pa);
    ld3(p, b, pb);
    for (int k = 0; k < 3; ++k) mid[k] = (pa[k] + pb[k]) * 0.5;
    double x[3] = {0.0, 0.0, 0.0}, cx = 0.0;
    bool use = false;
    if (optimal) {
        const double c00 = q[3] * q[5] - q[4] * q[4], c01 = q[2] * q[4] - q[1] * q[5], c02 = q[1] * q[4] - q[2] * q[3];
        const double c11 = q[0] * q[5] - q[2] * q[2], c12 = q[1] * q[2] - q[0] * q[4], c22 = q[0] * q[3] - q[1] * q[1];
        const double det = (q[0] * c00 + q[1] * c01) + q[2] * c02;
        const double t3 = ((q[0] + q[3]) + q[5]) / 3.0;
        const double thr = 1e-9 * ((t3 * t3) * t3);
        if (fabs(det) > thr) {
            x[0] = -((c00 * q[6] + c01 * q[7]) + c02 * q[8]) / det;
            x[1] = -((c01 * q[6] + c11 * q[7]) + c12 * q[8]) / det;
            x[2] = -((c02 * q[6] + c12 * q[7]) + c22 * q[8]) / det;
            double dm[3];
            sub3(x, mid, dm);
            sub3(pa, pb, d);
            use = dot3(dm, dm) <= 4.0 * dot3(d, d);
        }
    }
    if (use) {
        cx = quadric_cost(q, x);
    } else {                                                 // the cheapest of p_a, p_b, the midpoint; ties in that order
        const double ca = quadric_cost(q, pa), cb = quadric_cost(q, pb), cm = quadric_cost(q, mid);
        cx = ca;
        for (int k = 0; k < 3; ++k) x[k] = pa[k];
        if (cb < cx) {
            cx = cb;
            for (int k = 0; k < 3; ++k) x[k] = pb[k];
        }
        if (cm < cx) {
            cx = cm;
            for (int k = 0; k < 3; ++k) x[k] = mid[k];
        }
    }
    for (int k = 0; k < 3; ++k) xo[3 * (size_t)e + k] = x[k];
    cost[e] = cx;
    key[e] = (long long)(((unsigned long long)__double_as_longlong(cx) >> 32) << 32) | (long long)e;
    const int ca = vcls[a], cb = vcls[b];
    const bool locked = ((ca | cb) & CLS_LOCKED) != 0;
    const bool pinch = ecnt[e] == 2 && (ca & CLS_BOUNDARY) && (cb & CLS_BOUNDARY);
    valid[e] = (!locked && !pinch && ecnt[e] >= 1 && ecnt[e] <= 2) ? 1 : 0;
}

// ------------------------------------------------------------------ candidates (D6) and the independent set (D7)

__global__ __launch_bounds__(THREADS) void md_m1_init_kernel(const int* __restrict__ f, int n, int V, long long* __restrict__ m1) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int x = f[c];
    if (x >= 0 && x < V) m1[x] = KEY_NONE;
}

struct Fans {
    const int* f;
    const int* node;
    const int* order;
    const int* first;
    const int* last;
    int V, F, U;
};

// corner j of the sorted list -> face t, the corner's position k and the face's vertices; false when out of range
__device__ __forceinline__ bool fan_face(const Fans& m, int j, int& t, int& k, int idx[3]) {
    const int c = m.order[j];
    if (c < 0 || c >= 3 * m.F) return false;
    t = c / 3;
    k = c - 3 * t;
    return load_face(m.f, t, m.V, idx);
}

__device__ __forceinline__ void fan_range(const Fans& m, int u, int& lo, int& hi) {
    lo = max(m.first[u], 0);
    hi = min(m.last[u], 3 * m.F);
}

// does a face of the fan [lo, hi) hold vertex w?
__device__ __forceinline__ bool fan_holds(const Fans& m, int lo, int hi, int w) {
    for (int j = lo; j < hi; ++j) {
        int t, k, idx[3];
        if (!fan_face(m, j, t, k, idx)) continue;
        if (idx[0] == w || idx[1] == w || idx[2] == w) return true;
    }
    return false;
}

// no flip, no null face: n . n' > 0 for the face with corner k moved to x
__device__ __forceinline__ bool keeps_side(const double* __restrict__ p, const int idx[3], int k, const double x[3]) {
    double q[3][3], n0[3], n1[3];
    for (int c = 0; c < 3; ++c) ld3(p, idx[c], q[c]);
    face_g(q[0], q[1], q[2], n0);
    for (int a = 0; a < 3; ++a) q[k][a] = x[a];
    face_g(q[0], q[1], q[2], n1);
    return dot3(n0, n1) > 0.0;
}

// One end of D6: the faces of u that do not hold `other` keep their side.  With `link`: counts the vertices adjacent to
// both ends (each at its first occurrence in u's fan), and no face of `other` may have the same opposite edge.
__device__ bool check_end(const Fans& m, const double* __restrict__ p, int u, int other, const double x[3], bool link,
                          int& common) {
    int lo, hi, olo, ohi;
    fan_range(m, u, lo, hi);
    fan_range(m, other, olo, ohi);
    for (int j = lo; j < hi; ++j) {
        int t, k, idx[3];
        if (!fan_face(m, j, t, k, idx)) return false;
        const int w1 = idx[(k + 1) % 3], w2 = idx[(k + 2) % 3];
        const bool shared = w1 == other || w2 == other;
        if (!shared) {
            if (!keeps_side(p, idx, k, x)) return false;
            if (link) {                                      // the edge opposite u in t against those opposite `other`
                const int oe = m.node[3 * (size_t)t + (k + 1) % 3];
                for (int j2 = olo; j2 < ohi; ++j2) {
                    int t2, k2, idx2[3];
                    if (!fan_face(m, j2, t2, k2, idx2)) return false;
                    if (idx2[(k2 + 1) % 3] == u || idx2[(k2 + 2) % 3] == u) continue;
                    if (m.node[3 * (size_t)t2 + (k2 + 1) % 3] == oe) return false;
                }
            }
        }
        if (!link) continue;
        for (int s = 0; s < 2; ++s) {
            const int w = s ? w2 : w1;
            if (w == other) continue;
            if (!fan_holds(m, lo, j, w) && fan_holds(m, olo, ohi, w)) ++common;
        }
    }
    return true;
}

__global__ __launch_bounds__(THREADS) void md_validate_kernel(Fans m, const double* __restrict__ p,
                                                              const long long* __restrict__ ukeys, const int* __restrict__ ecnt,
                                                              const int* __restrict__ valid, const double* __restrict__ xo,
                                                              const long long* __restrict__ cand, int K,
                                                              long long* __restrict__ m1, int* __restrict__ ok) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= K) return;
    const long long key = cand[i];
    const long long e64 = key & 0xffffffffLL;
    bool good = key >= 0 && e64 < m.U && valid[e64];
    int a = 0, b = 0;
    if (good) {
        const long long uk = ukeys[e64];
        a = (int)(uk / m.V);
        b = (int)(uk % m.V);
        double x[3];
        ld3(xo, (int)e64, x);
        int common = 0, unused = 0;
        good = check_end(m, p, a, b, x, true, common) && common == ecnt[e64] && check_end(m, p, b, a, x, false, unused);
    }
    ok[i] = good ? 1 : 0;
    if (good) {
        atomicMin((unsigned long long*)(m1 + a), (unsigned long long)key);
        atomicMin((unsigned long long*)(m1 + b), (unsigned long long)key);
    }
}

// m2[u] = the smallest m1 over u and its neighbours = over the vertices of u's faces
__device__ __forceinline__ long long fan_min(const Fans& m, const long long* __restrict__ m1, int u) {
    long long r = m1[u];
    int lo, hi;
    fan_range(m, u, lo, hi);
    for (int j = lo; j < hi; ++j) {
        int t, k, idx[3];
        if (!fan_face(m, j, t, k, idx)) continue;
        for (int c = 0; c < 3; ++c) r = min(r, m1[idx[c]]);
    }
    return r;
}

__global__ __launch_bounds__(THREADS) void md_select_kernel(Fans m, const long long* __restrict__ ukeys,
                                                            const long long* __restrict__ cand, const int* __restrict__ ok,
                                                            int K, const long long* __restrict__ m1, int* __restrict__ sel) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= K) return;
    int s = 0;
    if (ok[i]) {
        const long long key = cand[i];
        const long long uk = ukeys[key & 0xffffffffLL];
        const int a = (int)(uk / m.V), b = (int)(uk % m.V);
        s = (fan_min(m, m1, a) == key && fan_min(m, m1, b) == key) ? 1 : 0;
    }
    sel[i] = s;
}

// ------------------------------------------------------------------ budget (D8) and collapse (D9)

__global__ __launch_bounds__(THREADS) void md_weight_kernel(const long long* __restrict__ cand, const int* __restrict__ sel,
                                                            const int* __restrict__ ecnt, int K, int U, int* __restrict__ w) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= K) return;
    const long long e = cand[i] & 0xffffffffLL;
    w[i] = (sel[i] && e < U) ? ecnt[e] : 0;
}

__global__ __launch_bounds__(THREADS) void md_collapse_kernel(Fans m, int* __restrict__ f, double* __restrict__ p,
                                                              double* __restrict__ Q, const long long* __restrict__ ukeys,
                                                              const double* __restrict__ xo, const long long* __restrict__ cand,
                                                              const int* __restrict__ sel, const int* __restrict__ before,
                                                              int K, int target, int* __restrict__ alive,
                                                              int* __restrict__ n_collapsed) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    const bool go = i < K && sel[i] && (cand[i] & 0xffffffffLL) < m.U && m.F - before[i] > target;
    const int n = wave_sum(go ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(n_collapsed, n);
    if (!go) return;
    const long long e = cand[i] & 0xffffffffLL;
    const long long uk = ukeys[e];
    const int a = (int)(uk / m.V), b = (int)(uk % m.V);
    for (int k = 0; k < 3; ++k) p[3 * (size_t)a + k] = xo[3 * (size_t)e + k];
    for (int k = 0; k < 10; ++k) Q[10 * (size_t)a + k] = Q[10 * (size_t)a + k] + Q[10 * (size_t)b + k];
    int lo, hi;
    fan_range(m, b, lo, hi);
    for (int j = lo; j < hi; ++j) {
        const int c = m.order[j];
        if (c < 0 || c >= 3 * m.F) continue;
        const int t = c / 3;
        const int i0 = f[3 * (size_t)t], i1 = f[3 * (size_t)t + 1], i2 = f[3 * (size_t)t + 2];
        if (i0 == a || i1 == a || i2 == a) alive[t] = 0;
        else f[c] = a;
    }
}

__global__ __launch_bounds__(THREADS) void md_gather_rows_kernel(const int* __restrict__ in, const int* __restrict__ rank,
                                                                 int n, int* __restrict__ out) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= n) return;
    const int o = rank[t];
    if (o < 0) return;
    for (int k = 0; k < 3; ++k) out[3 * (size_t)o + k] = in[3 * (size_t)t + k];
}

// ------------------------------------------------------------------ output (D10)

__global__ __launch_bounds__(THREADS) void md_ref_kernel(const int* __restrict__ f, int n, int V, int* __restrict__ ref) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int x = f[c];
    if (x >= 0 && x < V) ref[x] = 1;
}

__global__ __launch_bounds__(THREADS) void md_vertex_out_kernel(const double* __restrict__ p, const int* __restrict__ newid,
                                                                int V, float* __restrict__ out_v, long long* __restrict__ vmap) {
    const int x = blockIdx.x * THREADS + threadIdx.x;
    if (x >= V) return;
    const int o = newid[x];
    if (o < 0) return;
    for (int k = 0; k < 3; ++k) out_v[3 * (size_t)o + k] = (float)p[3 * (size_t)x + k];
    vmap[o] = x;
}

__global__ __launch_bounds__(THREADS) void md_face_out_kernel(const int* __restrict__ f, const int* __restrict__ newid, int n,
                                                              int V, int* __restrict__ out_f) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int x = f[c];
    out_f[c] = (x >= 0 && x < V) ? newid[x] : -1;
}

// ------------------------------------------------------------------ vertex normals of the decimated mesh

__global__ __launch_bounds__(THREADS) void md_normal_kernel(const float* __restrict__ v, const int* __restrict__ f,
                                                            const int* __restrict__ order, const int* __restrict__ first,
                                                            const int* __restrict__ last, int V, int F, float* __restrict__ out) {
    const int x = blockIdx.x * THREADS + threadIdx.x;
    if (x >= V) return;
    double s[3] = {0.0, 0.0, 0.0};
    const int lo = max(first[x], 0), hi = min(last[x], 3 * F);
    for (int j = lo; j < hi; ++j) {
        const int c = order[j];
        if (c < 0 || c >= 3 * F) continue;
        int idx[3];
        if (!load_face(f, c / 3, V, idx)) continue;
        double q[3][3], g[3];
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) q[k][a] = (double)v[3 * (size_t)idx[k] + a];
        face_g(q[0], q[1], q[2], g);
        for (int a = 0; a < 3; ++a) s[a] = s[a] + g[a];
    }
    const double l2 = dot3(s, s);
    const double inv = l2 > 0.0 ? 1.0 / sqrt(l2) : 0.0;
    for (int a = 0; a < 3; ++a) out[3 * (size_t)x + a] = (float)(s[a] * inv);
}

}  // namespace

// ------------------------------------------------------------------ host side
namespace {

// 4 int regions of M entries, 2 pairs of totals, no change flags; small() holds the collapse counter
using Ws = MeshWs<4, 2, 0>;

int64_t items(int V, int F) { return std::max<int64_t>({(int64_t)V, 3 * (int64_t)F, 1}); }

int check_sizes(const char* name, int V, int F) {
    PRIMX_REQUIRE(V >= 0 && F >= 0, "%s: need V, F >= 0 (got %d, %d)", name, V, F);
    PRIMX_REQUIRE(10 * (int64_t)V < I31 && 9 * (int64_t)F < I31, "%s: 10 * V and 9 * F must be < 2^31 (got V = %d, F = %d)",
                  name, V, F);
    return PRIMX_OK;
}

int check_edges(const char* name, int F, int U) {
    PRIMX_REQUIRE(U >= 0 && U <= 3 * (int64_t)F, "%s: need 0 <= U <= 3 F (got U = %d, F = %d)", name, U, F);
    return PRIMX_OK;
}

}  // namespace

extern "C" int primx_meshdecim_workspace(int V, int F, int64_t* bytes) {
    PRIMX_REQUIRE(bytes, "primx_meshdecim_workspace: null pointer");
    PRIMX_TRY(check_sizes("primx_meshdecim_workspace", V, F));
    *bytes = (int64_t)Ws(items(V, F)).total;
    return PRIMX_OK;
}

extern "C" int primx_meshdecim_edges(const int* f, const int* node, const int* sv, int V, int F, int U, int* ecnt, int* vcls,
                                     int* first, int* last, void* stream) {
    const char* name = "primx_meshdecim_edges";
    PRIMX_TRY(check_sizes(name, V, F));
    PRIMX_TRY(check_edges(name, F, U));
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(f && node && sv && ecnt && vcls && first && last, "%s: null pointer", name);
    PRIMX_REQUIRE(V >= 1 && U >= 1, "%s: faces without vertices or edges", name);
    hipStream_t st = (hipStream_t)stream;
    const int n = 3 * F, nb = nblocks(n, THREADS);
    PRIMX_TRY(fill(ecnt, U, 0, st, name));
    hipLaunchKernelGGL(md_corner_init_kernel, dim3(nb), dim3(THREADS), 0, st, f, n, V, vcls);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(md_edge_count_kernel, dim3(nb), dim3(THREADS), 0, st, node, n, U, ecnt);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(md_ranges_kernel, dim3(nb), dim3(THREADS), 0, st, sv, n, V, first, last);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(md_class_kernel, dim3(nb), dim3(THREADS), 0, st, f, node, n, V, U, (const int*)ecnt, vcls);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_meshdecim_quadrics(const float* v, const int* f, const int* node, const int* order, const int* first,
                                        const int* last, const int* ecnt, int V, int F, int U, double* p, double* Q,
                                        void* stream) {
    const char* name = "primx_meshdecim_quadrics";
    PRIMX_TRY(check_sizes(name, V, F));
    PRIMX_TRY(check_edges(name, F, U));
    if (V == 0) return PRIMX_OK;
    PRIMX_REQUIRE(v && first && last && p && Q && (F == 0 || (f && node && order && ecnt)), "%s: null pointer", name);
    hipLaunchKernelGGL(md_quadric_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, v, f, node, order,
                       first, last, ecnt, V, F, U, p, Q);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_meshdecim_costs(const double* p, const double* Q, const int64_t* ukeys, const int* ecnt, const int* vcls,
                                     int V, int U, int optimalplacement, double* x, double* cost, int64_t* key, int* valid,
                                     void* stream) {
    const char* name = "primx_meshdecim_costs";
    PRIMX_TRY(check_sizes(name, V, 0));
    PRIMX_REQUIRE(U >= 0 && 3 * (int64_t)U < I31, "%s: need 0 <= 3 U < 2^31 (got U = %d)", name, U);
    if (U == 0) return PRIMX_OK;
    PRIMX_REQUIRE(p && Q && ukeys && ecnt && vcls && x && cost && key && valid, "%s: null pointer", name);
    PRIMX_REQUIRE(V >= 2, "%s: edges without vertices (V = %d)", name, V);
    hipLaunchKernelGGL(md_cost_kernel, dim3(nblocks(U, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, p, Q,
                       (const long long*)ukeys, ecnt, vcls, V, U, optimalplacement ? 1 : 0, x, cost, (long long*)key, valid);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_meshdecim_select(const double* p, const int* f, const int* node, const int* order, const int* first,
                                      const int* last, const int64_t* ukeys, const int* ecnt, const int* valid,
                                      const double* x, const int64_t* cand, int V, int F, int U, int K, int64_t* m1, int* ok,
                                      int* sel, void* stream) {
    const char* name = "primx_meshdecim_select";
    PRIMX_TRY(check_sizes(name, V, F));
    PRIMX_TRY(check_edges(name, F, U));
    PRIMX_REQUIRE(K >= 0 && K <= U, "%s: need 0 <= K <= U (got K = %d, U = %d)", name, K, U);
    if (K == 0) return PRIMX_OK;
    PRIMX_REQUIRE(p && f && node && order && first && last && ukeys && ecnt && valid && x && cand && m1 && ok && sel,
                  "%s: null pointer", name);
    PRIMX_REQUIRE(V >= 2, "%s: edges without vertices (V = %d)", name, V);
    hipStream_t st = (hipStream_t)stream;
    const Fans m{f, node, order, first, last, V, F, U};
    hipLaunchKernelGGL(md_m1_init_kernel, dim3(nblocks(3 * (int64_t)F, THREADS)), dim3(THREADS), 0, st, f, 3 * F, V,
                       (long long*)m1);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(md_validate_kernel, dim3(nblocks(K, THREADS)), dim3(THREADS), 0, st, m, p, (const long long*)ukeys, ecnt,
                       valid, x, (const long long*)cand, K, (long long*)m1, ok);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(md_select_kernel, dim3(nblocks(K, THREADS)), dim3(THREADS), 0, st, m, (const long long*)ukeys,
                       (const long long*)cand, (const int*)ok, K, (const long long*)m1, sel);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_meshdecim_collapse(double* p, double* Q, int* f, const int* order, const int* first, const int* last,
                                        const int64_t* ukeys, const int* ecnt, const double* x, const int64_t* cand,
                                        const int* sel, int V, int F, int U, int K, int target, void* ws, int64_t ws_bytes,
                                        int* out_f, int64_t* counts, void* stream) {
    const char* name = "primx_meshdecim_collapse";
    PRIMX_REQUIRE(counts, "%s: null pointer", name);
    PRIMX_TRY(check_sizes(name, V, F));
    PRIMX_TRY(check_edges(name, F, U));
    PRIMX_REQUIRE(K >= 0 && K <= U && target >= 0, "%s: need 0 <= K <= U and target >= 0 (got K = %d, U = %d, target = %d)", name,
                  K, U, target);
    counts[0] = 0;
    counts[1] = F;
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(p && Q && f && order && first && last && ukeys && ecnt && x && out_f && (K == 0 || (cand && sel)),
                  "%s: null pointer", name);
    Ws w;
    PRIMX_TRY(check_ws(name, items(V, F), ws, ws_bytes, w));
    hipStream_t st = (hipStream_t)stream;
    int *weight = w.R(0), *before = w.R(1), *alive = w.R(2), *rank = w.R(3), *n_collapsed = w.small();
    PRIMX_TRY(fill(alive, F, 1, st, name));
    PRIMX_TRY(fill(n_collapsed, 1, 0, st, name));
    if (K > 0) {
        hipLaunchKernelGGL(md_weight_kernel, dim3(nblocks(K, THREADS)), dim3(THREADS), 0, st, (const long long*)cand, sel, ecnt, K,
                           U, weight);
        PRIMX_CHECK_LAUNCH(name);
        PRIMX_TRY(scan(weight, K, false, before, nullptr, w.bsum(), w.tot(1), st, name));
        const Fans m{f, nullptr, order, first, last, V, F, U};
        hipLaunchKernelGGL(md_collapse_kernel, dim3(nblocks(K, THREADS)), dim3(THREADS), 0, st, m, f, p, Q,
                           (const long long*)ukeys, x, (const long long*)cand, sel, (const int*)before, K, target, alive,
                           n_collapsed);
        PRIMX_CHECK_LAUNCH(name);
    }
    PRIMX_TRY(scan(alive, F, true, rank, nullptr, w.bsum(), w.tot(0), st, name));
    hipLaunchKernelGGL(md_gather_rows_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, (const int*)f, (const int*)rank, F,
                       out_f);
    PRIMX_CHECK_LAUNCH(name);
    long long h[2];
    int hc = 0;
    PRIMX_TRY(readback(h, w.tot(0), sizeof(h), st, name));
    PRIMX_TRY(readback(&hc, n_collapsed, sizeof(hc), st, name));
    counts[0] = hc;     // collapses of the round
    counts[1] = h[0];   // live faces after it
    return PRIMX_OK;
}

extern "C" int primx_meshdecim_finish(const double* p, const int* f, int V, int F, void* ws, int64_t ws_bytes, float* out_v,
                                      int* out_f, int64_t* vmap, int64_t* n_out, void* stream) {
    const char* name = "primx_meshdecim_finish";
    PRIMX_REQUIRE(n_out, "%s: null pointer", name);
    PRIMX_TRY(check_sizes(name, V, F));
    *n_out = 0;
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(V >= 1, "%s: faces without vertices (V = 0)", name);
    PRIMX_REQUIRE(p && f && out_v && out_f && vmap, "%s: null pointer", name);
    Ws w;
    PRIMX_TRY(check_ws(name, items(V, F), ws, ws_bytes, w));
    hipStream_t st = (hipStream_t)stream;
    int *ref = w.R(0), *newid = w.R(1);
    const int n = 3 * F;
    PRIMX_TRY(fill(ref, V, 0, st, name));
    hipLaunchKernelGGL(md_ref_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, f, n, V, ref);
    PRIMX_CHECK_LAUNCH(name);
    PRIMX_TRY(scan(ref, V, true, newid, nullptr, w.bsum(), w.tot(0), st, name));
    hipLaunchKernelGGL(md_vertex_out_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, st, p, (const int*)newid, V, out_v,
                       (long long*)vmap);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(md_face_out_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, f, (const int*)newid, n, V, out_f);
    PRIMX_CHECK_LAUNCH(name);
    long long h[2];
    PRIMX_TRY(readback(h, w.tot(0), sizeof(h), st, name));
    *n_out = h[0];
    return PRIMX_OK;
}

extern "C" int primx_meshdecim_normals(const float* v, const int* f, const int* sv, const int* order, int V, int F, void* ws,
                                       int64_t ws_bytes, float* normals, void* stream) {
    const char* name = "primx_meshdecim_normals";
    PRIMX_TRY(check_sizes(name, V, F));
    if (V == 0) {
        PRIMX_REQUIRE(F == 0, "%s: faces without vertices (V = 0)", name);
        return PRIMX_OK;
    }
    PRIMX_REQUIRE(v && normals && (F == 0 || (f && sv && order)), "%s: null pointer", name);
    Ws w;
    PRIMX_TRY(check_ws(name, items(V, F), ws, ws_bytes, w));
    hipStream_t st = (hipStream_t)stream;
    int *first = w.R(0), *last = w.R(1);
    PRIMX_TRY(fill(first, V, 0, st, name));
    PRIMX_TRY(fill(last, V, 0, st, name));
    if (F > 0) {
        hipLaunchKernelGGL(md_ranges_kernel, dim3(nblocks(3 * (int64_t)F, THREADS)), dim3(THREADS), 0, st, sv, 3 * F, V, first,
                           last);
        PRIMX_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(md_normal_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, st, v, f, order, (const int*)first,
                       (const int*)last, V, F, normals);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}
