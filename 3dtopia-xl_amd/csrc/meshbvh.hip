// Mesh BVH (no counterpart in the reference): the mesh field query of meshfield.hip through a bounding volume hierarchy - the
// same dist, face and out_attr bit for bit, the winding number by the far-field expansion of Barill et al. 2018 ("Fast winding
// numbers for soups and clouds").  Rules and the C ABI: include/primx_hip.h "Mesh BVH"; restatement: tests/meshbvh_numpy.py.
//
//   keys:   the vertices' bounding box and largest absolute coordinate by a two-stage reduction (per-block partials, then one
//           block), then one 64-bit key per face: its centroid's 30-bit Morton code above its own index.  The caller sorts.
//   tree:   the records of meshfield_pair.h in sorted order, 8 to a leaf; over the leaves an implicit complete binary tree
//           (node 1 the root, 2 i and 2 i + 1 the children of i, the leaves at L .. 2 L - 1, L the leaf count rounded up to a
//           power of two).  One thread per leaf, then one launch per level, every node from its two children: no atomics on
//           the tree and a fixed order of every float64 sum, so two builds give the same bits.
//   query:  one thread per point (64-bit point index).  Two walks without a stack: the node index itself tells where to go
//           next (up while the node is the second child of its parent, then to the sibling: a count of trailing bits), so
//           no thread keeps an array.  The distance walk visits the nearer child first and keeps, one bit per level, which
//           child that was; the winding walk goes left first.
//   rays:   one thread per ray, or per point with a table of directions ("Mesh rays" R1-R6; restatement: tests/meshray_numpy.py):
//           the distance walk's way through the tree with the watertight ray / triangle test and the box test of meshray_pair.h.
//
// Every floating-point expression is evaluated as written (no contraction).
#include <cmath>
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_common.h"

#include "meshfield_pair.h"

#include "meshray_pair.h"

constexpr int LEAF = 8;                  // faces per leaf
constexpr int NODE_F4 = 6;               // float4 per node (96 bytes)
constexpr int MOM = 16;                  // doubles per node of build scratch: N [3], sum of areas, sum of area * centroid [3], M [9]
constexpr int BB_MAXB = 256;             // blocks of the bounding-box reduction at most
constexpr int BB_PER_BLOCK = 4096;       // vertices per block at least
constexpr float DELTA_SCALE = 0x1p-17f;  // the boxes' inflation: delta = DELTA_SCALE * the largest |coordinate| of the mesh
constexpr int64_t HEAD = 256;            // status (int) at 0; lo [3], hi [3], maxabs, delta (floats) at 64

// node i, six float4: (lo.x, lo.y, lo.z, hi.x) (hi.y, hi.z, r, faces below as int: 0 = empty) (p.x, p.y, p.z, N.x)
// (N.y, N.z, C00, C01) (C02, C10, C11, C12) (C20, C21, C22, 0)
struct Layout {
    int nleaf, L;
    int64_t recs, orig, nodes, mom, part, total;
};

inline Layout layout(int F) {
    Layout o;
    o.nleaf = (F + LEAF - 1) / LEAF;
    o.L = 1;
    while (o.L < o.nleaf) o.L *= 2;
    auto up = [](int64_t x) { return (x + 15) & ~(int64_t)15; };
    o.recs = HEAD;
    o.orig = o.recs + (int64_t)64 * F;
    o.nodes = o.orig + up((int64_t)4 * F);
    o.mom = o.nodes + (int64_t)NODE_F4 * 16 * 2 * o.L;
    o.part = o.mom + (int64_t)MOM * 8 * 2 * o.L;
    o.total = o.part + (int64_t)BB_MAXB * 8 * 4;
    return o;
}

// ------------------------------------------------------------------------------------------------ bounding box, keys
__device__ __forceinline__ float block_minf(float x, float* red) {
    for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    x = red[0];
    for (int w = 1; w < THREADS / 64; ++w) x = fminf(x, red[w]);
    return x;
}

// block b: min and max of the coordinates of its slice of the vertices -> part[8 b + 0 .. 5]
__global__ __launch_bounds__(THREADS) void bb_part_kernel(const float* __restrict__ v, int V, int per, float* __restrict__ part) {
    __shared__ float red[THREADS / 64];
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < V ? lo + per : V;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) mn[k] = fminf(mn[k], v[3 * i + k]), mx[k] = fmaxf(mx[k], v[3 * i + k]);
    }
    float out[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = block_minf(mn[k], red), out[3 + k] = -block_minf(-mx[k], red);
    if (threadIdx.x == 0) {
        float* o = part + 8 * blockIdx.x;
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = out[k];
    }
}

// one block: the partials of nblk blocks -> head[0 .. 7] = lo, hi, the largest |coordinate|, delta
__global__ __launch_bounds__(THREADS) void bb_final_kernel(const float* __restrict__ part, int nblk, float* __restrict__ head) {
    __shared__ float red[THREADS / 64];
    const bool have = (int)threadIdx.x < nblk;
    float out[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[k] = block_minf(have ? part[8 * threadIdx.x + k] : INFINITY, red);
        out[3 + k] = -block_minf(have ? -part[8 * threadIdx.x + 3 + k] : INFINITY, red);
    }
    if (threadIdx.x == 0) {
        float m = 0.0f;
#pragma unroll
        for (int k = 0; k < 6; ++k) head[k] = out[k], m = fmaxf(m, fabsf(out[k]));
        head[6] = m;
        head[7] = m * DELTA_SCALE;
    }
}

__device__ __forceinline__ unsigned spread10(unsigned x) {  // bit k of x -> bit 3 k
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__device__ __forceinline__ unsigned quant(float c, float lo, float s) {
    return (unsigned)(int)fminf(fmaxf((c - lo) * s, 0.0f), 1023.0f);     // a NaN gives 0
}

__global__ __launch_bounds__(THREADS) void key_kernel(const float* __restrict__ v, const int* __restrict__ f, int V, int F,
                                                      const float* __restrict__ head, long long* __restrict__ keys) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    const int i0 = f[(int64_t)3 * t], i1 = f[(int64_t)3 * t + 1], i2 = f[(int64_t)3 * t + 2];
    unsigned code = 0;
    if (!(i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V)) {      // (the tree pass refuses the others)
        const float ext = fmaxf(fmaxf(head[3] - head[0], head[4] - head[1]), head[5] - head[2]);
        const float s = ext > 0.0f ? 1024.0f / ext : 0.0f;
        unsigned q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = ((v[(int64_t)3 * i0 + k] + v[(int64_t)3 * i1 + k]) + v[(int64_t)3 * i2 + k]) / 3.0f;
            q[k] = quant(c, head[k], s);
        }
        code = (spread10(q[0]) << 2) | (spread10(q[1]) << 1) | spread10(q[2]);
    }
    keys[t] = (long long)(((unsigned long long)code << 32) | (unsigned)t);
}

// ------------------------------------------------------------------------------------------------ the tree
__device__ __forceinline__ void write_empty(float4* __restrict__ nd, double* __restrict__ mom) {
    nd[0] = float4{INFINITY, INFINITY, INFINITY, -INFINITY};
    nd[1] = float4{-INFINITY, -INFINITY, 0.0f, __int_as_float(0)};
    const float4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    nd[2] = z, nd[3] = z, nd[4] = z, nd[5] = z;
    for (int k = 0; k < MOM; ++k) mom[k] = 0.0;
}

// the node from its (inflated) box, its float64 sums and its face count: every moment rounded to fp32 once, here
__device__ __forceinline__ void write_node(float4* __restrict__ nd, double* __restrict__ mom, const float* lo, const float* hi,
                                           const double* m, int count) {
    double p[3];
    for (int k = 0; k < 3; ++k) p[k] = m[3] > 0.0 ? m[4 + k] / m[3] : 0.5 * ((double)lo[k] + (double)hi[k]);
    double e[3];
    for (int k = 0; k < 3; ++k) e[k] = fmax(p[k] - (double)lo[k], (double)hi[k] - p[k]);
    const double r = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    float c[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (float)(m[7 + 3 * i + j] - p[i] * m[j]);
    nd[0] = float4{lo[0], lo[1], lo[2], hi[0]};
    nd[1] = float4{hi[1], hi[2], (float)r, __int_as_float(count)};
    nd[2] = float4{(float)p[0], (float)p[1], (float)p[2], (float)m[0]};
    nd[3] = float4{(float)m[1], (float)m[2], c[0], c[1]};
    nd[4] = float4{c[2], c[3], c[4], c[5]};
    nd[5] = float4{c[6], c[7], c[8], 0.0f};
    for (int k = 0; k < MOM; ++k) mom[k] = m[k];
}

// one thread per leaf slot l < L: node L + l from the records 8 l .. 8 l + 7 (those below F), in that order
__global__ __launch_bounds__(THREADS) void leaf_kernel(const float4* __restrict__ recs, int F, int nleaf, int L,
                                                       const float* __restrict__ head, float4* __restrict__ nodes,
                                                       double* __restrict__ moms) {
    const int l = blockIdx.x * THREADS + threadIdx.x;
    if (l >= L) return;
    float4* nd = nodes + (int64_t)NODE_F4 * (L + l);
    double* mom = moms + (int64_t)MOM * (L + l);
    if (l >= nleaf) {
        write_empty(nd, mom);
        return;
    }
    const float delta = head[7];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double m[MOM];
    for (int k = 0; k < MOM; ++k) m[k] = 0.0;
    const int first = LEAF * l, cnt = min(LEAF, F - first);
    for (int j = 0; j < cnt; ++j) {
        const Rec r = unpack(recs + (int64_t)4 * (first + j));
        if (r.kind < 0) continue;                            // an index out of range: the host refuses the call
        const float a[3] = {r.ax, r.ay, r.az}, b[3] = {r.bx, r.by, r.bz}, c[3] = {r.cx, r.cy, r.cz};
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], fminf(a[k], fminf(b[k], c[k])));
            hi[k] = fmaxf(hi[k], fmaxf(a[k], fmaxf(b[k], c[k])));
        }
        if (r.kind != 0) continue;                           // a zero-area face: in the box, nothing in the moments
        double ab[3], ac[3], cen[3];
        for (int k = 0; k < 3; ++k) {
            ab[k] = (double)b[k] - (double)a[k], ac[k] = (double)c[k] - (double)a[k];
            cen[k] = (((double)a[k] + (double)b[k]) + (double)c[k]) / 3.0;
        }
        const double A[3] = {0.5 * (ab[1] * ac[2] - ab[2] * ac[1]), 0.5 * (ab[2] * ac[0] - ab[0] * ac[2]),
                             0.5 * (ab[0] * ac[1] - ab[1] * ac[0])};
        const double ar = sqrt((A[0] * A[0] + A[1] * A[1]) + A[2] * A[2]);
        for (int k = 0; k < 3; ++k) m[k] += A[k], m[4 + k] += ar * cen[k];
        m[3] += ar;
        for (int i = 0; i < 3; ++i)
            for (int k = 0; k < 3; ++k) m[7 + 3 * i + k] += cen[i] * A[k];
    }
    for (int k = 0; k < 3; ++k) lo[k] = lo[k] - delta, hi[k] = hi[k] + delta;
    write_node(nd, mom, lo, hi, m, cnt);
}

// one thread per node of one level (first .. 2 first - 1): the union of the children's boxes, left + right of their sums
__global__ __launch_bounds__(THREADS) void level_kernel(int first, float4* __restrict__ nodes, double* __restrict__ moms) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= first) return;
    const int64_t i = (int64_t)first + t;
    const float4 a0 = nodes[NODE_F4 * 2 * i], a1 = nodes[NODE_F4 * 2 * i + 1];
    const float4 b0 = nodes[NODE_F4 * (2 * i + 1)], b1 = nodes[NODE_F4 * (2 * i + 1) + 1];
    const int ca = __float_as_int(a1.w), cb = __float_as_int(b1.w);
    float4* nd = nodes + NODE_F4 * i;
    double* mom = moms + MOM * i;
    if (ca + cb == 0) {
        write_empty(nd, mom);
        return;
    }
    // (an empty child's box is (+inf, -inf) and its sums are 0)
    const float lo[3] = {fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z)};
    const float hi[3] = {fmaxf(a0.w, b0.w), fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y)};
    double m[MOM];
    for (int k = 0; k < MOM; ++k) m[k] = moms[MOM * 2 * i + k] + moms[MOM * (2 * i + 1) + k];
    write_node(nd, mom, lo, hi, m, ca + cb);
}

__global__ __launch_bounds__(THREADS) void orig_kernel(const int* __restrict__ order, int F, int* __restrict__ orig) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t < F) orig[t] = order[t];
}

// ------------------------------------------------------------------------------------------------ the query
// the fp32 squared distance from p to the box, as written: per axis max(lo - p, p - hi, 0), then dot3 of that with itself
__device__ __forceinline__ float box_d2(float px, float py, float pz, const float4& q0, const float4& q1) {
    const float dx = fmaxf(fmaxf(q0.x - px, px - q0.w), 0.0f);
    const float dy = fmaxf(fmaxf(q0.y - py, py - q1.x), 0.0f);
    const float dz = fmaxf(fmaxf(q0.z - pz, pz - q1.y), 0.0f);
    return dot3(dx, dy, dz, dx, dy, dz);
}

__global__ __launch_bounds__(THREADS) void bvh_query_kernel(const float* __restrict__ pts, int64_t n,
                                                            const float4* __restrict__ recs, const int* __restrict__ orig,
                                                            const float4* __restrict__ nodes, int L, int F,
                                                            const int* __restrict__ f, const float* __restrict__ attr, int C,
                                                            float beta, float* __restrict__ dist, int* __restrict__ face,
                                                            float* __restrict__ wn, float* __restrict__ out_attr) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];

    // ---- distance: depth first, the nearer child first; bit k of `trail` (from the node's own level upwards) = the right
    // child went first there, so node ^ trail has a 1 wherever the walk is in a second child
    float best = INFINITY;
    int bf = 0, bs = 0;                                      // the winner's face index and its place in the sorted records
    unsigned node = 1, trail = 0;
    while (true) {
        const float4 q0 = nodes[(int64_t)NODE_F4 * node], q1 = nodes[(int64_t)NODE_F4 * node + 1];
        bool descend = false;
        if (__float_as_int(q1.w) != 0 && !(box_d2(px, py, pz, q0, q1) > best)) {     // skipped only when lb2 > best, strictly
            if (node >= (unsigned)L) {
                const int first = LEAF * (int)(node - (unsigned)L), cnt = min(LEAF, F - first);
                for (int j = 0; j < cnt; ++j) {
                    const Rec r = unpack(recs + (int64_t)4 * (first + j));
                    float d2, v, w, term;
                    pair(px, py, pz, r, r.kind, d2, v, w, term);
                    const int of = orig[first + j];
                    if (d2 < best || (d2 == best && of < bf)) best = d2, bf = of, bs = first + j;   // (d2, face), lexicographic
                }
            } else {
                descend = true;
            }
        }
        if (descend) {
            const float4* c = nodes + (int64_t)NODE_F4 * 2 * node;
            const float4 l0 = c[0], l1 = c[1], r0 = c[NODE_F4], r1 = c[NODE_F4 + 1];
            const float dl = __float_as_int(l1.w) != 0 ? box_d2(px, py, pz, l0, l1) : INFINITY;
            const float dr = __float_as_int(r1.w) != 0 ? box_d2(px, py, pz, r0, r1) : INFINITY;
            const unsigned right_first = dr < dl ? 1u : 0u;
            node = 2 * node + right_first;
            trail = 2 * trail + right_first;
        } else {
            unsigned u = (node ^ trail) + 1;                 // up past every second child, then to the sibling
            const int s = __builtin_ctz(u);
            u >>= s;
            if (u == 1) break;
            trail >>= s;
            node = u ^ trail;
        }
    }

    // ---- winding number: left first; a node farther than beta r from p adds its expansion, a nearer one is opened
    float acc = 0.0f;
    node = 1;
    while (true) {
        const float4 q1 = nodes[(int64_t)NODE_F4 * node + 1];
        bool descend = false;
        if (__float_as_int(q1.w) != 0) {
            const float4 q2 = nodes[(int64_t)NODE_F4 * node + 2];
            const float x = q2.x - px, y = q2.y - py, z = q2.z - pz;
            const float d2 = dot3(x, y, z, x, y, z);
            const float br = beta * q1.z;
            if (d2 <= br * br) {
                if (node >= (unsigned)L) {
                    const int first = LEAF * (int)(node - (unsigned)L), cnt = min(LEAF, F - first);
                    for (int j = 0; j < cnt; ++j) {
                        const Rec r = unpack(recs + (int64_t)4 * (first + j));
                        float e2, v, w, term;
                        pair(px, py, pz, r, r.kind, e2, v, w, term);
                        acc += term;
                    }
                } else {
                    descend = true;
                }
            } else {
                const float4 q3 = nodes[(int64_t)NODE_F4 * node + 3], q4 = nodes[(int64_t)NODE_F4 * node + 4],
                             q5 = nodes[(int64_t)NODE_F4 * node + 5];
                const float d = sqrtf(d2), d3 = d2 * d, d5 = d3 * d2;
                const float nx = dot3(q2.w, q3.x, q3.y, x, y, z);
                const float tr = (q3.z + q4.z) + q5.z;
                const float cx = dot3(q3.z, q3.w, q4.x, x, y, z), cy = dot3(q4.y, q4.z, q4.w, x, y, z),
                            cz = dot3(q5.x, q5.y, q5.z, x, y, z);
                const float xcx = dot3(x, y, z, cx, cy, cz);
                const float omega = (nx / d3 + tr / d3) - (3.0f * xcx) / d5;
                acc += 0.5f * omega;
            }
        }
        if (descend) {
            node = 2 * node;
        } else {
            unsigned u = node + 1;
            u >>= __builtin_ctz(u);
            if (u == 1) break;
            node = u;
        }
    }

    dist[i] = sqrtf(best);
    face[i] = bf;
    wn[i] = acc * 0.15915494309189535f;                      // 2 sum / (4 pi)
    if (C > 0) {
        const Rec r = unpack(recs + (int64_t)4 * bs);
        float d2, v, w, term;
        pair(px, py, pz, r, r.kind, d2, v, w, term);
        const float u = (1.0f - v) - w;
        const float* ga = attr + (int64_t)f[(int64_t)3 * bf] * C;
        const float* gb = attr + (int64_t)f[(int64_t)3 * bf + 1] * C;
        const float* gc = attr + (int64_t)f[(int64_t)3 * bf + 2] * C;
        for (int c = 0; c < C; ++c) out_attr[i * C + c] = (ga[c] * u + gb[c] * v) + gc[c] * w;
    }
}

// ------------------------------------------------------------------------------------------------ rays ("Mesh rays", R1-R6)
// The closest accepted record along one ray, or with `any` the first one met: the distance walk's way through the tree (no
// stack: node and trail), the child whose interval starts nearer first, a node skipped only when ray_box refuses it.
__device__ __forceinline__ void ray_walk(const Ray& q, float tmin, float tmax, bool any, const float4* __restrict__ recs,
                                         const int* __restrict__ orig, const float4* __restrict__ nodes, int L, int F, float& bt,
                                         int& bf, float& bv, float& bw) {
    bt = tmax, bf = -1, bv = 0.0f, bw = 0.0f;
    if (!q.ok) return;
    unsigned node = 1, trail = 0;
    while (true) {
        const float4 q0 = nodes[(int64_t)NODE_F4 * node], q1 = nodes[(int64_t)NODE_F4 * node + 1];
        bool descend = false;
        float tn;
        if (__float_as_int(q1.w) != 0 && ray_box(q, q0, q1, tmin, bt, tn)) {
            if (node >= (unsigned)L) {
                const int first = LEAF * (int)(node - (unsigned)L), cnt = min(LEAF, F - first);
                for (int j = 0; j < cnt; ++j) {
                    const Rec r = unpack(recs + (int64_t)4 * (first + j));
                    float t, v, w;
                    if (!ray_pair(q, r, tmin, tmax, t, v, w)) continue;
                    const int of = orig[first + j];
                    if (bf < 0 || t < bt || (t == bt && of < bf)) bt = t, bf = of, bv = v, bw = w;   // (t, face), lexicographic
                }
                if (any && bf >= 0) break;
            } else {
                descend = true;
            }
        }
        if (descend) {
            const float4* c = nodes + (int64_t)NODE_F4 * 2 * node;
            const float4 l0 = c[0], l1 = c[1], r0 = c[NODE_F4], r1 = c[NODE_F4 + 1];
            float tl, tr;
            const bool hl = __float_as_int(l1.w) != 0 && ray_box(q, l0, l1, tmin, bt, tl);
            const bool hr = __float_as_int(r1.w) != 0 && ray_box(q, r0, r1, tmin, bt, tr);
            const unsigned right_first = hr && (!hl || tr < tl) ? 1u : 0u;
            node = 2 * node + right_first;
            trail = 2 * trail + right_first;
        } else {
            unsigned u = (node ^ trail) + 1;                 // up past every second child, then to the sibling
            const int s = __builtin_ctz(u);
            u >>= s;
            if (u == 1) break;
            trail >>= s;
            node = u ^ trail;
        }
    }
}

__global__ __launch_bounds__(THREADS) void bvh_raycast_kernel(const float* __restrict__ org, const float* __restrict__ dir, int64_t n,
                                                              float tmin, float tmax, int any, const float4* __restrict__ recs,
                                                              const int* __restrict__ orig, const float4* __restrict__ nodes, int L,
                                                              int F, float* __restrict__ t, int* __restrict__ face,
                                                              float* __restrict__ bary) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const Ray q = ray_setup(org[3 * i], org[3 * i + 1], org[3 * i + 2], dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
    float bt, bv, bw;
    int bf;
    ray_walk(q, tmin, tmax, any != 0, recs, orig, nodes, L, F, bt, bf, bv, bw);
    t[i] = bf >= 0 ? bt : INFINITY;
    face[i] = bf;
    bary[2 * i] = bv, bary[2 * i + 1] = bw;
}

// one thread per point: an any-hit ray along each direction in turn, tmax = inf; the number that met nothing, up to `limit`
__global__ __launch_bounds__(THREADS) void bvh_visibility_kernel(const float* __restrict__ pts, int64_t n,
                                                                 const float* __restrict__ dirs, int D, float tmin, int limit,
                                                                 const float4* __restrict__ recs, const int* __restrict__ orig,
                                                                 const float4* __restrict__ nodes, int L, int F,
                                                                 int* __restrict__ escapes) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    int esc = 0;
    for (int k = 0; k < D; ++k) {
        const Ray q = ray_setup(px, py, pz, dirs[3 * k], dirs[3 * k + 1], dirs[3 * k + 2]);
        float bt, bv, bw;
        int bf;
        ray_walk(q, tmin, INFINITY, true, recs, orig, nodes, L, F, bt, bf, bv, bw);
        if (bf < 0) ++esc;
        if (limit > 0 && esc >= limit) break;
    }
    escapes[i] = esc;
}

int bounding_box(const float* v, int V, char* ws, const Layout& lay, hipStream_t st, const char* name) {
    int per = (V + BB_MAXB - 1) / BB_MAXB;
    if (per < BB_PER_BLOCK) per = BB_PER_BLOCK;
    const int nblk = (V + per - 1) / per;
    float* part = (float*)(ws + lay.part);
    hipLaunchKernelGGL(bb_part_kernel, dim3(nblk), dim3(THREADS), 0, st, v, V, per, part);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(bb_final_kernel, dim3(1), dim3(THREADS), 0, st, (const float*)part, nblk, (float*)(ws + 64));
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

}  // namespace

extern "C" int primx_mesh_bvh_workspace(int F, int64_t* bytes) {
    PRIMX_REQUIRE(bytes, "primx_mesh_bvh_workspace: null pointer");
    PRIMX_REQUIRE(F >= 1 && F <= INT32_MAX / 4, "primx_mesh_bvh_workspace: F must lie in 1 .. (2^31 - 1) / 4 (got %d)", F);
    *bytes = layout(F).total;
    return PRIMX_OK;
}

extern "C" int primx_mesh_bvh_build(const float* v, const int* f, int V, int F, const int* order, int64_t* keys, void* ws,
                                    int64_t ws_bytes, void* stream) {
    const char* name = "primx_mesh_bvh_build";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_TRY(check_mesh(name, v, f, V, F));
    const Layout lay = layout(F);
    PRIMX_REQUIRE(ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= lay.total,
                  "%s: the workspace needs primx_mesh_bvh_workspace(F) = %lld bytes, 16-byte aligned", name, (long long)lay.total);
    PRIMX_REQUIRE(order || keys, "%s: give keys (the key pass) or order (the tree pass)", name);
    char* w = (char*)ws;
    PRIMX_TRY(bounding_box(v, V, w, lay, st, name));
    const float* head = (const float*)(w + 64);
    if (!order) {                                            // the key pass: nothing is read back
        hipLaunchKernelGGL(key_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, v, f, V, F, head, (long long*)keys);
        PRIMX_CHECK_LAUNCH(name);
        return PRIMX_OK;
    }
    int* status = (int*)w;
    float4* recs = (float4*)(w + lay.recs);
    float4* nodes = (float4*)(w + lay.nodes);
    double* moms = (double*)(w + lay.mom);
    PRIMX_TRY(zero(status, sizeof(int), st, name));
    hipLaunchKernelGGL(mf_prep_kernel<true>, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, v, f, V, F, order, recs, status);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(orig_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, order, F, (int*)(w + lay.orig));
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(leaf_kernel, dim3(nblocks(lay.L, THREADS)), dim3(THREADS), 0, st, (const float4*)recs, F, lay.nleaf, lay.L,
                       head, nodes, moms);
    PRIMX_CHECK_LAUNCH(name);
    for (int first = lay.L / 2; first >= 1; first /= 2) {
        hipLaunchKernelGGL(level_kernel, dim3(nblocks(first, THREADS)), dim3(THREADS), 0, st, first, nodes, moms);
        PRIMX_CHECK_LAUNCH(name);
    }
    int flag = 0;
    PRIMX_TRY(readback(&flag, status, sizeof(flag), st, name));
    PRIMX_REQUIRE((flag & 2) == 0, "%s: an entry of order lies outside [0, F)", name);
    PRIMX_REQUIRE(flag == 0, "%s: a face index lies outside [0, V)", name);
    return PRIMX_OK;
}

extern "C" int primx_mesh_bvh_query(const float* pts, int64_t n, const int* f, int F, const float* attr, int C, const void* bvh,
                                    int64_t bvh_bytes, float beta, float* dist, int* face, float* wn, float* out_attr,
                                    void* stream) {
    const char* name = "primx_mesh_bvh_query";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_REQUIRE(f, "%s: null pointer", name);
    PRIMX_REQUIRE(F >= 1 && F <= INT32_MAX / 4, "%s: F must lie in 1 .. (2^31 - 1) / 4 (got %d)", name, F);
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX * THREADS, "%s: n out of range", name);
    PRIMX_REQUIRE(C >= 0 && C <= 16, "%s: C must lie in 0 .. 16 (got %d)", name, C);
    PRIMX_REQUIRE(C == 0 || attr, "%s: null attribute pointer with C = %d", name, C);
    PRIMX_REQUIRE(beta >= 0.0f, "%s: beta must be at least 0", name);
    const Layout lay = layout(F);
    PRIMX_REQUIRE(bvh && ((uintptr_t)bvh & 15) == 0 && bvh_bytes >= lay.total,
                  "%s: the tree needs primx_mesh_bvh_workspace(F) = %lld bytes, 16-byte aligned", name, (long long)lay.total);
    if (n == 0) return PRIMX_OK;
    PRIMX_REQUIRE(pts && dist && face && wn && (C == 0 || out_attr), "%s: null pointer", name);
    const char* w = (const char*)bvh;
    hipLaunchKernelGGL(bvh_query_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, pts, n, (const float4*)(w + lay.recs),
                       (const int*)(w + lay.orig), (const float4*)(w + lay.nodes), lay.L, F, f, attr, C, beta, dist, face, wn,
                       out_attr);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_mesh_bvh_raycast(const float* org, const float* dir, int64_t n, float tmin, float tmax, int any_hit,
                                      const int* f, int F, const void* bvh, int64_t bvh_bytes, float* t, int* face, float* bary,
                                      void* stream) {
    const char* name = "primx_mesh_bvh_raycast";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_REQUIRE(f, "%s: null pointer", name);
    PRIMX_REQUIRE(F >= 1 && F <= INT32_MAX / 4, "%s: F must lie in 1 .. (2^31 - 1) / 4 (got %d)", name, F);
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX * THREADS, "%s: n out of range", name);
    PRIMX_REQUIRE(tmin <= tmax, "%s: tmin must not exceed tmax, and neither may be a NaN", name);
    const Layout lay = layout(F);
    PRIMX_REQUIRE(bvh && ((uintptr_t)bvh & 15) == 0 && bvh_bytes >= lay.total,
                  "%s: the tree needs primx_mesh_bvh_workspace(F) = %lld bytes, 16-byte aligned", name, (long long)lay.total);
    if (n == 0) return PRIMX_OK;
    PRIMX_REQUIRE(org && dir && t && face && bary, "%s: null pointer", name);
    const char* w = (const char*)bvh;
    hipLaunchKernelGGL(bvh_raycast_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, org, dir, n, tmin, tmax, any_hit,
                       (const float4*)(w + lay.recs), (const int*)(w + lay.orig), (const float4*)(w + lay.nodes), lay.L, F, t, face,
                       bary);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_mesh_bvh_visibility(const float* pts, int64_t n, const float* dirs, int D, float tmin, int limit, const int* f,
                                         int F, const void* bvh, int64_t bvh_bytes, int* escapes, void* stream) {
    const char* name = "primx_mesh_bvh_visibility";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_REQUIRE(f && dirs, "%s: null pointer", name);
    PRIMX_REQUIRE(F >= 1 && F <= INT32_MAX / 4, "%s: F must lie in 1 .. (2^31 - 1) / 4 (got %d)", name, F);
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX * THREADS, "%s: n out of range", name);
    PRIMX_REQUIRE(D >= 1 && D <= INT32_MAX / 3, "%s: D must be at least 1 (got %d)", name, D);
    PRIMX_REQUIRE(limit >= 0, "%s: limit must be at least 0 (got %d)", name, limit);
    PRIMX_REQUIRE(tmin <= INFINITY, "%s: tmin is a NaN", name);
    const Layout lay = layout(F);
    PRIMX_REQUIRE(bvh && ((uintptr_t)bvh & 15) == 0 && bvh_bytes >= lay.total,
                  "%s: the tree needs primx_mesh_bvh_workspace(F) = %lld bytes, 16-byte aligned", name, (long long)lay.total);
    if (n == 0) return PRIMX_OK;
    PRIMX_REQUIRE(pts && escapes, "%s: null pointer", name);
    const char* w = (const char*)bvh;
    hipLaunchKernelGGL(bvh_visibility_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, pts, n, dirs, D, tmin, limit,
                       (const float4*)(w + lay.recs), (const int*)(w + lay.orig), (const float4*)(w + lay.nodes), lay.L, F, escapes);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}
