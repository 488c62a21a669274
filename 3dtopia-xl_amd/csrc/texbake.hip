// Texture bake (inference.py:126-211): face labels and charts of the UV unwrap, the atlas raster, and the quantize + texel
// fill of the baked attributes.  Replaces xatlas (charts), nvdiffrast (raster + interpolate) and the scipy / scikit-learn
// fill of the reference; the packing of the chart rectangles stays on the host (mesh.py).
//
// Every phase that needs another workgroup's results is a launch of its own; integer atomics are used only where the
// result does not depend on arrival order (atomicMin / atomicAdd into maps read by a later launch).  Output order is fixed
// (faces by index, texels in raster order), so every output is bitwise deterministic.
//
//   labels:     one thread per face: rules 1-2 of include/primx_hip.h (fp32, no FMA contraction: a numpy restatement
//               matches bit for bit).
//   components: connected components of faces joined through shared "corner nodes" (node = vertex * 6 + label for the
//               charts, any other grouping the caller encodes the same way).  min face per node (atomicMin), then
//               union-find: hook roots onto smaller ids (atomicMin, reads only the previous parent array) + one pointer
//               jump per round, three rotating parent arrays; a change flag per round, read back every ROUND_BATCH rounds.
//               Component id = rank of the component's smallest face (block prefix + one-workgroup scan).
//   raster:     one thread per face over its texel bounding box, exact int64 edge functions of 1/256-texel fixed-point
//               corners, rule "E > 0, or E == 0 on an owned edge"; face id map by atomicMin, cover count by atomicAdd;
//               then per-block counts + one-workgroup scan of (covered, doubly covered).
//   compact:    covered texels in raster order (ballot / mbcnt block prefix), each with the 3-D point of its barycentrics.
//   fill:       scatter of the quantized bytes, band map, then per 16 x 16 tile the nearest band texel inside a
//               (2R + 1)^2 window held in LDS.
//   occlusion:  ambient occlusion of the SDF lattice (no counterpart in the reference): one thread per covered texel marches
//               K directions x J trilinear samples through the lattice, rules A1-A4 of include/primx_hip.h; gather-bound.
#include <algorithm>
#include <utility>

#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_common.h"

constexpr int ROUND_BATCH = 4;          // union-find rounds between two reads of the change flags
constexpr int MAX_ROUNDS = 512;
constexpr int TILE = 16;                // fill tile edge (TILE * TILE = THREADS)
constexpr int MAX_RADIUS = 64;
constexpr int MAX_BAND = 16;
constexpr int MAX_SIZE = 16384;         // atlas W, H
constexpr int FIX = 256;                // fixed-point units per texel
constexpr int NO_FACE = 0x7fffffff;

// ------------------------------------------------------------------ labels

__device__ __forceinline__ int axis_label(float s0, float s1, float s2) {
    const float a0 = fabsf(s0), a1 = fabsf(s1), a2 = fabsf(s2);
    int a = 0;
    float m = a0, sa = s0;
    if (a1 > m) { a = 1; m = a1; sa = s1; }
    if (a2 > m) { a = 2; sa = s2; }
    return 2 * a + (sa >= 0.f ? 0 : 1);
}

__global__ __launch_bounds__(THREADS) void tb_labels_kernel(const float* __restrict__ v, const float* __restrict__ n,
                                                            const int* __restrict__ f, int V, int F,
                                                            int* __restrict__ label) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    int idx[3];
    for (int k = 0; k < 3; ++k) {
        idx[k] = f[3 * (size_t)t + k];
        if (idx[k] < 0 || idx[k] >= V) { label[t] = 0; return; }   // refused on the host side of the API contract
    }
    const float* p0 = v + 3 * (size_t)idx[0];
    const float* p1 = v + 3 * (size_t)idx[1];
    const float* p2 = v + 3 * (size_t)idx[2];
    const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    const float g[3] = {e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x};
    float s[3];
    if (n) {
        const float* n0 = n + 3 * (size_t)idx[0];
        const float* n1 = n + 3 * (size_t)idx[1];
        const float* n2 = n + 3 * (size_t)idx[2];
        for (int c = 0; c < 3; ++c) s[c] = (n0[c] + n1[c]) + n2[c];
    } else {
        for (int c = 0; c < 3; ++c) s[c] = g[c];
    }
    int lab = axis_label(s[0], s[1], s[2]);
    const int a = lab >> 1;
    const float ga = (lab & 1) ? -g[a] : g[a];
    const float gn = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);   // correctly rounded (not __fsqrt_rn: v_sqrt_f32, 1 ulp)
    if (ga <= 0.2f * gn) lab = axis_label(g[0], g[1], g[2]);
    label[t] = lab;
}

// ------------------------------------------------------------------ components

__global__ __launch_bounds__(THREADS) void tb_cc_init_kernel(int* __restrict__ minface, int U, int* __restrict__ X,
                                                             int* __restrict__ Y, int F) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t < U) minface[t] = NO_FACE;
    if (t < F) { X[t] = t; Y[t] = t; }
}

__global__ __launch_bounds__(THREADS) void tb_cc_minface_kernel(const int* __restrict__ node, int F, int U,
                                                                int* __restrict__ minface) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= 3 * F) return;
    const int u = node[t];
    if (u >= 0 && u < U) atomicMin(minface + u, t / 3);
}

// Edges (face, min face of each of its corner nodes).  X is read-only here; Y (== X on entry) takes the hooks: a root r
// adjacent to a smaller id gets Y[r] = the smallest such id (atomicMin: the result does not depend on arrival order).
__global__ __launch_bounds__(THREADS) void tb_cc_hook_kernel(const int* __restrict__ node, const int* __restrict__ minface,
                                                             int F, int U, const int* __restrict__ X, int* __restrict__ Y,
                                                             int* __restrict__ flag) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    const int a = X[t];
    bool hooked = false;
    for (int k = 0; k < 3; ++k) {
        const int u = node[3 * (size_t)t + k];
        if (u < 0 || u >= U) continue;
        const int b = X[minface[u]];
        if (a < b && X[b] == b) { atomicMin(Y + b, a); hooked = true; }
        if (b < a && X[a] == a) { atomicMin(Y + a, b); hooked = true; }
    }
    if (hooked) *flag = 1;
}

// One pointer jump: X[t] = Z[t] = Y[Y[t]] (parents only ever point to smaller ids, so there are no cycles).
__global__ __launch_bounds__(THREADS) void tb_cc_jump_kernel(const int* __restrict__ Y, int F, int* __restrict__ X,
                                                             int* __restrict__ Z, int* __restrict__ flag) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    const int y = Y[t], yy = Y[y];
    X[t] = yy;
    Z[t] = yy;
    if (yy != y) *flag = 1;
}

__global__ __launch_bounds__(THREADS) void tb_cc_count_kernel(const int* __restrict__ X, int F, long long* __restrict__ bsum) {
    int c = 0;
    for (int r = 0; r < ROUNDS; ++r) {
        const int t = blockIdx.x * PTS + r * THREADS + threadIdx.x;
        c += (t < F && X[t] == t) ? 1 : 0;
    }
    block_sums(c, 0, bsum);
}

__global__ __launch_bounds__(THREADS) void tb_cc_rank_kernel(const int* __restrict__ X, int F,
                                                             const long long* __restrict__ boff, int* __restrict__ rank) {
    __shared__ int s_wave[THREADS / 64];
    long long run = boff[2 * (size_t)blockIdx.x];
    for (int r = 0; r < ROUNDS; ++r) {
        const int t = blockIdx.x * PTS + r * THREADS + threadIdx.x;
        const bool root = t < F && X[t] == t;
        int tot;
        const int pre = block_prefix(root, s_wave, tot);
        if (root) rank[t] = (int)(run + pre);
        run += tot;
    }
}

__global__ __launch_bounds__(THREADS) void tb_cc_assign_kernel(const int* __restrict__ X, const int* __restrict__ rank, int F,
                                                               int* __restrict__ comp) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t < F) comp[t] = rank[X[t]];
}

// ------------------------------------------------------------------ raster

struct Tri {
    long long ax, ay, bx, by, cx, cy, area;
};

__device__ __forceinline__ bool load_tri(const int* uv, const int* ft, int NUV, int face, Tri& T) {
    int i[3];
    for (int k = 0; k < 3; ++k) {
        i[k] = ft[3 * (size_t)face + k];
        if (i[k] < 0 || i[k] >= NUV) return false;
    }
    T.ax = uv[2 * (size_t)i[0]]; T.ay = uv[2 * (size_t)i[0] + 1];
    T.bx = uv[2 * (size_t)i[1]]; T.by = uv[2 * (size_t)i[1] + 1];
    T.cx = uv[2 * (size_t)i[2]]; T.cy = uv[2 * (size_t)i[2] + 1];
    T.area = (T.bx - T.ax) * (T.cy - T.ay) - (T.by - T.ay) * (T.cx - T.ax);
    return T.area > 0;
}

// edge function of the directed edge p -> q at (x, y): > 0 on the interior side of a face with positive area
__device__ __forceinline__ long long edge_fn(long long px, long long py, long long qx, long long qy, long long x, long long y) {
    return (qx - px) * (y - py) - (qy - py) * (x - px);
}

// a centre exactly on the edge p -> q belongs to the face when the shift (+eps, +eps^2) moves it inside
__device__ __forceinline__ bool edge_in(long long e, long long px, long long py, long long qx, long long qy) {
    const long long dx = qx - px, dy = qy - py;
    return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {   // b > 0
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

__global__ __launch_bounds__(THREADS) void tb_clear_kernel(int* __restrict__ fid, int* __restrict__ cover, int HW) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t < HW) { fid[t] = NO_FACE; cover[t] = 0; }
}

__global__ __launch_bounds__(THREADS) void tb_raster_kernel(const int* __restrict__ uv, const int* __restrict__ ft, int NUV,
                                                            int F, int W, int H, int* __restrict__ fid,
                                                            int* __restrict__ cover) {
    const int face = blockIdx.x * THREADS + threadIdx.x;
    if (face >= F) return;
    Tri T;
    if (!load_tri(uv, ft, NUV, face, T)) return;
    const long long xmin = min(T.ax, min(T.bx, T.cx)), xmax = max(T.ax, max(T.bx, T.cx));
    const long long ymin = min(T.ay, min(T.by, T.cy)), ymax = max(T.ay, max(T.by, T.cy));
    // texel j has its centre at FIX * j + FIX / 2
    const int j0 = (int)min((long long)W, max(0LL, -floor_div(FIX / 2 - xmin, FIX)));
    const int j1 = (int)max(-1LL, min((long long)W - 1, floor_div(xmax - FIX / 2, FIX)));
    const int i0 = (int)min((long long)H, max(0LL, -floor_div(FIX / 2 - ymin, FIX)));
    const int i1 = (int)max(-1LL, min((long long)H - 1, floor_div(ymax - FIX / 2, FIX)));
    for (int i = i0; i <= i1; ++i) {
        const long long y = (long long)FIX * i + FIX / 2;
        for (int j = j0; j <= j1; ++j) {
            const long long x = (long long)FIX * j + FIX / 2;
            if (!edge_in(edge_fn(T.bx, T.by, T.cx, T.cy, x, y), T.bx, T.by, T.cx, T.cy)) continue;
            if (!edge_in(edge_fn(T.cx, T.cy, T.ax, T.ay, x, y), T.cx, T.cy, T.ax, T.ay)) continue;
            if (!edge_in(edge_fn(T.ax, T.ay, T.bx, T.by, x, y), T.ax, T.ay, T.bx, T.by)) continue;
            const size_t t = (size_t)i * W + j;
            atomicMin(fid + t, face);
            atomicAdd(cover + t, 1);
        }
    }
}

// per block: (covered, doubly covered) counts; the empty sentinel becomes -1
__global__ __launch_bounds__(THREADS) void tb_cover_count_kernel(int* __restrict__ fid, const int* __restrict__ cover, int HW,
                                                                 long long* __restrict__ bsum) {
    int a = 0, b = 0;
    for (int r = 0; r < ROUNDS; ++r) {
        const int t = blockIdx.x * PTS + r * THREADS + threadIdx.x;
        if (t >= HW) continue;
        const int c = cover[t];
        if (c == 0) fid[t] = -1;
        a += c > 0 ? 1 : 0;
        b += c > 1 ? 1 : 0;
    }
    block_sums(a, b, bsum);
}

__global__ __launch_bounds__(THREADS) void tb_compact_kernel(const int* __restrict__ fid, int W, int HW,
                                                             const long long* __restrict__ boff, const int* __restrict__ uv,
                                                             const int* __restrict__ ft, int NUV, const float* __restrict__ v,
                                                             const int* __restrict__ f, int V, long long n,
                                                             int* __restrict__ texel, float* __restrict__ pts) {
    __shared__ int s_wave[THREADS / 64];
    long long run = boff[2 * (size_t)blockIdx.x];
    for (int r = 0; r < ROUNDS; ++r) {
        const int t = blockIdx.x * PTS + r * THREADS + threadIdx.x;
        const int face = t < HW ? fid[t] : -1;
        int tot;
        const int pre = block_prefix(face >= 0, s_wave, tot);
        const long long o = run + pre;
        run += tot;
        if (face < 0 || o >= n) continue;
        texel[o] = t;
        float p[3] = {0.f, 0.f, 0.f};
        Tri T;
        int vi[3];
        bool ok = load_tri(uv, ft, NUV, face, T);
        for (int k = 0; k < 3; ++k) {
            vi[k] = f[3 * (size_t)face + k];
            ok = ok && vi[k] >= 0 && vi[k] < V;
        }
        if (ok) {
            const long long x = (long long)FIX * (t % W) + FIX / 2, y = (long long)FIX * (t / W) + FIX / 2;
            const float ar = (float)T.area;
            const float l[3] = {__fdiv_rn((float)edge_fn(T.bx, T.by, T.cx, T.cy, x, y), ar),
                                __fdiv_rn((float)edge_fn(T.cx, T.cy, T.ax, T.ay, x, y), ar),
                                __fdiv_rn((float)edge_fn(T.ax, T.ay, T.bx, T.by, x, y), ar)};
            for (int c = 0; c < 3; ++c)
                p[c] = (l[0] * v[3 * (size_t)vi[0] + c] + l[1] * v[3 * (size_t)vi[1] + c]) + l[2] * v[3 * (size_t)vi[2] + c];
        }
        pts[3 * o] = p[0];
        pts[3 * o + 1] = p[1];
        pts[3 * o + 2] = p[2];
    }
}

// ------------------------------------------------------------------ normal map: tangents, texel normals

// label -> (u axis, v axis) of its projection (mesh.py PROJECTION); the projection axis is label >> 1
__constant__ int PROJ_U[6] = {1, 2, 2, 0, 0, 1};

__device__ __forceinline__ float len3(const float* a) { return sqrtf((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }
__device__ __forceinline__ float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// rules T1-T4 of include/primx_hip.h; one thread per face corner, equal values from every corner of a split vertex
__global__ __launch_bounds__(THREADS) void tb_tangents_kernel(const float* __restrict__ nrm, const int* __restrict__ ft,
                                                              const int* __restrict__ label, int NUV, int F,
                                                              float* __restrict__ tangent) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= 3 * F) return;
    const int vtx = ft[t], lab = label[t / 3];
    if (vtx < 0 || vtx >= NUV || lab < 0 || lab > 5) return;
    const int a = PROJ_U[lab], c = lab >> 1;
    const float sigma = (lab & 1) ? -1.f : 1.f;
    const float N[3] = {nrm[3 * (size_t)vtx], nrm[3 * (size_t)vtx + 1], nrm[3 * (size_t)vtx + 2]};
    const float m = fmaxf(fabsf(N[0]), fmaxf(fabsf(N[1]), fabsf(N[2])));
    float d[3] = {0.f, 0.f, 0.f};
    d[a] = 1.f;
    if (fabsf(N[c]) > 1e-4f * m) {                                  // T1
        d[c] = -__fdiv_rn(N[a], N[c]);
    } else if (m > 0.f) {                                           // T2
        const float nn = dot3(N, N);
        const float k = __fdiv_rn(N[a], nn);
        for (int x = 0; x < 3; ++x) d[x] = d[x] - N[x] * k;
        if (dot3(d, d) < 1e-8f) {
            const float sa = N[a] > 0.f ? 1.f : (N[a] < 0.f ? -1.f : 0.f);
            const float e = N[c] >= 0.f ? -sa : sa;
            const float k2 = __fdiv_rn(e * N[c], nn);
            for (int x = 0; x < 3; ++x) d[x] = (x == c ? e : 0.f) - N[x] * k2;
        }
    }
    const float l = len3(d);
    float* o = tangent + 4 * (size_t)vtx;
    for (int x = 0; x < 3; ++x) o[x] = l > 0.f ? __fdiv_rn(d[x], l) : (x == a ? 1.f : 0.f);
    o[3] = sigma * N[c] < 0.f ? 1.f : -1.f;                         // T4
}

__global__ __launch_bounds__(THREADS) void tb_normal_texels_kernel(const int* __restrict__ texel, long long n,
                                                                   const int* __restrict__ fid, int W, int HW,
                                                                   const int* __restrict__ uv, const int* __restrict__ ft,
                                                                   int NUV, int F, const float* __restrict__ nrm,
                                                                   const float* __restrict__ tangent,
                                                                   const float* __restrict__ g, float* __restrict__ nts,
                                                                   float* __restrict__ attr) {
    const long long k = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (k >= n) return;
    float r[3] = {0.f, 0.f, 1.f};
    const int t = texel[k];
    const int face = (t >= 0 && t < HW) ? fid[t] : -1;
    Tri T;
    if (face >= 0 && face < F && load_tri(uv, ft, NUV, face, T)) {      // load_tri: corners inside [0, NUV), area > 0
        const int vi[3] = {ft[3 * (size_t)face], ft[3 * (size_t)face + 1], ft[3 * (size_t)face + 2]};
        const long long x = (long long)FIX * (t % W) + FIX / 2, y = (long long)FIX * (t / W) + FIX / 2;
        const float ar = (float)T.area;
        const float l[3] = {__fdiv_rn((float)edge_fn(T.bx, T.by, T.cx, T.cy, x, y), ar),
                            __fdiv_rn((float)edge_fn(T.cx, T.cy, T.ax, T.ay, x, y), ar),
                            __fdiv_rn((float)edge_fn(T.ax, T.ay, T.bx, T.by, x, y), ar)};
        float Ni[3], Tp[3];
        for (int c = 0; c < 3; ++c) {
            Ni[c] = (l[0] * nrm[3 * (size_t)vi[0] + c] + l[1] * nrm[3 * (size_t)vi[1] + c]) + l[2] * nrm[3 * (size_t)vi[2] + c];
            Tp[c] = (l[0] * tangent[4 * (size_t)vi[0] + c] + l[1] * tangent[4 * (size_t)vi[1] + c]) +
                    l[2] * tangent[4 * (size_t)vi[2] + c];
        }
        const float w = tangent[4 * (size_t)vi[0] + 3];
        const float ln = len3(Ni);
        if (ln > 0.f) {
            for (int c = 0; c < 3; ++c) Ni[c] = __fdiv_rn(Ni[c], ln);
            const float nt = dot3(Ni, Tp);
            float Ti[3];
            for (int c = 0; c < 3; ++c) Ti[c] = Tp[c] - Ni[c] * nt;
            const float lt = len3(Ti);
            if (lt > 0.f) {
                for (int c = 0; c < 3; ++c) Ti[c] = __fdiv_rn(Ti[c], lt);
                const float B[3] = {w * (Ni[1] * Ti[2] - Ni[2] * Ti[1]), w * (Ni[2] * Ti[0] - Ni[0] * Ti[2]),
                                    w * (Ni[0] * Ti[1] - Ni[1] * Ti[0])};
                const float gv[3] = {g[3 * k], g[3 * k + 1], g[3 * k + 2]};
                const float q[3] = {dot3(gv, Ti), dot3(gv, B), dot3(gv, Ni)};
                const float lq = len3(q);
                if (lq > 0.f)
                    for (int c = 0; c < 3; ++c) r[c] = __fdiv_rn(q[c], lq);
            }
        }
    }
    for (int c = 0; c < 3; ++c) nts[3 * k + c] = r[c];
    if (attr) {
        float* o = attr + 6 * k;
        o[0] = 0.f; o[4] = 0.f; o[5] = 0.f;
        for (int c = 0; c < 3; ++c) {
            const float b = rintf(255.f * (0.5f * r[c] + 0.5f));        // byte; the fill's trunc(x * 255) gives it back
            o[1 + c] = __fdiv_rn(b + 0.5f, 255.f);
        }
    }
}

// ------------------------------------------------------------------ ambient occlusion of the lattice

constexpr int MAX_DIRS = 256;
constexpr int MAX_STEPS = 64;
constexpr int MAX_LATTICE = 1024;

__device__ __forceinline__ float lerp1(float p, float q, float t) { return p + t * (q - p); }

// rule A1 of include/primx_hip.h; the clamp keeps every index inside [0, R - 1] whatever x holds (fmaxf drops a NaN)
__device__ __forceinline__ float occ_phi(const float* __restrict__ lat, int R, float rm1, const float* x, float iso) {
    size_t cell[3];
    float f[3];
    for (int a = 0; a < 3; ++a) {
        const float c = fminf(fmaxf(x[a], -1.f), 1.f);
        const float u = ((c + 1.f) * 0.5f) * rm1;
        const int i = max(0, min((int)floorf(u), R - 2));
        cell[a] = (size_t)i;
        f[a] = u - (float)i;
    }
    const size_t r = (size_t)R;
    const float* p0 = lat + (cell[0] * r + cell[1]) * r + cell[2];       // x, y
    const float* p1 = p0 + r;                                            // x, y + 1
    const float* p2 = p0 + r * r;                                        // x + 1, y
    const float* p3 = p2 + r;                                            // x + 1, y + 1
    const float z00 = lerp1(p0[0], p0[1], f[2]), z01 = lerp1(p1[0], p1[1], f[2]);
    const float z10 = lerp1(p2[0], p2[1], f[2]), z11 = lerp1(p3[0], p3[1], f[2]);
    return lerp1(lerp1(z00, z01, f[1]), lerp1(z10, z11, f[1]), f[0]) - iso;
}

// rules A2-A4; one thread per texel (raster order: neighbouring lanes walk neighbouring cells), the directions in LDS (every lane
// reads the same address: a broadcast)
__global__ __launch_bounds__(THREADS) void tb_occlusion_kernel(const float* __restrict__ lat, int R, const float* __restrict__ pts,
                                                               const float* __restrict__ nrm, long long n,
                                                               const float* __restrict__ dirs, int K, int J, float radius,
                                                               float bias, float iso, float* __restrict__ occ) {
    __shared__ float s_dir[3 * MAX_DIRS];
    for (int q = threadIdx.x; q < 3 * K; q += THREADS) s_dir[q] = dirs[q];
    __syncthreads();
    const long long k = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (k >= n) return;
    const float rm1 = (float)(R - 1);
    const float h = __fdiv_rn(2.f, rm1), fj = (float)J;
    const float N[3] = {nrm[3 * k], nrm[3 * k + 1], nrm[3 * k + 2]};
    float o[3];
    for (int a = 0; a < 3; ++a) o[a] = pts[3 * k + a] + bias * N[a];
    const float phi0 = fmaxf(occ_phi(lat, R, rm1, o, iso), 0.5f * h);
    float num = 0.f, den = 0.f;
    for (int d = 0; d < K; ++d) {
        const float* D = s_dir + 3 * d;
        const float c = fmaxf(0.f, dot3(N, D));
        if (!(c > 0.f)) continue;
        float m = 0.f;
        for (int j = 0; j < J; ++j) {
            const float t = __fdiv_rn(radius * (float)(j + 1), fj);
            const float x[3] = {o[0] + t * D[0], o[1] + t * D[1], o[2] + t * D[2]};
            const float v = occ_phi(lat, R, rm1, x, iso);
            m = j == 0 ? v : fminf(m, v);
            if (m <= 0.f) break;                                         // V is 0 from here on
        }
        const float V = fminf(fmaxf(__fdiv_rn(m, phi0), 0.f), 1.f);
        num += c * (1.f - V);
        den += c;
    }
    occ[k] = den > 0.f ? 1.f - __fdiv_rn(num, den) : 1.f;
}

// ------------------------------------------------------------------ quantize + fill

__device__ __forceinline__ uint8_t quant(float x) {
    const float y = x * 255.f;                       // trunc(fp32(x * 255)): the reference's astype(uint8)
    return (uint8_t)(y >= 255.f ? 255 : (y > 0.f ? (int)y : 0));
}

// img [HW][8] bytes: albedo RGB, 0, 0 (R of metallic-roughness), roughness, metallic, pad
__global__ __launch_bounds__(THREADS) void tb_scatter_kernel(const float* __restrict__ attr, const int* __restrict__ texel,
                                                             long long n, int HW, uint8_t* __restrict__ img) {
    const long long k = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (k >= n) return;
    const int t = texel[k];
    if (t < 0 || t >= HW) return;
    const float* a = attr + 6 * k;
    uint8_t* o = img + 8 * (size_t)t;
    o[0] = quant(a[1]);
    o[1] = quant(a[2]);
    o[2] = quant(a[3]);
    o[3] = 0;
    o[4] = quant(a[4]);
    o[5] = quant(a[5]);
}

// band[t] = covered and some texel within city-block distance `band` is uncovered or outside the image
__global__ __launch_bounds__(THREADS) void tb_band_kernel(const int* __restrict__ fid, int W, int H, int band,
                                                          uint8_t* __restrict__ out) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= W * H) return;
    const int i = t / W, j = t - i * W;
    bool edge = false;
    if (fid[t] >= 0) {
        for (int di = -band; di <= band && !edge; ++di) {
            const int rem = band - abs(di);
            for (int dj = -rem; dj <= rem; ++dj) {
                const int y = i + di, x = j + dj;
                if (y < 0 || y >= H || x < 0 || x >= W || fid[(size_t)y * W + x] < 0) { edge = true; break; }
            }
        }
    }
    out[t] = edge ? 1 : 0;
}

// One 16 x 16 tile per block: band flags of the tile + an R-texel halo in LDS; each uncovered texel with a band texel
// within city-block distance R copies the band texel at the smallest squared distance (scan order (row, column) keeps
// the first of equal distances); covered texels keep their own bytes; everything else is 0.
__global__ __launch_bounds__(THREADS) void tb_fill_kernel(const uint8_t* __restrict__ bandmap, const int* __restrict__ fid,
                                                          const uint8_t* __restrict__ img, int W, int H, int R,
                                                          uint8_t* __restrict__ albedo, uint8_t* __restrict__ mr) {
    __shared__ uint8_t s_band[(TILE + 2 * MAX_RADIUS) * (TILE + 2 * MAX_RADIUS)];
    const int span = TILE + 2 * R;
    const int ti = blockIdx.y * TILE, tj = blockIdx.x * TILE;
    int any = 0;
    for (int q = threadIdx.x; q < span * span; q += THREADS) {
        const int y = ti - R + q / span, x = tj - R + q % span;
        const uint8_t b = (y >= 0 && y < H && x >= 0 && x < W) ? bandmap[(size_t)y * W + x] : 0;
        s_band[q] = b;
        any |= b;
    }
    any = __syncthreads_or(any);
    const int li = threadIdx.x / TILE, lj = threadIdx.x % TILE;
    const int i = ti + li, j = tj + lj;
    if (i >= H || j >= W) return;
    const size_t t = (size_t)i * W + j;
    long long src = -1;
    if (fid[t] >= 0) {
        src = (long long)t;
    } else if (any) {
        int best = 0x7fffffff, bi = 0, bj = 0, l1 = 0x7fffffff;
        for (int di = -R; di <= R; ++di) {
            const uint8_t* row = s_band + (li + R + di) * span + lj + R;
            for (int dj = -R; dj <= R; ++dj) {
                if (!row[dj]) continue;
                const int d2 = di * di + dj * dj;
                if (d2 < best) { best = d2; bi = di; bj = dj; }
                l1 = min(l1, abs(di) + abs(dj));
            }
        }
        if (l1 <= R) src = (long long)(i + bi) * W + (j + bj);
    }
    uint8_t o[6] = {0, 0, 0, 0, 0, 0};
    if (src >= 0)
        for (int c = 0; c < 6; ++c) o[c] = img[8 * src + c];
    albedo[3 * t] = o[0]; albedo[3 * t + 1] = o[1]; albedo[3 * t + 2] = o[2];
    mr[3 * t] = o[3]; mr[3 * t + 1] = o[4]; mr[3 * t + 2] = o[5];
}

}  // namespace

// ------------------------------------------------------------------ host side
namespace {

struct CcLayout {
    size_t minface, p0, p1, p2, rank, bsum, flags, tot, total;
    int nblk;
};

CcLayout cc_layout(int F, int U) {
    CcLayout l;
    Arena a;
    l.nblk = nblocks(F, PTS);
    l.minface = a.take((size_t)U * 4);
    l.p0 = a.take((size_t)F * 4);
    l.p1 = a.take((size_t)F * 4);
    l.p2 = a.take((size_t)F * 4);
    l.rank = a.take((size_t)F * 4);
    l.bsum = a.take((size_t)l.nblk * 16);
    l.flags = a.take(ROUND_BATCH * 4);
    l.tot = a.take(16);
    l.total = a.total;
    return l;
}

int check_cc(const char* name, int F, int U) {
    PRIMX_REQUIRE(F >= 0, "%s: need F >= 0 (got %d)", name, F);
    PRIMX_REQUIRE(U >= 1, "%s: need U >= 1 (got %d)", name, U);
    PRIMX_REQUIRE(3 * (int64_t)F < I31, "%s: 3 * F must be < 2^31 (got F = %d)", name, F);
    return PRIMX_OK;
}

struct RasterLayout {
    size_t bsum, total;
    int nblk;
};

RasterLayout raster_layout(int W, int H) {
    RasterLayout l;
    Arena a;
    l.nblk = nblocks((int64_t)W * H, PTS);
    l.bsum = a.take((size_t)l.nblk * 16);
    l.total = a.total;
    return l;
}

int check_atlas(const char* name, int W, int H) {
    PRIMX_REQUIRE(W >= 1 && W <= MAX_SIZE && H >= 1 && H <= MAX_SIZE, "%s: W, H must be in [1, %d] (got %d x %d)", name,
                  MAX_SIZE, W, H);
    return PRIMX_OK;
}

struct FillLayout {
    size_t img, band, total;
};

FillLayout fill_layout(int W, int H) {
    FillLayout l;
    Arena a;
    l.img = a.take((size_t)W * H * 8);
    l.band = a.take((size_t)W * H);
    l.total = a.total;
    return l;
}

int check_mesh(const char* name, int V, int F, int NUV) {
    PRIMX_REQUIRE(F >= 0 && V >= 0 && NUV >= 0, "%s: need F, V, NUV >= 0 (got %d, %d, %d)", name, F, V, NUV);
    PRIMX_REQUIRE(3 * (int64_t)F < I31 && 3 * (int64_t)V < I31 && 2 * (int64_t)NUV < I31,
                  "%s: 3 * F, 3 * V and 2 * NUV must be < 2^31 (got F = %d, V = %d, NUV = %d)", name, F, V, NUV);
    return PRIMX_OK;
}

}  // namespace

extern "C" int primx_texbake_labels(const float* v, const float* n, const int* f, int V, int F, int* label, void* stream) {
    PRIMX_REQUIRE(F >= 0 && V >= 0, "primx_texbake_labels: need F, V >= 0 (got %d, %d)", F, V);
    PRIMX_REQUIRE(3 * (int64_t)F < I31 && 6 * (int64_t)V < I31,
                  "primx_texbake_labels: 3 * F and 6 * V must be < 2^31 (got F = %d, V = %d)", F, V);
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(v && f && label, "primx_texbake_labels: null pointer");
    PRIMX_REQUIRE(V >= 1, "primx_texbake_labels: faces without vertices (V = 0)");
    hipLaunchKernelGGL(tb_labels_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, v, n, f, V, F,
                       label);
    PRIMX_CHECK_LAUNCH("primx_texbake_labels");
    return PRIMX_OK;
}

extern "C" int primx_texbake_components_workspace(int F, int U, int64_t* bytes) {
    PRIMX_REQUIRE(bytes, "primx_texbake_components_workspace: null pointer");
    PRIMX_TRY(check_cc("primx_texbake_components_workspace", F, U));
    *bytes = (int64_t)cc_layout(F, U).total;
    return PRIMX_OK;
}

extern "C" int primx_texbake_components(const int* node, int F, int U, void* ws, int64_t ws_bytes, int* comp,
                                        int64_t* n_comp, void* stream) {
    PRIMX_REQUIRE(n_comp, "primx_texbake_components: null pointer");
    PRIMX_TRY(check_cc("primx_texbake_components", F, U));
    *n_comp = 0;
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(node && ws && comp, "primx_texbake_components: null pointer");
    const CcLayout l = cc_layout(F, U);
    PRIMX_REQUIRE(ws_bytes >= (int64_t)l.total, "primx_texbake_components: workspace of %lld bytes, need %lld",
                  (long long)ws_bytes, (long long)l.total);
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    int* minface = (int*)(w + l.minface);
    int* buf[3] = {(int*)(w + l.p0), (int*)(w + l.p1), (int*)(w + l.p2)};
    int* flags = (int*)(w + l.flags);
    long long* bsum = (long long*)(w + l.bsum);
    hipLaunchKernelGGL(tb_cc_init_kernel, dim3(nblocks(std::max(U, F), THREADS)), dim3(THREADS), 0, st, minface, U, buf[0],
                       buf[1], F);
    PRIMX_CHECK_LAUNCH("primx_texbake_components (init)");
    hipLaunchKernelGGL(tb_cc_minface_kernel, dim3(nblocks(3 * (int64_t)F, THREADS)), dim3(THREADS), 0, st, node, F, U, minface);
    PRIMX_CHECK_LAUNCH("primx_texbake_components (min face)");
    // X = buf[0] (settled parents), Y = buf[y] (== X, takes the hooks), Z = the third array
    int y = 1, z = 2, rounds = 0;
    bool done = false;
    while (!done) {
        PRIMX_REQUIRE(rounds < MAX_ROUNDS, "primx_texbake_components: no convergence after %d rounds", rounds);
        PRIMX_TRY(zero(flags, ROUND_BATCH * sizeof(int), st, "primx_texbake_components"));
        for (int r = 0; r < ROUND_BATCH; ++r) {
            hipLaunchKernelGGL(tb_cc_hook_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, node, minface, F, U,
                               (const int*)buf[0], buf[y], flags + r);
            PRIMX_CHECK_LAUNCH("primx_texbake_components (hook)");
            hipLaunchKernelGGL(tb_cc_jump_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, (const int*)buf[y], F,
                               buf[0], buf[z], flags + r);
            PRIMX_CHECK_LAUNCH("primx_texbake_components (jump)");
            std::swap(y, z);
        }
        rounds += ROUND_BATCH;
        int h[ROUND_BATCH];
        PRIMX_TRY(readback(h, flags, sizeof(h), st, "primx_texbake_components"));
        for (int r = 0; r < ROUND_BATCH; ++r) done = done || h[r] == 0;   // a round without change: every later one too
    }
    hipLaunchKernelGGL(tb_cc_count_kernel, dim3(l.nblk), dim3(THREADS), 0, st, (const int*)buf[0], F, bsum);
    PRIMX_CHECK_LAUNCH("primx_texbake_components (count)");
    long long* tot = (long long*)(w + l.tot);
    PRIMX_TRY(scan_blocks(bsum, l.nblk, tot, st, "primx_texbake_components (scan)"));
    int* rank = (int*)(w + l.rank);
    hipLaunchKernelGGL(tb_cc_rank_kernel, dim3(l.nblk), dim3(THREADS), 0, st, (const int*)buf[0], F, (const long long*)bsum,
                       rank);
    PRIMX_CHECK_LAUNCH("primx_texbake_components (rank)");
    hipLaunchKernelGGL(tb_cc_assign_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, (const int*)buf[0],
                       (const int*)rank, F, comp);
    PRIMX_CHECK_LAUNCH("primx_texbake_components (assign)");
    long long ht[2];
    PRIMX_TRY(readback(ht, tot, sizeof(ht), st, "primx_texbake_components"));
    *n_comp = ht[0];
    return PRIMX_OK;
}

extern "C" int primx_texbake_raster_workspace(int W, int H, int64_t* bytes) {
    PRIMX_REQUIRE(bytes, "primx_texbake_raster_workspace: null pointer");
    PRIMX_TRY(check_atlas("primx_texbake_raster_workspace", W, H));
    *bytes = (int64_t)raster_layout(W, H).total;
    return PRIMX_OK;
}

extern "C" int primx_texbake_raster(const int* uv, const int* ft, int NUV, int F, int W, int H, int* face_id, int* cover,
                                    void* ws, int64_t ws_bytes, int64_t* totals, void* stream) {
    PRIMX_TRY(check_atlas("primx_texbake_raster", W, H));
    PRIMX_TRY(check_mesh("primx_texbake_raster", 0, F, NUV));
    PRIMX_REQUIRE(face_id && cover && ws && totals, "primx_texbake_raster: null pointer");
    PRIMX_REQUIRE(F == 0 || (uv && ft), "primx_texbake_raster: null pointer");
    const RasterLayout l = raster_layout(W, H);
    PRIMX_REQUIRE(ws_bytes >= (int64_t)l.total, "primx_texbake_raster: workspace of %lld bytes, need %lld",
                  (long long)ws_bytes, (long long)l.total);
    hipStream_t st = (hipStream_t)stream;
    const int HW = W * H;
    long long* bsum = (long long*)((char*)ws + l.bsum);
    hipLaunchKernelGGL(tb_clear_kernel, dim3(nblocks(HW, THREADS)), dim3(THREADS), 0, st, face_id, cover, HW);
    PRIMX_CHECK_LAUNCH("primx_texbake_raster (clear)");
    if (F > 0) {
        hipLaunchKernelGGL(tb_raster_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, uv, ft, NUV, F, W, H, face_id,
                           cover);
        PRIMX_CHECK_LAUNCH("primx_texbake_raster (raster)");
    }
    hipLaunchKernelGGL(tb_cover_count_kernel, dim3(l.nblk), dim3(THREADS), 0, st, face_id, (const int*)cover, HW, bsum);
    PRIMX_CHECK_LAUNCH("primx_texbake_raster (count)");
    return scan_blocks(bsum, l.nblk, (long long*)totals, st, "primx_texbake_raster (scan)");
}

extern "C" int primx_texbake_compact(const int* face_id, int W, int H, const void* ws, int64_t ws_bytes, const int* uv,
                                     const int* ft, int NUV, const float* v, const int* f, int V, int F, int64_t n,
                                     int* texel, float* points, void* stream) {
    PRIMX_TRY(check_atlas("primx_texbake_compact", W, H));
    PRIMX_TRY(check_mesh("primx_texbake_compact", V, F, NUV));
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)W * H, "primx_texbake_compact: n = %lld is not a count of texels", (long long)n);
    if (n == 0) return PRIMX_OK;
    PRIMX_REQUIRE(face_id && ws && uv && ft && v && f && texel && points, "primx_texbake_compact: null pointer");
    const RasterLayout l = raster_layout(W, H);
    PRIMX_REQUIRE(ws_bytes >= (int64_t)l.total, "primx_texbake_compact: workspace of %lld bytes, need %lld",
                  (long long)ws_bytes, (long long)l.total);
    hipLaunchKernelGGL(tb_compact_kernel, dim3(l.nblk), dim3(THREADS), 0, (hipStream_t)stream, face_id, W, W * H,
                       (const long long*)((const char*)ws + l.bsum), uv, ft, NUV, v, f, V, (long long)n, texel, points);
    PRIMX_CHECK_LAUNCH("primx_texbake_compact");
    return PRIMX_OK;
}

extern "C" int primx_texbake_fill_workspace(int W, int H, int64_t* bytes) {
    PRIMX_REQUIRE(bytes, "primx_texbake_fill_workspace: null pointer");
    PRIMX_TRY(check_atlas("primx_texbake_fill_workspace", W, H));
    *bytes = (int64_t)fill_layout(W, H).total;
    return PRIMX_OK;
}

extern "C" int primx_texbake_fill(const float* attr, const int* texel, int64_t n, const int* face_id, int W, int H,
                                  int radius, int band, void* ws, int64_t ws_bytes, uint8_t* albedo,
                                  uint8_t* metallic_roughness, void* stream) {
    PRIMX_TRY(check_atlas("primx_texbake_fill", W, H));
    PRIMX_REQUIRE(radius >= 1 && radius <= MAX_RADIUS, "primx_texbake_fill: radius must be in [1, %d] (got %d)", MAX_RADIUS,
                  radius);
    PRIMX_REQUIRE(band >= 1 && band <= MAX_BAND, "primx_texbake_fill: band must be in [1, %d] (got %d)", MAX_BAND, band);
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)W * H, "primx_texbake_fill: n = %lld is not a count of texels", (long long)n);
    PRIMX_REQUIRE(face_id && ws && albedo && metallic_roughness, "primx_texbake_fill: null pointer");
    PRIMX_REQUIRE(n == 0 || (attr && texel), "primx_texbake_fill: null pointer");
    const FillLayout l = fill_layout(W, H);
    PRIMX_REQUIRE(ws_bytes >= (int64_t)l.total, "primx_texbake_fill: workspace of %lld bytes, need %lld", (long long)ws_bytes,
                  (long long)l.total);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* img = (uint8_t*)ws + l.img;
    uint8_t* bandmap = (uint8_t*)ws + l.band;
    const int HW = W * H;
    if (n > 0) {
        hipLaunchKernelGGL(tb_scatter_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, attr, texel, (long long)n, HW,
                           img);
        PRIMX_CHECK_LAUNCH("primx_texbake_fill (scatter)");
    }
    hipLaunchKernelGGL(tb_band_kernel, dim3(nblocks(HW, THREADS)), dim3(THREADS), 0, st, face_id, W, H, band, bandmap);
    PRIMX_CHECK_LAUNCH("primx_texbake_fill (band)");
    hipLaunchKernelGGL(tb_fill_kernel, dim3(nblocks(W, TILE), nblocks(H, TILE)), dim3(THREADS), 0, st,
                       (const uint8_t*)bandmap, face_id, (const uint8_t*)img, W, H, radius, albedo, metallic_roughness);
    PRIMX_CHECK_LAUNCH("primx_texbake_fill (fill)");
    return PRIMX_OK;
}

extern "C" int primx_texbake_tangents(const float* nrm, const int* ft, const int* label, int NUV, int F, float* tangent,
                                      void* stream) {
    PRIMX_TRY(check_mesh("primx_texbake_tangents", 0, F, NUV));
    PRIMX_REQUIRE(4 * (int64_t)NUV < I31, "primx_texbake_tangents: 4 * NUV must be < 2^31 (got NUV = %d)", NUV);
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(nrm && ft && label && tangent, "primx_texbake_tangents: null pointer");
    PRIMX_REQUIRE(NUV >= 1, "primx_texbake_tangents: faces without vertices (NUV = 0)");
    hipLaunchKernelGGL(tb_tangents_kernel, dim3(nblocks(3 * (int64_t)F, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, nrm,
                       ft, label, NUV, F, tangent);
    PRIMX_CHECK_LAUNCH("primx_texbake_tangents");
    return PRIMX_OK;
}

extern "C" int primx_texbake_normal_texels(const int* texel, int64_t n, const int* face_id, int W, int H, const int* uv,
                                           const int* ft, int NUV, int F, const float* nrm, const float* tangent,
                                           const float* g, float* nts, float* attr, void* stream) {
    PRIMX_TRY(check_atlas("primx_texbake_normal_texels", W, H));
    PRIMX_TRY(check_mesh("primx_texbake_normal_texels", 0, F, NUV));
    PRIMX_REQUIRE(4 * (int64_t)NUV < I31, "primx_texbake_normal_texels: 4 * NUV must be < 2^31 (got NUV = %d)", NUV);
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)W * H, "primx_texbake_normal_texels: n = %lld is not a count of texels", (long long)n);
    if (n == 0) return PRIMX_OK;
    PRIMX_REQUIRE(texel && face_id && uv && ft && nrm && tangent && g && nts, "primx_texbake_normal_texels: null pointer");
    hipLaunchKernelGGL(tb_normal_texels_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, texel,
                       (long long)n, face_id, W, W * H, uv, ft, NUV, F, nrm, tangent, g, nts, attr);
    PRIMX_CHECK_LAUNCH("primx_texbake_normal_texels");
    return PRIMX_OK;
}

extern "C" int primx_texbake_occlusion(const float* lattice, int R, const float* pts, const float* nrm, int64_t n,
                                       const float* dirs, int K, int steps, float radius, float bias, float isovalue, float* occ,
                                       void* stream) {
    PRIMX_REQUIRE(R >= 2 && R <= MAX_LATTICE, "primx_texbake_occlusion: R must be in [2, %d] (got %d)", MAX_LATTICE, R);
    PRIMX_REQUIRE(K >= 1 && K <= MAX_DIRS, "primx_texbake_occlusion: K must be in [1, %d] (got %d)", MAX_DIRS, K);
    PRIMX_REQUIRE(steps >= 1 && steps <= MAX_STEPS, "primx_texbake_occlusion: steps must be in [1, %d] (got %d)", MAX_STEPS, steps);
    PRIMX_REQUIRE(radius > 0.f && bias >= 0.f, "primx_texbake_occlusion: need radius > 0 and bias >= 0 (got %g, %g)", (double)radius,
                  (double)bias);
    PRIMX_REQUIRE(n >= 0 && n < I31, "primx_texbake_occlusion: n must be in [0, 2^31) (got %lld)", (long long)n);
    if (n == 0) return PRIMX_OK;
    PRIMX_REQUIRE(lattice && pts && nrm && dirs && occ, "primx_texbake_occlusion: null pointer");
    hipLaunchKernelGGL(tb_occlusion_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, lattice, R, pts, nrm,
                       (long long)n, dirs, K, steps, radius, bias, isovalue, occ);
    PRIMX_CHECK_LAUNCH("primx_texbake_occlusion");
    return PRIMX_OK;
}
