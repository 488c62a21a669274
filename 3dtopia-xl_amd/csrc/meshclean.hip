// Mesh cleanup (inference.py:126, the reference's clean_mesh(v, f, min_f=8, min_d=5, repair=True, remesh=False)):
// rules R0-R8 of include/primx_hip.h, replacing the pymeshlab filters of utils/meshutils.py:118-193.
//
// Every phase that needs another workgroup's results is a launch of its own; integer atomics are used only where the
// result does not depend on arrival order (atomicMin / atomicMax / atomicAdd into maps read by a later launch; the slot
// a vertex takes inside its grid cell does depend on it, but every reader of a cell takes a min or an any over it).
// Output order is fixed (faces and vertices by index, block-prefix compaction), so every output is bitwise
// deterministic.
//
//   merge:       referenced flags, bounding box (order-preserving int encoding of fp32, atomicMin / atomicMax), host
//                readback -> radius and grid; counting sort of the referenced vertices into the grid; then rounds
//                (double-buffered states, a change flag per round read back every ROUND_BATCH rounds): a vertex is
//                CAPTURED once a lower-index CENTRE lies within r, and decided once every lower-index vertex within r is.
//   faces:       smallest face per vertex-set id (atomicMin), keep = not degenerate, smallest, g != 0; compaction.
//   components:  per component face count and bounding box (one wave-reduced atomic per wave where a wave's faces share
//                a component), the mesh's box from the components', drop flags; compaction; per-edge face counts and the
//                candidate keys (|g| bits, face) of R6.
//   edges:       the sorted candidates in one sequential pass on one lane; compaction.
//   fans:        per vertex its lowest corner and its fan count (a fan counted at its smallest corner); split vertices in
//                corner order; output vertex ids and vmap.
#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <utility>

#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_common.h"

constexpr int GRID_CAP = 128;            // grid cells per axis at most
constexpr int ROUND_BATCH = 8;           // merge rounds between two reads of the change flags
constexpr int UND = 0, CEN = 1, CAPT = 2, FIN = 3, NONE = 4;   // merge states (NONE: unreferenced)

__device__ __forceinline__ int ord_enc(float x) {
    const int i = __float_as_int(x);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
__device__ __host__ __forceinline__ float ord_dec(int i) {
    const int b = i >= 0 ? i : i ^ 0x7fffffff;
    float x;
    memcpy(&x, &b, 4);
    return x;
}

// ------------------------------------------------------------------ merge (R0-R2)

__global__ __launch_bounds__(THREADS) void mc_ref_kernel(const int* __restrict__ f, int F, int V, int* __restrict__ ref) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= 3 * F) return;
    const int x = f[t];
    if (x >= 0 && x < V) ref[x] = 1;
}

// bb [6] = encoded (min x, y, z, max x, y, z) over the referenced vertices
__global__ __launch_bounds__(THREADS) void mc_bbox_kernel(const float* __restrict__ v, const int* __restrict__ ref, int V,
                                                          int* __restrict__ bb) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    const bool ok = t < V && ref[t];
    int lo[3], hi[3];
    for (int c = 0; c < 3; ++c) {
        const int e = ok ? ord_enc(v[3 * (size_t)t + c]) : 0;
        lo[c] = wave_min(ok ? e : INT_MAX);
        hi[c] = wave_max(ok ? e : INT_MIN);
    }
    if ((threadIdx.x & 63) == 0 && lo[0] != INT_MAX)
        for (int c = 0; c < 3; ++c) { atomicMin(bb + c, lo[c]); atomicMax(bb + 3 + c, hi[c]); }
}

struct Grid {
    float lo[3];
    float inv;
    int d[3];
};

__device__ __forceinline__ int cell_axis(float x, float lo, float inv, int d) {
    const int c = (int)floorf((x - lo) * inv);
    return min(d - 1, max(0, c));
}

__global__ __launch_bounds__(THREADS) void mc_cell_kernel(const float* __restrict__ v, const int* __restrict__ ref, int V,
                                                          Grid g, int* __restrict__ cellof, int* __restrict__ count) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= V) return;
    if (!ref[t]) { cellof[t] = -1; return; }
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = cell_axis(v[3 * (size_t)t + a], g.lo[a], g.inv, g.d[a]);
    const int id = (c[0] * g.d[1] + c[1]) * g.d[2] + c[2];
    cellof[t] = id;
    atomicAdd(count + id, 1);
}

__global__ __launch_bounds__(THREADS) void mc_scatter_kernel(const int* __restrict__ cellof, int V, int* __restrict__ cursor,
                                                             int* __restrict__ sorted, int* __restrict__ st0,
                                                             int* __restrict__ st1) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= V) return;
    const int id = cellof[t];
    const int s = id >= 0 ? UND : NONE;
    st0[t] = s;
    st1[t] = s;
    if (id < 0) return;
    sorted[atomicAdd(cursor + id, 1)] = t;   // slot order inside a cell is not used by any result
}

// One round: states in -> out (every vertex writes its state); captor written when a vertex becomes FIN.
__global__ __launch_bounds__(THREADS) void mc_round_kernel(const float* __restrict__ v, const int* __restrict__ cellof,
                                                           const int* __restrict__ start, const int* __restrict__ sorted,
                                                           int V, Grid g, float r2, const int* __restrict__ in,
                                                           int* __restrict__ out, int* __restrict__ captor,
                                                           int* __restrict__ flag) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= V) return;
    const int s = in[i];
    if (s != UND && s != CAPT) { out[i] = s; return; }
    const int id = cellof[i];
    const int cz = id % g.d[2], cy = (id / g.d[2]) % g.d[1], cx = id / (g.d[2] * g.d[1]);
    const float xi = v[3 * (size_t)i], yi = v[3 * (size_t)i + 1], zi = v[3 * (size_t)i + 2];
    bool und = false;
    int mc = INT_MAX;
    for (int ax = max(0, cx - 1); ax <= min(g.d[0] - 1, cx + 1); ++ax)
        for (int ay = max(0, cy - 1); ay <= min(g.d[1] - 1, cy + 1); ++ay)
            for (int az = max(0, cz - 1); az <= min(g.d[2] - 1, cz + 1); ++az) {
                const int c = (ax * g.d[1] + ay) * g.d[2] + az;
                const int e = start[c + 1];
                for (int q = start[c]; q < e; ++q) {
                    const int j = sorted[q];
                    if (j >= i) continue;
                    const float dx = xi - v[3 * (size_t)j], dy = yi - v[3 * (size_t)j + 1], dz = zi - v[3 * (size_t)j + 2];
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 < r2 || d2 == 0.f)) continue;
                    const int sj = in[j];
                    und = und || sj == UND;
                    if (sj == CEN) mc = min(mc, j);
                }
            }
    int o = s;
    if (!und) {
        o = mc == INT_MAX ? CEN : FIN;
        if (o == FIN) captor[i] = mc;
    } else if (s == UND && mc != INT_MAX) {
        o = CAPT;
    }
    out[i] = o;
    if (o != s) *flag = 1;
}

__global__ __launch_bounds__(THREADS) void mc_centre_kernel(const int* __restrict__ st, const int* __restrict__ captor,
                                                            const int* __restrict__ ref, int V, int merged,
                                                            int* __restrict__ centre) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= V) return;
    if (!merged) { centre[i] = ref[i] ? i : -1; return; }
    const int s = st[i];
    centre[i] = s == CEN ? i : (s == FIN ? captor[i] : -1);
}

// ------------------------------------------------------------------ faces (R2-R4)

__device__ __forceinline__ bool load_face(const int* f, int t, int V, int idx[3]) {
    for (int k = 0; k < 3; ++k) {
        idx[k] = f[3 * (size_t)t + k];
        if (idx[k] < 0 || idx[k] >= V) return false;
    }
    return idx[0] != idx[1] && idx[1] != idx[2] && idx[0] != idx[2];
}

__device__ __forceinline__ void face_g(const float* v, const int idx[3], float g[3]) {
    const float* p0 = v + 3 * (size_t)idx[0];
    const float* p1 = v + 3 * (size_t)idx[1];
    const float* p2 = v + 3 * (size_t)idx[2];
    const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    g[0] = e1y * e2z - e1z * e2y;
    g[1] = e1z * e2x - e1x * e2z;
    g[2] = e1x * e2y - e1y * e2x;
}

__global__ __launch_bounds__(THREADS) void mc_face_min_kernel(const int* __restrict__ fr, const int* __restrict__ tid, int V,
                                                              int F, int* __restrict__ minface) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    int idx[3];
    const int k = tid[t];
    if (load_face(fr, t, V, idx) && k >= 0 && k < F) atomicMin(minface + k, t);
}

__global__ __launch_bounds__(THREADS) void mc_face_keep_kernel(const float* __restrict__ v, const int* __restrict__ fr,
                                                               const int* __restrict__ tid, const int* __restrict__ minface,
                                                               int V, int F, int* __restrict__ keep) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    int idx[3];
    const int k = tid[t];
    bool ok = load_face(fr, t, V, idx) && k >= 0 && k < F && minface[k] == t;
    if (ok) {
        float g[3];
        face_g(v, idx, g);
        ok = !(g[0] == 0.f && g[1] == 0.f && g[2] == 0.f);
    }
    keep[t] = ok ? 1 : 0;
}

// out[rank[t]] = in[t] for the rows with rank >= 0 (rows of `width` ints)
__global__ __launch_bounds__(THREADS) void mc_gather_rows_kernel(const int* __restrict__ in, const int* __restrict__ rank,
                                                                 int n, int width, int* __restrict__ out) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= n) return;
    const int o = rank[t];
    if (o < 0) return;
    for (int k = 0; k < width; ++k) out[(size_t)width * o + k] = in[(size_t)width * t + k];
}

// ------------------------------------------------------------------ components (R5) and the R6 candidates

__global__ __launch_bounds__(THREADS) void mc_comp_init_kernel(int* __restrict__ cnt, int* __restrict__ bb, int C,
                                                               int* __restrict__ gbb) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t < C) {
        cnt[t] = 0;
        for (int k = 0; k < 3; ++k) { bb[6 * (size_t)t + k] = INT_MAX; bb[6 * (size_t)t + 3 + k] = INT_MIN; }
    }
    if (t < 3) { gbb[t] = INT_MAX; gbb[3 + t] = INT_MIN; }
}

__global__ __launch_bounds__(THREADS) void mc_comp_stats_kernel(const float* __restrict__ v, const int* __restrict__ f,
                                                                const int* __restrict__ comp, int V, int F, int C,
                                                                int* __restrict__ cnt, int* __restrict__ bb) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    int idx[3];
    int c = -1;
    int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
    if (t < F) {
        c = comp[t];
        bool ok = c >= 0 && c < C;
        for (int k = 0; k < 3 && ok; ++k) {
            idx[k] = f[3 * (size_t)t + k];
            ok = idx[k] >= 0 && idx[k] < V;
        }
        if (!ok) c = -1;
        else
            for (int a = 0; a < 3; ++a)
                for (int k = 0; k < 3; ++k) {
                    const int e = ord_enc(v[3 * (size_t)idx[k] + a]);
                    lo[a] = min(lo[a], e);
                    hi[a] = max(hi[a], e);
                }
    }
    const int cf = __builtin_amdgcn_readfirstlane(c);
    if (__ballot(c >= 0 && c != cf) == 0) {            // the wave's faces share one component (or none is valid)
        const int n = wave_sum(c >= 0 ? 1 : 0);
        for (int a = 0; a < 3; ++a) { lo[a] = wave_min(lo[a]); hi[a] = wave_max(hi[a]); }
        if ((threadIdx.x & 63) == 0 && cf >= 0 && n > 0) {
            atomicAdd(cnt + cf, n);
            for (int a = 0; a < 3; ++a) { atomicMin(bb + 6 * (size_t)cf + a, lo[a]); atomicMax(bb + 6 * (size_t)cf + 3 + a, hi[a]); }
        }
    } else if (c >= 0) {
        atomicAdd(cnt + c, 1);
        for (int a = 0; a < 3; ++a) { atomicMin(bb + 6 * (size_t)c + a, lo[a]); atomicMax(bb + 6 * (size_t)c + 3 + a, hi[a]); }
    }
}

__global__ __launch_bounds__(THREADS) void mc_comp_union_kernel(const int* __restrict__ bb, int C, int* __restrict__ gbb) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    int lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = wave_min(t < C ? bb[6 * (size_t)t + a] : INT_MAX);
        hi[a] = wave_max(t < C ? bb[6 * (size_t)t + 3 + a] : INT_MIN);
    }
    if ((threadIdx.x & 63) == 0 && lo[0] != INT_MAX)
        for (int a = 0; a < 3; ++a) { atomicMin(gbb + a, lo[a]); atomicMax(gbb + 3 + a, hi[a]); }
}

__device__ __forceinline__ double diag_of(const int* bb) {
    double e[3];
    for (int a = 0; a < 3; ++a) e[a] = (double)ord_dec(bb[3 + a]) - (double)ord_dec(bb[a]);
    return __dsqrt_rn((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
}

__global__ __launch_bounds__(THREADS) void mc_comp_decide_kernel(const int* __restrict__ cnt, const int* __restrict__ bb,
                                                                 const int* __restrict__ gbb, int C, int min_f,
                                                                 double min_d, int* __restrict__ drop) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= C) return;
    const double thr = (min_d / 100.0) * diag_of(gbb);
    drop[t] = (cnt[t] < min_f || diag_of(bb + 6 * (size_t)t) < thr) ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void mc_face_alive_kernel(const int* __restrict__ comp, const int* __restrict__ drop,
                                                                int F, int C, int* __restrict__ keep) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    const int c = comp[t];
    keep[t] = (c >= 0 && c < C && !drop[c]) ? 1 : 0;
}

// faces per undirected edge over the faces with keep[t] (keep NULL: every face)
__global__ __launch_bounds__(THREADS) void mc_edge_count_kernel(const int* __restrict__ node, const int* __restrict__ keep,
                                                                int F, int U, int* __restrict__ ecnt) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F || (keep && !keep[t])) return;
    for (int k = 0; k < 3; ++k) {
        const int e = node[3 * (size_t)t + k];
        if (e >= 0 && e < U) atomicAdd(ecnt + e, 1);
    }
}

__global__ __launch_bounds__(THREADS) void mc_cand_flag_kernel(const int* __restrict__ node, const int* __restrict__ keep,
                                                               const int* __restrict__ ecnt, int F, int U,
                                                               int* __restrict__ cand) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    bool c = false;
    if (keep[t])
        for (int k = 0; k < 3; ++k) {
            const int e = node[3 * (size_t)t + k];
            c = c || (e >= 0 && e < U && ecnt[e] > 2);
        }
    cand[t] = c ? 1 : 0;
}

// cand_key[crank[t]] = (bits of |g|) << 32 | the face's index after compaction (frank[t])
__global__ __launch_bounds__(THREADS) void mc_cand_key_kernel(const float* __restrict__ v, const int* __restrict__ f,
                                                              const int* __restrict__ crank, const int* __restrict__ frank,
                                                              int V, int F, long long* __restrict__ cand_key) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F || crank[t] < 0) return;
    int idx[3];
    float g[3] = {0.f, 0.f, 0.f};
    if (load_face(f, t, V, idx)) face_g(v, idx, g);
    // sqrtf is the correctly rounded root; __fsqrt_rn compiles to the bare v_sqrt_f32 (1 ulp), which reorders near-ties of R6
    const float gn = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    cand_key[crank[t]] = ((long long)__float_as_int(gn) << 32) | (long long)frank[t];
}

// ------------------------------------------------------------------ edges (R6)

// The candidates in key order on one lane: a candidate goes when one of its edges still has more than 2 faces.
__global__ __launch_bounds__(64) void mc_edge_pass_kernel(const int* __restrict__ node, const long long* __restrict__ key,
                                                          long long n, int F, int U, int* __restrict__ ecnt,
                                                          int* __restrict__ keep) {
    if (threadIdx.x != 0) return;
    for (long long q = 0; q < n; ++q) {
        const int t = (int)(key[q] & 0xffffffffLL);
        if (t < 0 || t >= F) continue;
        int e[3];
        bool ok = true, over = false;
        for (int k = 0; k < 3; ++k) {
            e[k] = node[3 * (size_t)t + k];
            ok = ok && e[k] >= 0 && e[k] < U;
        }
        if (!ok) continue;
        for (int k = 0; k < 3; ++k) over = over || ecnt[e[k]] > 2;
        if (!over) continue;
        keep[t] = 0;
        for (int k = 0; k < 3; ++k) ecnt[e[k]] -= 1;
    }
}

// ------------------------------------------------------------------ fans (R7) and the output (R8)

__global__ __launch_bounds__(THREADS) void mc_corner_a_kernel(const int* __restrict__ f, const int* __restrict__ fan, int n,
                                                              int V, int NF, int* __restrict__ ref, int* __restrict__ lowc,
                                                              int* __restrict__ firstc) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int x = f[c];
    if (x < 0 || x >= V) return;
    ref[x] = 1;
    if (!fan) return;
    atomicMin(lowc + x, c);
    const int k = fan[c];
    if (k >= 0 && k < NF) atomicMin(firstc + k, c);
}

__global__ __launch_bounds__(THREADS) void mc_corner_b_kernel(const int* __restrict__ f, const int* __restrict__ fan, int n,
                                                              int V, int NF, const int* __restrict__ firstc,
                                                              int* __restrict__ nfans) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int x = f[c], k = fan[c];
    if (x >= 0 && x < V && k >= 0 && k < NF && firstc[k] == c) atomicAdd(nfans + x, 1);
}

__global__ __launch_bounds__(THREADS) void mc_split_flag_kernel(const int* __restrict__ f, int n, int V,
                                                                const int* __restrict__ lowc, const int* __restrict__ nfans,
                                                                int* __restrict__ split) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int x = f[c];
    split[c] = (x >= 0 && x < V && lowc[x] == c && nfans[x] > 1) ? 1 : 0;
}

__global__ __launch_bounds__(THREADS) void mc_vmap_kernel(const int* __restrict__ newid, int V, long long* __restrict__ vmap) {
    const int x = blockIdx.x * THREADS + threadIdx.x;
    if (x < V && newid[x] >= 0) vmap[newid[x]] = x;
}

__global__ __launch_bounds__(THREADS) void mc_corner_out_kernel(const int* __restrict__ f, const int* __restrict__ fan, int n,
                                                                int V, const int* __restrict__ newid,
                                                                const int* __restrict__ lowc, const int* __restrict__ nfans,
                                                                const int* __restrict__ srank,
                                                                const long long* __restrict__ n_ref,
                                                                int* __restrict__ out, long long* __restrict__ vmap) {
    const int c = blockIdx.x * THREADS + threadIdx.x;
    if (c >= n) return;
    const int x = f[c];
    if (x < 0 || x >= V) { out[c] = -1; return; }
    int id = newid[x];
    if (fan && nfans[x] > 1) {
        const int l = lowc[x];
        if (fan[c] == fan[l]) id = (int)(*n_ref + srank[l]);
        if (l == c) vmap[*n_ref + srank[c]] = x;
    }
    out[c] = id;
}

}  // namespace

// ------------------------------------------------------------------ host side
namespace {

constexpr int64_t NCELLS = (int64_t)GRID_CAP * GRID_CAP * GRID_CAP;

// 8 int regions of M entries, 4 pairs of totals, the change flags of a batch of rounds
using Ws = MeshWs<8, 4, ROUND_BATCH>;

int64_t items(int V, int F) { return std::max<int64_t>({(int64_t)V, 3 * (int64_t)F, NCELLS + 1, 1}); }

int check_sizes(const char* name, int V, int F) {
    PRIMX_REQUIRE(V >= 0 && F >= 0, "%s: need V, F >= 0 (got %d, %d)", name, V, F);
    PRIMX_REQUIRE(3 * (int64_t)V < I31 && 9 * (int64_t)F < I31, "%s: 3 * V and 9 * F must be < 2^31 (got V = %d, F = %d)",
                  name, V, F);
    return PRIMX_OK;
}

float host_dec(int i) { return ord_dec(i); }

}  // namespace

extern "C" int primx_meshclean_workspace(int V, int F, int64_t* bytes) {
    PRIMX_REQUIRE(bytes, "primx_meshclean_workspace: null pointer");
    PRIMX_TRY(check_sizes("primx_meshclean_workspace", V, F));
    *bytes = (int64_t)Ws(items(V, F)).total;
    return PRIMX_OK;
}

extern "C" int primx_meshclean_merge(const float* v, const int* f, int V, int F, double v_pct, void* ws, int64_t ws_bytes,
                                     int* centre, int64_t* rounds, float* radius, void* stream) {
    const char* name = "primx_meshclean_merge";
    PRIMX_REQUIRE(rounds && radius, "%s: null pointer", name);
    PRIMX_TRY(check_sizes(name, V, F));
    PRIMX_REQUIRE(v_pct >= 0.0 && std::isfinite(v_pct), "%s: need a finite v_pct >= 0 (got %g)", name, v_pct);
    *rounds = 0;
    *radius = 0.f;
    if (V == 0) return PRIMX_OK;
    PRIMX_REQUIRE(v && centre && (F == 0 || f), "%s: null pointer", name);
    Ws w;
    PRIMX_TRY(check_ws(name, items(V, F), ws, ws_bytes, w));
    hipStream_t st = (hipStream_t)stream;
    int *ref = w.R(0), *st0 = w.R(1), *st1 = w.R(2), *captor = w.R(3), *cellof = w.R(4), *cursor = w.R(5), *start = w.R(6),
        *sorted = w.R(7), *bb = w.small();
    PRIMX_TRY(fill(ref, V, 0, st, name));
    if (F > 0) {
        hipLaunchKernelGGL(mc_ref_kernel, dim3(nblocks(3 * (int64_t)F, THREADS)), dim3(THREADS), 0, st, f, F, V, ref);
        PRIMX_CHECK_LAUNCH(name);
    }
    bool merged = false;
    if (v_pct > 0.0 && F > 0) {
        PRIMX_TRY(fill(bb, 3, INT_MAX, st, name));
        PRIMX_TRY(fill(bb + 3, 3, INT_MIN, st, name));
        hipLaunchKernelGGL(mc_bbox_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, st, v, (const int*)ref, V, bb);
        PRIMX_CHECK_LAUNCH(name);
        int h[6];
        PRIMX_TRY(readback(h, bb, sizeof(h), st, name));
        merged = h[0] != INT_MAX;
        if (merged) {
            double ext[3], emax = 0.0;
            Grid g;
            for (int a = 0; a < 3; ++a) {
                g.lo[a] = host_dec(h[a]);
                ext[a] = (double)host_dec(h[3 + a]) - (double)g.lo[a];
                emax = std::max(emax, ext[a]);
            }
            const double D = std::sqrt((ext[0] * ext[0] + ext[1] * ext[1]) + ext[2] * ext[2]);
            const float r = (float)((v_pct / 100.0) * D);
            const float r2 = r * r;
            *radius = r;
            const double wd = std::max({(double)r * 1.001, emax / (GRID_CAP - 1), 1e-30});
            g.inv = (float)(1.0 / wd);
            int64_t ncell = 1;
            for (int a = 0; a < 3; ++a) {
                g.d[a] = (int)std::min<double>(GRID_CAP, std::floor(ext[a] * (double)g.inv) + 1.0);
                g.d[a] = std::max(1, g.d[a]);
                ncell *= g.d[a];
            }
            PRIMX_TRY(fill(cursor, ncell + 1, 0, st, name));
            hipLaunchKernelGGL(mc_cell_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, st, v, (const int*)ref, V, g,
                               cellof, cursor);
            PRIMX_CHECK_LAUNCH(name);
            PRIMX_TRY(scan(cursor, (int)ncell + 1, false, start, cursor, w.bsum(), w.tot(0), st, name));
            hipLaunchKernelGGL(mc_scatter_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, st, (const int*)cellof, V,
                               cursor, sorted, st0, st1);
            PRIMX_CHECK_LAUNCH(name);
            int* buf[2] = {st0, st1};
            int cur = 0;
            int64_t done_rounds = -1, issued = 0;
            while (done_rounds < 0) {
                PRIMX_REQUIRE(issued <= 2 * (int64_t)V + ROUND_BATCH, "%s: no convergence after %lld rounds", name,
                              (long long)issued);
                PRIMX_TRY(zero(w.flags(), ROUND_BATCH * sizeof(int), st, name));
                for (int q = 0; q < ROUND_BATCH; ++q) {
                    hipLaunchKernelGGL(mc_round_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, st, v,
                                       (const int*)cellof, (const int*)start, (const int*)sorted, V, g, r2,
                                       (const int*)buf[cur], buf[cur ^ 1], captor, w.flags() + q);
                    PRIMX_CHECK_LAUNCH(name);
                    cur ^= 1;
                }
                int hf[ROUND_BATCH];
                PRIMX_TRY(readback(hf, w.flags(), sizeof(hf), st, name));
                for (int q = 0; q < ROUND_BATCH && done_rounds < 0; ++q)
                    if (hf[q] == 0) done_rounds = issued + q;   // a round without change: every later one too
                issued += ROUND_BATCH;
            }
            *rounds = done_rounds;
            st0 = buf[cur];
        }
    }
    hipLaunchKernelGGL(mc_centre_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, st, (const int*)st0,
                       (const int*)captor, (const int*)ref, V, (int)merged, centre);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_meshclean_faces(const float* v, const int* fr, const int* tid, int V, int F, void* ws, int64_t ws_bytes,
                                     int* out_f, int64_t* n_out, void* stream) {
    const char* name = "primx_meshclean_faces";
    PRIMX_REQUIRE(n_out, "%s: null pointer", name);
    PRIMX_TRY(check_sizes(name, V, F));
    *n_out = 0;
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(v && fr && tid && out_f, "%s: null pointer", name);
    PRIMX_REQUIRE(V >= 1, "%s: faces without vertices (V = 0)", name);
    Ws w;
    PRIMX_TRY(check_ws(name, items(V, F), ws, ws_bytes, w));
    hipStream_t st = (hipStream_t)stream;
    int *minface = w.R(0), *keep = w.R(1), *rank = w.R(2);
    PRIMX_TRY(fill(minface, F, INT_MAX, st, name));
    hipLaunchKernelGGL(mc_face_min_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, fr, tid, V, F, minface);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mc_face_keep_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, v, fr, tid,
                       (const int*)minface, V, F, keep);
    PRIMX_CHECK_LAUNCH(name);
    PRIMX_TRY(scan(keep, F, true, rank, nullptr, w.bsum(), w.tot(0), st, name));
    hipLaunchKernelGGL(mc_gather_rows_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, fr, (const int*)rank, F, 3,
                       out_f);
    PRIMX_CHECK_LAUNCH(name);
    long long h[2];
    PRIMX_TRY(readback(h, w.tot(0), sizeof(h), st, name));
    *n_out = h[0];
    return PRIMX_OK;
}

extern "C" int primx_meshclean_components(const float* v, const int* f, const int* node, const int* comp, int V, int F,
                                          int U, int n_comp, int min_f, double min_d, int repair, void* ws,
                                          int64_t ws_bytes, int* out_f, int* out_node, int64_t* cand_key,
                                          int64_t* counts, void* stream) {
    const char* name = "primx_meshclean_components";
    PRIMX_REQUIRE(counts, "%s: null pointer", name);
    PRIMX_TRY(check_sizes(name, V, F));
    PRIMX_REQUIRE(min_f >= 0 && min_d >= 0.0 && std::isfinite(min_d), "%s: need min_f >= 0 and a finite min_d >= 0 "
                  "(got %d, %g)", name, min_f, min_d);
    PRIMX_REQUIRE(n_comp >= 0 && n_comp <= F && U >= 0 && U <= 3 * (int64_t)F,
                  "%s: need 0 <= n_comp <= F and 0 <= U <= 3 F (got %d, %d, F = %d)", name, n_comp, U, F);
    counts[0] = counts[1] = counts[2] = 0;
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(v && f && node && comp && out_f && out_node && cand_key, "%s: null pointer", name);
    PRIMX_REQUIRE(V >= 1 && n_comp >= 1 && U >= 1, "%s: faces without vertices, components or edges", name);
    Ws w;
    PRIMX_TRY(check_ws(name, items(V, F), ws, ws_bytes, w));
    hipStream_t st = (hipStream_t)stream;
    // R0 cnt, R1-R2 boxes (6 n_comp <= 2 M), R3 drop, R4 face rank, R5 edge counts, R6 candidates, R7 scratch
    int *cnt = w.R(0), *bb = w.R(1), *drop = w.R(3), *frank = w.R(4), *ecnt = w.R(5), *cand = w.R(6), *scratch = w.R(7),
        *gbb = w.small();
    hipLaunchKernelGGL(mc_comp_init_kernel, dim3(nblocks(std::max(n_comp, 3), THREADS)), dim3(THREADS), 0, st, cnt, bb, n_comp,
                       gbb);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mc_comp_stats_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, v, f, comp, V, F, n_comp, cnt,
                       bb);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mc_comp_union_kernel, dim3(nblocks(n_comp, THREADS)), dim3(THREADS), 0, st, (const int*)bb, n_comp,
                       gbb);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mc_comp_decide_kernel, dim3(nblocks(n_comp, THREADS)), dim3(THREADS), 0, st, (const int*)cnt,
                       (const int*)bb, (const int*)gbb, n_comp, min_f, min_d, drop);
    PRIMX_CHECK_LAUNCH(name);
    PRIMX_TRY(scan(drop, n_comp, true, scratch, nullptr, w.bsum(), w.tot(1), st, name));
    int* alive = cnt;   // the counts are read: reuse the region for the face flags
    hipLaunchKernelGGL(mc_face_alive_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, comp, (const int*)drop, F,
                       n_comp, alive);
    PRIMX_CHECK_LAUNCH(name);
    PRIMX_TRY(scan(alive, F, true, frank, nullptr, w.bsum(), w.tot(0), st, name));
    hipLaunchKernelGGL(mc_gather_rows_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, f, (const int*)frank, F, 3,
                       out_f);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mc_gather_rows_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, node, (const int*)frank, F, 3,
                       out_node);
    PRIMX_CHECK_LAUNCH(name);
    if (repair) {
        PRIMX_TRY(fill(ecnt, U, 0, st, name));
        hipLaunchKernelGGL(mc_edge_count_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, node, (const int*)alive, F,
                           U, ecnt);
        PRIMX_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(mc_cand_flag_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, node, (const int*)alive,
                           (const int*)ecnt, F, U, cand);
        PRIMX_CHECK_LAUNCH(name);
        PRIMX_TRY(scan(cand, F, true, scratch, nullptr, w.bsum(), w.tot(2), st, name));
        hipLaunchKernelGGL(mc_cand_key_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, v, f, (const int*)scratch,
                           (const int*)frank, V, F, (long long*)cand_key);
        PRIMX_CHECK_LAUNCH(name);
    } else {
        PRIMX_TRY(zero(w.tot(2), 16, st, name));
    }
    long long h[6];
    PRIMX_TRY(readback(h, w.tot(0), sizeof(h), st, name));
    counts[0] = h[0];   // faces kept
    counts[1] = h[2];   // components removed
    counts[2] = h[4];   // R6 candidates
    return PRIMX_OK;
}

extern "C" int primx_meshclean_edges(const int* f, const int* node, int F, int U, const int64_t* cand_key, int64_t n_cand,
                                     void* ws, int64_t ws_bytes, int* out_f, int64_t* n_out, void* stream) {
    const char* name = "primx_meshclean_edges";
    PRIMX_REQUIRE(n_out, "%s: null pointer", name);
    PRIMX_TRY(check_sizes(name, 0, F));
    PRIMX_REQUIRE(U >= 0 && U <= 3 * (int64_t)F && n_cand >= 0 && n_cand <= F,
                  "%s: need 0 <= U <= 3 F and 0 <= n_cand <= F (got %d, %lld, F = %d)", name, U, (long long)n_cand, F);
    *n_out = 0;
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(f && node && out_f && (n_cand == 0 || cand_key), "%s: null pointer", name);
    PRIMX_REQUIRE(U >= 1, "%s: faces without edges (U = 0)", name);
    Ws w;
    PRIMX_TRY(check_ws(name, items(0, F), ws, ws_bytes, w));
    hipStream_t st = (hipStream_t)stream;
    int *ecnt = w.R(0), *keep = w.R(1), *rank = w.R(2);
    PRIMX_TRY(fill(ecnt, U, 0, st, name));
    PRIMX_TRY(fill(keep, F, 1, st, name));
    if (n_cand > 0) {
        hipLaunchKernelGGL(mc_edge_count_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, node, nullptr, F, U, ecnt);
        PRIMX_CHECK_LAUNCH(name);
        hipLaunchKernelGGL(mc_edge_pass_kernel, dim3(1), dim3(64), 0, st, node, (const long long*)cand_key,
                           (long long)n_cand, F, U, ecnt, keep);
        PRIMX_CHECK_LAUNCH(name);
    }
    PRIMX_TRY(scan(keep, F, true, rank, nullptr, w.bsum(), w.tot(0), st, name));
    hipLaunchKernelGGL(mc_gather_rows_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, f, (const int*)rank, F, 3,
                       out_f);
    PRIMX_CHECK_LAUNCH(name);
    long long h[2];
    PRIMX_TRY(readback(h, w.tot(0), sizeof(h), st, name));
    *n_out = h[0];
    return PRIMX_OK;
}

extern "C" int primx_meshclean_fans(const int* f, const int* fan, int V, int F, int n_fans, void* ws, int64_t ws_bytes,
                                    int* out_f, int64_t* vmap, int64_t* counts, void* stream) {
    const char* name = "primx_meshclean_fans";
    PRIMX_REQUIRE(counts, "%s: null pointer", name);
    PRIMX_TRY(check_sizes(name, V, F));
    PRIMX_REQUIRE(n_fans >= 0 && n_fans <= 3 * (int64_t)F, "%s: need 0 <= n_fans <= 3 F (got %d, F = %d)", name, n_fans, F);
    counts[0] = counts[1] = 0;
    if (F == 0) return PRIMX_OK;
    PRIMX_REQUIRE(f && out_f && vmap, "%s: null pointer", name);
    PRIMX_REQUIRE(V >= 1 && (!fan || n_fans >= 1), "%s: faces without vertices or fans", name);
    Ws w;
    PRIMX_TRY(check_ws(name, items(V, F), ws, ws_bytes, w));
    hipStream_t st = (hipStream_t)stream;
    const int n = 3 * F;
    int *nfans = w.R(0), *lowc = w.R(1), *ref = w.R(2), *firstc = w.R(3), *newid = w.R(4), *srank = w.R(5), *split = w.R(6);
    PRIMX_TRY(fill(nfans, V, 0, st, name));
    PRIMX_TRY(fill(lowc, V, INT_MAX, st, name));
    PRIMX_TRY(fill(ref, V, 0, st, name));
    PRIMX_TRY(fill(firstc, n_fans, INT_MAX, st, name));
    hipLaunchKernelGGL(mc_corner_a_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, f, fan, n, V, n_fans, ref, lowc,
                       firstc);
    PRIMX_CHECK_LAUNCH(name);
    if (fan) {
        hipLaunchKernelGGL(mc_corner_b_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, f, fan, n, V, n_fans,
                           (const int*)firstc, nfans);
        PRIMX_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(mc_split_flag_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, f, n, V, (const int*)lowc,
                       (const int*)nfans, split);
    PRIMX_CHECK_LAUNCH(name);
    PRIMX_TRY(scan(split, n, true, srank, nullptr, w.bsum(), w.tot(1), st, name));
    PRIMX_TRY(scan(ref, V, true, newid, nullptr, w.bsum(), w.tot(0), st, name));
    hipLaunchKernelGGL(mc_vmap_kernel, dim3(nblocks(V, THREADS)), dim3(THREADS), 0, st, (const int*)newid, V,
                       (long long*)vmap);
    PRIMX_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(mc_corner_out_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, f, fan, n, V,
                       (const int*)newid, (const int*)lowc, (const int*)nfans, (const int*)srank,
                       (const long long*)w.tot(0), out_f, (long long*)vmap);
    PRIMX_CHECK_LAUNCH(name);
    long long h[4];
    PRIMX_TRY(readback(h, w.tot(0), sizeof(h), st, name));
    counts[0] = h[0];   // referenced input vertices
    counts[1] = h[2];   // split vertices
    return PRIMX_OK;
}
