// Mesh extraction (inference.py:86-125): marching cubes over the PrimSDF lattice and the noise-primitive filter.
//
// Marching cubes over a [nx, ny, nz] fp32 lattice, linear index p = (i * ny + j) * nz + k (meshgrid 'ij', inference.py:108).
// Point p owns its +axis0 / +axis1 / +axis2 edges and the cell at its minimum corner; the case table (mc_tables.h) is
// generated from the rule stated in gen_mc_tables.py.  Output order is fixed - vertices by (owner point, axis), triangles by
// (cell, table order) - so the result is bitwise deterministic without atomics.  Four launches, no inter-workgroup hand-off:
//   1. classify: per point a packed word (cube index | vertex bits << 8 | triangle count << 11) + per-block sums;
//   2. scan:     ONE workgroup turns the block sums into exclusive block offsets and writes the two totals;
//   ----- the host reads the totals (one sync) and allocates exact outputs -----
//   3. vertices: block-local prefix (__ballot / mbcnt over 64 lanes), per-point vertex offset, then each vertex - position
//                in index coordinates (crossing axis at i0 + t, t = (iso - v0) / (v1 - v0)) and the unit normal of the
//                lattice gradient (central differences, one-sided at the borders) interpolated along the edge by t;
//   4. triangles: the cell's edges resolved to their owners' vertex offsets.
// Every block covers PTS = 1024 consecutive points, thread t the points base + r * 256 + t (r = 0..3), so the point order
// inside a block is (r, t) and the per-round prefix keeps it.
//
// The noise filter (inference.py:89-103) is bit-exact against torch on the CPU: FMA contraction is off in this file.
#include "common.h"
#include "mc_tables.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_common.h"

struct Dims {
    int nx, ny, nz;
    unsigned nynz, n;
};

__device__ __forceinline__ void decode(const Dims& d, unsigned p, int& i, int& j, int& k) {
    i = (int)(p / d.nynz);
    const unsigned r = p - (unsigned)i * d.nynz;
    j = (int)(r / (unsigned)d.nz);
    k = (int)(r - (unsigned)j * (unsigned)d.nz);
}

// offset of corner c (bit b at (b & 1, b >> 1 & 1, b >> 2 & 1)) from the cell's minimum corner
__device__ __forceinline__ unsigned corner_off(const Dims& d, int c) {
    return (c & 1) * d.nynz + ((c >> 1) & 1) * (unsigned)d.nz + ((c >> 2) & 1);
}

__global__ __launch_bounds__(THREADS) void mc_classify_kernel(const float* __restrict__ vol, Dims d, float iso,
                                                              unsigned* __restrict__ words, long long* __restrict__ bsum) {
    __shared__ int8_t s_ntri[256];
    s_ntri[threadIdx.x] = MC_NTRI[threadIdx.x];
    __syncthreads();
    int nv = 0, nt = 0;
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned p = blockIdx.x * (unsigned)PTS + r * THREADS + threadIdx.x;
        if (p >= d.n) continue;
        int i, j, k;
        decode(d, p, i, j, k);
        const bool in0 = vol[p] < iso;
        const bool xi = i + 1 < d.nx, xj = j + 1 < d.ny, xk = k + 1 < d.nz;
        const bool in1 = xi && (vol[p + d.nynz] < iso), in2 = xj && (vol[p + d.nz] < iso), in4 = xk && (vol[p + 1] < iso);
        const unsigned vb = (xi && in1 != in0 ? 1u : 0u) | (xj && in2 != in0 ? 2u : 0u) | (xk && in4 != in0 ? 4u : 0u);
        unsigned cube = 0;
        if (xi && xj && xk) {
            cube = (in0 ? 1u : 0u) | (in1 ? 2u : 0u) | (in2 ? 4u : 0u) | (in4 ? 16u : 0u);
            cube |= (vol[p + corner_off(d, 3)] < iso ? 8u : 0u) | (vol[p + corner_off(d, 5)] < iso ? 32u : 0u) |
                    (vol[p + corner_off(d, 6)] < iso ? 64u : 0u) | (vol[p + corner_off(d, 7)] < iso ? 128u : 0u);
        }
        const int t = s_ntri[cube];
        words[p] = cube | (vb << 8) | ((unsigned)t << 11);
        nv += __popc(vb);
        nt += t;
    }
    block_sums(nv, nt, bsum);
}

// d value / d axis at point p (index units): central differences inside, one-sided at the borders (np.gradient, edge_order 1)
__device__ __forceinline__ float grad1(const float* vol, unsigned p, unsigned stride, int i, int n) {
    if (i == 0) return vol[p + stride] - vol[p];
    if (i == n - 1) return vol[p] - vol[p - stride];
    return (vol[p + stride] - vol[p - stride]) * 0.5f;
}

__global__ __launch_bounds__(THREADS) void mc_vertices_kernel(const float* __restrict__ vol, Dims d, float iso,
                                                              const unsigned* __restrict__ words,
                                                              const long long* __restrict__ boff, int* __restrict__ voff,
                                                              float* __restrict__ verts, float* __restrict__ normals) {
    __shared__ int s_wave[THREADS / 64];
    long long run = boff[2 * (size_t)blockIdx.x];
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned p = blockIdx.x * (unsigned)PTS + r * THREADS + threadIdx.x;
        const bool live = p < d.n;
        const unsigned vb = live ? (words[p] >> 8) & 7u : 0u;
        int tot;
        const int pre = block_prefix3(__popc(vb), s_wave, tot);
        long long o = run + pre;
        run += tot;
        if (vb == 0) continue;
        voff[p] = (int)o;
        int c[3];
        decode(d, p, c[0], c[1], c[2]);
        const int n[3] = {d.nx, d.ny, d.nz};
        const unsigned st[3] = {d.nynz, (unsigned)d.nz, 1u};
        const float v0 = vol[p];
        float g0[3];
        if (normals)
            for (int b = 0; b < 3; ++b) g0[b] = grad1(vol, p, st[b], c[b], n[b]);
        for (int a = 0; a < 3; ++a) {
            if (!((vb >> a) & 1u)) continue;
            const unsigned q = p + st[a];
            const float t = __fdiv_rn(iso - v0, vol[q] - v0);
            float* vp = verts + 3 * o;
            vp[0] = (float)c[0] + (a == 0 ? t : 0.f);
            vp[1] = (float)c[1] + (a == 1 ? t : 0.f);
            vp[2] = (float)c[2] + (a == 2 ? t : 0.f);
            if (normals) {
                float g[3];
                for (int b = 0; b < 3; ++b) {
                    const float g1 = grad1(vol, q, st[b], c[b] + (b == a ? 1 : 0), n[b]);
                    g[b] = (1.f - t) * g0[b] + t * g1;
                }
                const float l2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
                const float inv = l2 > 0.f ? __fdiv_rn(1.f, __fsqrt_rn(l2)) : 0.f;
                float* np_ = normals + 3 * o;
                np_[0] = g[0] * inv;
                np_[1] = g[1] * inv;
                np_[2] = g[2] * inv;
            }
            ++o;
        }
    }
}

__global__ __launch_bounds__(THREADS) void mc_triangles_kernel(Dims d, const unsigned* __restrict__ words,
                                                               const long long* __restrict__ boff,
                                                               const int* __restrict__ voff, int* __restrict__ tris) {
    __shared__ int8_t s_tri[256 * 16];
    __shared__ unsigned s_eoff[12];
    __shared__ int s_wave[THREADS / 64];
    for (int q = threadIdx.x; q < 256 * 16; q += THREADS) s_tri[q] = MC_TRI[q >> 4][q & 15];
    if (threadIdx.x < 12) s_eoff[threadIdx.x] = corner_off(d, MC_EDGE_CORNER[threadIdx.x]);   // edge -> its owner point
    __syncthreads();
    long long run = boff[2 * (size_t)blockIdx.x + 1];
    for (int r = 0; r < ROUNDS; ++r) {
        const unsigned p = blockIdx.x * (unsigned)PTS + r * THREADS + threadIdx.x;
        const unsigned w = p < d.n ? words[p] : 0u;
        const int nt = (int)((w >> 11) & 7u);
        int tot;
        const int pre = block_prefix3(nt, s_wave, tot);
        int* out = tris + 3 * (run + pre);
        run += tot;
        const int8_t* row = s_tri + 16 * (w & 255u);
        for (int e3 = 0; e3 < 3 * nt; ++e3) {
            const int e = row[e3];
            const int axis = MC_EDGE_AXIS[e];
            const unsigned owner = p + s_eoff[e];
            const unsigned ovb = (words[owner] >> 8) & 7u;
            out[e3] = voff[owner] + __popc(ovb & ((1u << axis) - 1u));
        }
    }
}

__global__ __launch_bounds__(THREADS) void noise_filter_kernel(const float* __restrict__ srt, int P,
                                                               uint8_t* __restrict__ keep) {
    __shared__ float4 s_prim[THREADS];
    const int i = blockIdx.x * THREADS + threadIdx.x;
    const bool live = i < P;
    float4 me = live ? reinterpret_cast<const float4*>(srt)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float best = 0.f;
    int best_j = -1;
    for (int j0 = 0; j0 < P; j0 += THREADS) {
        __syncthreads();
        if (j0 + (int)threadIdx.x < P) s_prim[threadIdx.x] = reinterpret_cast<const float4*>(srt)[j0 + threadIdx.x];
        __syncthreads();
        if (!live) continue;
        const int cnt = min(THREADS, P - j0);
        for (int t = 0; t < cnt; ++t) {
            const float4 q = s_prim[t];
            const float dx = me.y - q.y, dy = me.z - q.z, dz = me.w - q.w;
            float dist = sqrtf((dx * dx + dy * dy) + dz * dz);   // sum(-1) of a 3-element row: (x + y) + z; correctly rounded as torch.sqrt
            dist = dist + (j0 + t == i ? 1.f : 0.f);                  // dist += eye
            if (best_j < 0 || dist < best) { best = dist; best_j = j0 + t; }   // min(1): first index on ties
        }
    }
    if (live) keep[i] = best < me.x + srt[4 * (size_t)best_j] ? 1 : 0;
}

}  // namespace

// ------------------------------------------------------------------ host side
namespace {

struct Layout {
    size_t words, voff, bsum, total;
    int nblk;
};

Layout layout(int nx, int ny, int nz) {
    const size_t n = (size_t)nx * ny * nz;
    Layout l;
    Arena a;
    l.nblk = nblocks(n, PTS);
    l.words = a.take(n * 4);
    l.voff = a.take(n * 4);
    l.bsum = a.take((size_t)l.nblk * 16);
    l.total = a.total;
    return l;
}

int check_dims(const char* name, int nx, int ny, int nz) {
    PRIMX_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: need nx, ny, nz >= 2 (got %d, %d, %d)", name, nx, ny, nz);
    PRIMX_REQUIRE(3 * (int64_t)nx * ny * nz < ((int64_t)1 << 31), "%s: 3 * nx * ny * nz must be < 2^31 (got %d x %d x %d)",
                  name, nx, ny, nz);
    return PRIMX_OK;
}

Dims dims(int nx, int ny, int nz) {
    Dims d;
    d.nx = nx; d.ny = ny; d.nz = nz;
    d.nynz = (unsigned)ny * (unsigned)nz;
    d.n = d.nynz * (unsigned)nx;
    return d;
}

}  // namespace

extern "C" int primx_mcubes_workspace(int nx, int ny, int nz, int64_t* bytes) {
    PRIMX_REQUIRE(bytes, "primx_mcubes_workspace: null pointer");
    PRIMX_TRY(check_dims("primx_mcubes_workspace", nx, ny, nz));
    *bytes = (int64_t)layout(nx, ny, nz).total;
    return PRIMX_OK;
}

extern "C" int primx_mcubes_count(const float* vol, int nx, int ny, int nz, float iso, void* ws, int64_t ws_bytes,
                                  int64_t* totals, void* stream) {
    PRIMX_REQUIRE(vol && ws && totals, "primx_mcubes_count: null pointer");
    PRIMX_TRY(check_dims("primx_mcubes_count", nx, ny, nz));
    const Layout l = layout(nx, ny, nz);
    PRIMX_REQUIRE(ws_bytes >= (int64_t)l.total, "primx_mcubes_count: workspace of %lld bytes, need %lld",
                  (long long)ws_bytes, (long long)l.total);
    char* w = (char*)ws;
    hipLaunchKernelGGL(mc_classify_kernel, dim3(l.nblk), dim3(THREADS), 0, (hipStream_t)stream, vol, dims(nx, ny, nz), iso,
                       (unsigned*)(w + l.words), (long long*)(w + l.bsum));
    PRIMX_CHECK_LAUNCH("primx_mcubes_count (classify)");
    return scan_blocks((long long*)(w + l.bsum), l.nblk, (long long*)totals, (hipStream_t)stream, "primx_mcubes_count (scan)");
}

extern "C" int primx_mcubes_emit(const float* vol, int nx, int ny, int nz, float iso, const void* ws, int64_t ws_bytes,
                                 int64_t nverts, int64_t ntris, float* verts, float* normals, int* tris, void* stream) {
    PRIMX_REQUIRE(vol && ws, "primx_mcubes_emit: null pointer");
    PRIMX_TRY(check_dims("primx_mcubes_emit", nx, ny, nz));
    const Layout l = layout(nx, ny, nz);
    PRIMX_REQUIRE(ws_bytes >= (int64_t)l.total, "primx_mcubes_emit: workspace of %lld bytes, need %lld",
                  (long long)ws_bytes, (long long)l.total);
    PRIMX_REQUIRE(nverts >= 0 && ntris >= 0 && nverts <= 3 * (int64_t)nx * ny * nz,
                  "primx_mcubes_emit: counts (%lld, %lld) are not those of primx_mcubes_count", (long long)nverts,
                  (long long)ntris);
    if (nverts == 0 && ntris == 0) return PRIMX_OK;   // empty or full volume: nothing past the scan
    PRIMX_REQUIRE(verts && tris, "primx_mcubes_emit: null pointer");
    char* w = (char*)ws;
    const Dims d = dims(nx, ny, nz);
    hipLaunchKernelGGL(mc_vertices_kernel, dim3(l.nblk), dim3(THREADS), 0, (hipStream_t)stream, vol, d, iso,
                       (const unsigned*)(w + l.words), (const long long*)(w + l.bsum), (int*)(w + l.voff), verts, normals);
    PRIMX_CHECK_LAUNCH("primx_mcubes_emit (vertices)");
    hipLaunchKernelGGL(mc_triangles_kernel, dim3(l.nblk), dim3(THREADS), 0, (hipStream_t)stream, d,
                       (const unsigned*)(w + l.words), (const long long*)(w + l.bsum), (const int*)(w + l.voff), tris);
    PRIMX_CHECK_LAUNCH("primx_mcubes_emit (triangles)");
    return PRIMX_OK;
}

extern "C" int primx_noise_filter(const float* srt, int P, uint8_t* keep, void* stream) {
    PRIMX_REQUIRE(srt && keep, "primx_noise_filter: null pointer");
    PRIMX_REQUIRE(P > 0, "primx_noise_filter: need P > 0 (got %d)", P);
    hipLaunchKernelGGL(noise_filter_kernel, dim3(nblocks(P, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, srt, P,
                       keep);
    PRIMX_CHECK_LAUNCH("primx_noise_filter");
    return PRIMX_OK;
}
