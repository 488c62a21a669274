// Primitive fitting (the initialisation the 3DTopia-XL paper describes; the reference's PrimSDF._init_param is an empty
// `pass`, models/primsdf.py:48-50): mesh field query, face areas, area-weighted surface samples and farthest point sampling.
// Rules and the C ABI: include/primx_hip.h "Primitive fitting"; float64 / float32 restatement: tests/meshfield_numpy.py.
//
//   query:   (the per-pair arithmetic, the record and its preparation launch: meshfield_pair.h, shared with meshbvh.hip)
//            a preparation launch turns every face into a 64-byte record (a, b, c, b - a, c - a, kind) and flags indices
//            outside [0, V); the host reads the flag back and refuses the call before the query launch.  The query kernel
//            runs one thread per point (64-bit point index); a block streams the records through LDS in chunks of
//            MF_CHUNK and every lane reads the same record (a broadcast read).  Brute force over F by design.
//   areas:   one float64 per face.
//   points:  binary search of the inclusive float64 CDF, then the square-root placement, fp32.
//   fps:     one launch per chosen centre: the prologue of launch k reduces the partial argmaxes launch k - 1 left (every
//            block does, redundantly: no block waits on another), the body updates the running minima of the block's
//            slice and leaves its partial argmax.  No host synchronisation inside the loop; then one launch for `nn`.
//
// Every floating-point expression is evaluated as written (no contraction), so the bit-exact parts (areas, points, fps, nn)
// equal the numpy restatement and the query's fp32 error is the restatement's own fp32 error.
#include <cmath>
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_common.h"

constexpr int MF_CHUNK = 256;            // triangle records per LDS chunk (16 KiB)
constexpr int FPS_MAXB = 256;            // blocks of an fps launch at most (= partial argmaxes per parity)
constexpr int FPS_PER_BLOCK = 1024;      // candidates per block at least

#include "meshfield_pair.h"

__global__ __launch_bounds__(THREADS) void mf_query_kernel(const float* __restrict__ pts, int64_t n,
                                                           const float4* __restrict__ recs, int F,
                                                           const int* __restrict__ f, const float* __restrict__ attr, int C,
                                                           float* __restrict__ dist, int* __restrict__ face,
                                                           float* __restrict__ wn, float* __restrict__ out_attr) {
    __shared__ float4 lds[MF_CHUNK * 4];
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const bool live = i < n;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (live) px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    float best = INFINITY, acc = 0.0f;
    int bf = 0;
    for (int base = 0; base < F; base += MF_CHUNK) {
        const int cnt = min(MF_CHUNK, F - base);
        __syncthreads();                                     // the previous chunk has been read by every wave
        for (int k = threadIdx.x; k < cnt * 4; k += THREADS) lds[k] = recs[(int64_t)base * 4 + k];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const Rec r = unpack(lds + 4 * j);               // the same address in every lane: a broadcast read
            const int kind = __builtin_amdgcn_readfirstlane(r.kind);
            float d2, v, w, term;
            pair(px, py, pz, r, kind, d2, v, w, term);
            if (d2 < best) best = d2, bf = base + j;         // the first minimum wins
            acc += term;
        }
    }
    if (!live) return;
    dist[i] = sqrtf(best);
    face[i] = bf;
    wn[i] = acc * 0.15915494309189535f;                      // 2 sum / (4 pi)
    if (C > 0) {
        const Rec r = unpack(recs + (int64_t)4 * bf);
        float d2, v, w, term;
        pair(px, py, pz, r, r.kind, d2, v, w, term);
        const float u = (1.0f - v) - w;
        const float* ga = attr + (int64_t)f[(int64_t)3 * bf] * C;
        const float* gb = attr + (int64_t)f[(int64_t)3 * bf + 1] * C;
        const float* gc = attr + (int64_t)f[(int64_t)3 * bf + 2] * C;
        for (int c = 0; c < C; ++c) out_attr[i * C + c] = (ga[c] * u + gb[c] * v) + gc[c] * w;
    }
}

__global__ __launch_bounds__(THREADS) void mf_area_kernel(const float* __restrict__ v, const int* __restrict__ f, int V, int F,
                                                          double* __restrict__ area, int* __restrict__ status) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    const int i0 = f[(int64_t)3 * t], i1 = f[(int64_t)3 * t + 1], i2 = f[(int64_t)3 * t + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
        atomicOr(status, 1);
        area[t] = 0.0;
        return;
    }
    const double ax = v[(int64_t)3 * i0], ay = v[(int64_t)3 * i0 + 1], az = v[(int64_t)3 * i0 + 2];
    const double abx = (double)v[(int64_t)3 * i1] - ax, aby = (double)v[(int64_t)3 * i1 + 1] - ay, abz = (double)v[(int64_t)3 * i1 + 2] - az;
    const double acx = (double)v[(int64_t)3 * i2] - ax, acy = (double)v[(int64_t)3 * i2 + 1] - ay, acz = (double)v[(int64_t)3 * i2 + 2] - az;
    const double nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    area[t] = 0.5 * sqrt((nx * nx + ny * ny) + nz * nz);
}

__global__ __launch_bounds__(THREADS) void mf_points_kernel(const float* __restrict__ v, const int* __restrict__ f, int V, int F,
                                                            const double* __restrict__ cdf, const float* __restrict__ u,
                                                            int64_t N, float* __restrict__ pts, int* __restrict__ face,
                                                            int* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= N) return;
    const float u0 = u[3 * i], u1 = u[3 * i + 1], u2 = u[3 * i + 2];
    const double target = (double)u0 * cdf[F - 1];
    int lo = 0, hi = F - 1;                                  // the first face whose cdf exceeds the target (the last if none)
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cdf[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    face[i] = lo;
    const int i0 = f[(int64_t)3 * lo], i1 = f[(int64_t)3 * lo + 1], i2 = f[(int64_t)3 * lo + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
        atomicOr(status, 1);
        pts[3 * i] = 0.0f, pts[3 * i + 1] = 0.0f, pts[3 * i + 2] = 0.0f;
        return;
    }
    const float r = sqrtf(u1);
    const float w0 = 1.0f - r, w1 = r * (1.0f - u2), w2 = r * u2;
    for (int k = 0; k < 3; ++k)
        pts[3 * i + k] = (w0 * v[(int64_t)3 * i0 + k] + w1 * v[(int64_t)3 * i1 + k]) + w2 * v[(int64_t)3 * i2 + k];
}

// ------------------------------------------------------------------------------------------------ farthest point sampling
__device__ __forceinline__ unsigned long long block_max(unsigned long long k, unsigned long long* red) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(k, o);
        k = other > k ? other : k;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = k;
    __syncthreads();
    k = red[0];
    for (int wv = 1; wv < THREADS / 64; ++wv) k = red[wv] > k ? red[wv] : k;
    __syncthreads();
    return k;
}

// key of candidate i with running minimum m >= 0: larger m first, then the lower index; 0 = no candidate
__device__ __forceinline__ unsigned long long fps_key(float m, int i) {
    return ((unsigned long long)__float_as_uint(m) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
}

__global__ __launch_bounds__(THREADS) void fps_iter_kernel(const float* __restrict__ pts, int N, int it, int start, int nblk,
                                                           int per, float* __restrict__ mind,
                                                           unsigned long long* __restrict__ part, int* __restrict__ idx) {
    __shared__ unsigned long long red[THREADS / 64];
    int c = start;
    if (it > 0) {
        const unsigned long long* prev = part + ((it - 1) & 1) * FPS_MAXB;
        unsigned long long k = (int)threadIdx.x < nblk ? prev[threadIdx.x] : 0ull;
        k = block_max(k, red);
        c = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
        if ((unsigned)c >= (unsigned)N) c = 0;               // cannot happen for finite input: every block left a candidate's key
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) idx[it] = c;
    const float cx = pts[(int64_t)3 * c], cy = pts[(int64_t)3 * c + 1], cz = pts[(int64_t)3 * c + 2];
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < N ? lo + per : N;
    unsigned long long key = 0ull;
    for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
        const float dx = pts[3 * i] - cx, dy = pts[3 * i + 1] - cy, dz = pts[3 * i + 2] - cz;
        float m = (dx * dx + dy * dy) + dz * dz;
        if (it > 0) m = fminf(mind[i], m);
        mind[i] = m;
        const unsigned long long k = fps_key(m, (int)i);
        key = k > key ? k : key;
    }
    key = block_max(key, red);
    if (threadIdx.x == 0) part[(it & 1) * FPS_MAXB + blockIdx.x] = key;
}

__global__ __launch_bounds__(THREADS) void fps_nn_kernel(const float* __restrict__ pts, const int* __restrict__ idx, int K,
                                                         float* __restrict__ nn) {
    __shared__ float cen[THREADS * 3];
    const int k = blockIdx.x * THREADS + threadIdx.x;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (k < K) {
        const int64_t c = idx[k];
        x = pts[3 * c], y = pts[3 * c + 1], z = pts[3 * c + 2];
    }
    float best = INFINITY;
    for (int base = 0; base < K; base += THREADS) {
        const int cnt = min(THREADS, K - base);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const int64_t c = idx[base + threadIdx.x];
            cen[3 * threadIdx.x] = pts[3 * c], cen[3 * threadIdx.x + 1] = pts[3 * c + 1], cen[3 * threadIdx.x + 2] = pts[3 * c + 2];
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float dx = cen[3 * j] - x, dy = cen[3 * j + 1] - y, dz = cen[3 * j + 2] - z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (base + j != k) best = fminf(best, d2);
        }
    }
    if (k < K) nn[k] = K > 1 ? sqrtf(best) : 0.0f;
}

}  // namespace

extern "C" int primx_mesh_field_query(const float* pts, int64_t n, const float* v, const int* f, int V, int F,
                                      const float* attr, int C, void* ws, int64_t ws_bytes, float* dist, int* face, float* wn,
                                      float* out_attr, void* stream) {
    const char* name = "primx_mesh_field_query";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_TRY(check_mesh(name, v, f, V, F));
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX * THREADS, "%s: n out of range", name);
    PRIMX_REQUIRE(C >= 0 && C <= 16, "%s: C must lie in 0 .. 16 (got %d)", name, C);
    PRIMX_REQUIRE(C == 0 || attr, "%s: null attribute pointer with C = %d", name, C);
    PRIMX_REQUIRE(ws && ((uintptr_t)ws & 15) == 0 && ws_bytes >= WS_HEAD + (int64_t)64 * F,
                  "%s: the workspace needs 64 + 64 F bytes, 16-byte aligned", name);
    PRIMX_REQUIRE(n == 0 || (pts && dist && face && wn && (C == 0 || out_attr)), "%s: null pointer", name);
    int* status = (int*)ws;
    float4* recs = (float4*)((char*)ws + WS_HEAD);
    PRIMX_TRY(zero(status, sizeof(int), st, name));
    hipLaunchKernelGGL(mf_prep_kernel<false>, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, v, f, V, F, (const int*)nullptr, recs,
                       status);
    PRIMX_CHECK_LAUNCH(name);
    int flag = 0;
    PRIMX_TRY(readback(&flag, status, sizeof(flag), st, name));
    PRIMX_REQUIRE(flag == 0, "%s: a face index lies outside [0, V)", name);
    if (n == 0) return PRIMX_OK;
    hipLaunchKernelGGL(mf_query_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, pts, n, (const float4*)recs, F, f, attr,
                       C, dist, face, wn, out_attr);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_mesh_face_areas(const float* v, const int* f, int V, int F, double* area, int* status, void* stream) {
    const char* name = "primx_mesh_face_areas";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_TRY(check_mesh(name, v, f, V, F));
    PRIMX_REQUIRE(area && status, "%s: null pointer", name);
    PRIMX_TRY(zero(status, sizeof(int), st, name));
    hipLaunchKernelGGL(mf_area_kernel, dim3(nblocks(F, THREADS)), dim3(THREADS), 0, st, v, f, V, F, area, status);
    PRIMX_CHECK_LAUNCH(name);
    int flag = 0;
    PRIMX_TRY(readback(&flag, status, sizeof(flag), st, name));
    PRIMX_REQUIRE(flag == 0, "%s: a face index lies outside [0, V)", name);
    return PRIMX_OK;
}

extern "C" int primx_mesh_surface_points(const float* v, const int* f, int V, int F, const double* cdf, const float* u, int64_t N,
                                         float* pts, int* face, int* status, void* stream) {
    const char* name = "primx_mesh_surface_points";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_TRY(check_mesh(name, v, f, V, F));
    PRIMX_REQUIRE(cdf && status, "%s: null pointer", name);
    PRIMX_REQUIRE(N >= 0 && N <= (int64_t)INT32_MAX * THREADS, "%s: N out of range", name);
    if (N == 0) return PRIMX_OK;
    PRIMX_REQUIRE(u && pts && face, "%s: null pointer", name);
    PRIMX_TRY(zero(status, sizeof(int), st, name));
    hipLaunchKernelGGL(mf_points_kernel, dim3(nblocks(N, THREADS)), dim3(THREADS), 0, st, v, f, V, F, cdf, u, N, pts, face, status);
    PRIMX_CHECK_LAUNCH(name);
    int flag = 0;
    PRIMX_TRY(readback(&flag, status, sizeof(flag), st, name));
    PRIMX_REQUIRE(flag == 0, "%s: a face index lies outside [0, V)", name);
    return PRIMX_OK;
}

extern "C" int primx_fps(const float* pts, int N, int K, int start, void* ws, int64_t ws_bytes, int* idx, float* nn,
                         void* stream) {
    const char* name = "primx_fps";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_REQUIRE(pts && idx && nn, "%s: null pointer", name);
    PRIMX_REQUIRE(N >= 1 && N <= INT32_MAX / 3, "%s: N must lie in 1 .. (2^31 - 1) / 3 (got %d)", name, N);
    PRIMX_REQUIRE(K >= 1 && K <= N, "%s: K must lie in 1 .. N (got %d of %d)", name, K, N);
    PRIMX_REQUIRE(start >= 0 && start < N, "%s: start must lie in [0, N) (got %d)", name, start);
    const int64_t mind_bytes = ((int64_t)4 * N + 7) & ~(int64_t)7;
    PRIMX_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= mind_bytes + 2 * FPS_MAXB * 8,
                  "%s: the workspace needs 4 N (rounded up to 8) + 4096 bytes, 8-byte aligned", name);
    float* mind = (float*)ws;
    unsigned long long* part = (unsigned long long*)((char*)ws + mind_bytes);
    int per = (N + FPS_MAXB - 1) / FPS_MAXB;
    if (per < FPS_PER_BLOCK) per = FPS_PER_BLOCK;
    const int nblk = (N + per - 1) / per;
    for (int it = 0; it < K; ++it) {
        hipLaunchKernelGGL(fps_iter_kernel, dim3(nblk), dim3(THREADS), 0, st, pts, N, it, start, nblk, per, mind, part, idx);
        PRIMX_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(fps_nn_kernel, dim3(nblocks(K, THREADS)), dim3(THREADS), 0, st, pts, (const int*)idx, K, nn);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}
