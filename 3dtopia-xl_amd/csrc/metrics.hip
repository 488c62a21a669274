// Quality metrics (no counterpart in the reference, which has no evaluation code): the nearest neighbour of every point of one
// set in another, and the deterministic reduction of per-point distances into the sums, the maximum and the threshold counts
// that Chamfer distance, F-score, Hausdorff distance and normal consistency are made of.
// Rules and the C ABI: include/primx_hip.h "Quality metrics"; float64 / float32 restatement: tests/metrics_numpy.py.
//
//   nearest: brute force over b by design, as the mesh query is.  A block of THREADS threads carries PPT points of `a` per thread
//            (point base + r * THREADS + t in round r, 64-bit index) and streams b through LDS in chunks of NN_CHUNK points, kept as
//            b holds them (12 bytes a point); four points are three float4 reads at addresses every lane shares (broadcast reads),
//            so a point costs 3 LDS cycles per wave where one 12-byte read of its own costs 8, and those reads and one loop step
//            serve 4 PPT pairs.  No n x m matrix, no workspace, no atomics: the same bits on every run, and for every PPT.
//            A pair costs 11 VALU operations (3 subtractions, 3 products, 2 sums, compare, 2 selects) whatever PPT is; the LDS
//            reads, their wait and the loop step are shared by 4 PPT pairs.  Measured (DESIGN.md "Quality metrics"): four points
//            per thread are 10 to 13 % faster than one from 5 10^5 points on, 1.3 x slower at 3 10^5 and 1.9 x at 10^5, where they leave
//            SIMDs with one wave or none (a SIMD issues one wave's VALU instruction every 4 cycles and two waves' every 2).  The
//            host takes PPT = 4 from NN_WIDE points on and 1 below.
//   stats:   two launches.  Every block of the first reduces one contiguous slice in float64 - thread t the elements
//            lo + t, lo + t + THREADS, ... in that order, then the lanes of a wave by xor-shuffles 32, 16, .. 1, then the waves in
//            wave order - and writes ST_ROW partials; one block of the second adds the blocks' partials in block order.  No
//            floating-point atomics: two runs give the same 64-bit patterns.
//
// Every floating-point expression is evaluated as written (no contraction).
#include <cmath>
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_common.h"

constexpr int NN_CHUNK = 1024;           // points of b per LDS chunk (12 KiB); a multiple of 4
constexpr int NN_WIDE = 409600;          // points of a from which a thread carries four of them (400 blocks of 1024 points)
constexpr int ST_MAXB = 256;             // blocks of the first stats launch at most (= rows of partials in ws)
constexpr int ST_PER_BLOCK = 1024;       // elements per block at least
constexpr int ST_MAXT = 8;               // thresholds at most
constexpr int ST_ROW = 4 + ST_MAXT;      // doubles per row of partials: sum, sum of squares, max, normal sum, counts

struct Taus {
    float v[ST_MAXT];
};

template <int PPT>                       // points of a per thread: 1 or 4
__global__ __launch_bounds__(THREADS) void nn_kernel(const float* __restrict__ a, int64_t n, const float* __restrict__ b, int m,
                                                     float* __restrict__ dist, int* __restrict__ idx) {
    __shared__ float4 lds[NN_CHUNK * 3 / 4];                  // the chunk's 3 * NN_CHUNK floats as b holds them
    float* ldsf = (float*)lds;
    const int64_t first = (int64_t)blockIdx.x * (THREADS * PPT) + threadIdx.x;
    float px[PPT], py[PPT], pz[PPT], best[PPT];
    int bi[PPT];
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        const int64_t i = first + (int64_t)r * THREADS;
        px[r] = 0.0f, py[r] = 0.0f, pz[r] = 0.0f;
        if (i < n) px[r] = a[3 * i], py[r] = a[3 * i + 1], pz[r] = a[3 * i + 2];
        best[r] = INFINITY, bi[r] = 0;
    }
    for (int base = 0; base < m; base += NN_CHUNK) {
        const int cnt = min(NN_CHUNK, m - base);
        const int cnt4 = (cnt + 3) & ~3;                     // up to 3 points of padding at +inf: their d2 is +inf or NaN and never wins
        __syncthreads();                                     // the previous chunk has been read by every wave
        for (int k = threadIdx.x; k < 3 * cnt4; k += THREADS) ldsf[k] = k < 3 * cnt ? b[(int64_t)3 * base + k] : INFINITY;
        __syncthreads();
        for (int j = 0; j < cnt4; j += 4) {
            // four points of b = three float4: the same addresses in every lane, broadcast reads of 16 bytes
            const float4 q0 = lds[3 * (j >> 2)], q1 = lds[3 * (j >> 2) + 1], q2 = lds[3 * (j >> 2) + 2];
            const float bx[4] = {q0.x, q0.w, q1.z, q2.y}, by[4] = {q0.y, q1.x, q1.w, q2.z}, bz[4] = {q0.z, q1.y, q2.x, q2.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int r = 0; r < PPT; ++r) {
                    const float dx = px[r] - bx[u], dy = py[r] - by[u], dz = pz[r] - bz[u];
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (d2 < best[r]) best[r] = d2, bi[r] = base + j + u;   // the first minimum wins; a NaN never does
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        const int64_t i = first + (int64_t)r * THREADS;
        if (i < n) dist[i] = sqrtf(best[r]), idx[i] = bi[r];
    }
}

// the lanes of a wave by xor-shuffles, then the waves in wave order; the result in every thread.  Every thread calls it.
__device__ __forceinline__ double block_sum(double x, double* red) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    __syncthreads();                                         // `red` of the previous call has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    x = red[0];
    for (int w = 1; w < THREADS / 64; ++w) x += red[w];
    return x;
}

__device__ __forceinline__ double block_maxd(double x, double* red) {
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    x = red[0];
    for (int w = 1; w < THREADS / 64; ++w) x = fmax(x, red[w]);
    return x;
}

__global__ __launch_bounds__(THREADS) void st_part_kernel(const float* __restrict__ dist, const int* __restrict__ idx,
                                                          const float* __restrict__ na, const float* __restrict__ nb, int64_t n,
                                                          int64_t per, Taus tau, int T, double* __restrict__ part) {
    __shared__ double red[THREADS / 64];
    const int64_t lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < n ? lo + per : n;
    const bool normals = na != nullptr && nb != nullptr;
    double s1 = 0.0, s2 = 0.0, mx = 0.0, sn = 0.0, cnt[ST_MAXT];
#pragma unroll
    for (int t = 0; t < ST_MAXT; ++t) cnt[t] = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += THREADS) {
        const float d = dist[i];
        const double dd = (double)d;
        s1 += dd;
        s2 += dd * dd;
        mx = fmax(mx, dd);                                   // from 0; a NaN is passed over
#pragma unroll
        for (int t = 0; t < ST_MAXT; ++t)
            if (t < T && d <= tau.v[t]) cnt[t] += 1.0;
        if (normals) {
            const int64_t k = idx[i];
            const float dot = (na[3 * i] * nb[3 * k] + na[3 * i + 1] * nb[3 * k + 1]) + na[3 * i + 2] * nb[3 * k + 2];
            sn += (double)fabsf(dot);
        }
    }
    s1 = block_sum(s1, red), s2 = block_sum(s2, red), mx = block_maxd(mx, red), sn = block_sum(sn, red);
#pragma unroll
    for (int t = 0; t < ST_MAXT; ++t) cnt[t] = block_sum(cnt[t], red);
    if (threadIdx.x == 0) {
        double* o = part + (int64_t)ST_ROW * blockIdx.x;
        o[0] = s1, o[1] = s2, o[2] = mx, o[3] = sn;
#pragma unroll
        for (int t = 0; t < ST_MAXT; ++t) o[4 + t] = cnt[t];
    }
}

// one block: thread q < 4 + T owns quantity q and walks the blocks' partials in block order (nblk == 0: the empty set's values)
__global__ __launch_bounds__(64) void st_final_kernel(const double* __restrict__ part, int nblk, int T, double* __restrict__ out) {
    const int q = threadIdx.x;
    if (q >= 4 + T) return;
    double acc = 0.0;
    for (int k = 0; k < nblk; ++k) {
        const double x = part[(int64_t)ST_ROW * k + q];
        acc = q == 2 ? fmax(acc, x) : acc + x;
    }
    out[q] = acc;
}

}  // namespace

extern "C" int primx_nearest_points(const float* a, int64_t n, const float* b, int m, float* dist, int* idx, void* stream) {
    const char* name = "primx_nearest_points";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX * THREADS, "%s: n out of range", name);
    PRIMX_REQUIRE(m >= 1 && m <= INT32_MAX / 3, "%s: m must lie in 1 .. (2^31 - 1) / 3 (got %d)", name, m);
    PRIMX_REQUIRE(b, "%s: null pointer", name);
    if (n == 0) return PRIMX_OK;
    PRIMX_REQUIRE(a && dist && idx, "%s: null pointer", name);
    if (n >= NN_WIDE)
        hipLaunchKernelGGL(nn_kernel<4>, dim3(nblocks(n, THREADS * 4)), dim3(THREADS), 0, st, a, n, b, m, dist, idx);
    else
        hipLaunchKernelGGL(nn_kernel<1>, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, a, n, b, m, dist, idx);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}

extern "C" int primx_distance_stats(const float* dist, const int* idx, const float* na, const float* nb, int64_t n,
                                    const float* tau, int T, void* ws, int64_t ws_bytes, double* out, void* stream) {
    const char* name = "primx_distance_stats";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)1 << 53, "%s: n out of range", name);
    PRIMX_REQUIRE(T >= 0 && T <= ST_MAXT, "%s: T must lie in 0 .. %d (got %d)", name, ST_MAXT, T);
    PRIMX_REQUIRE(T == 0 || tau, "%s: null threshold pointer with T = %d", name, T);
    PRIMX_REQUIRE(out && (n == 0 || dist), "%s: null pointer", name);
    const bool normals = na != nullptr && nb != nullptr;
    PRIMX_REQUIRE(!normals || n == 0 || idx, "%s: normals need idx", name);
    PRIMX_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= (int64_t)ST_MAXB * ST_ROW * 8,
                  "%s: the workspace needs %d bytes, 8-byte aligned", name, ST_MAXB * ST_ROW * 8);
    Taus t;
    for (int k = 0; k < ST_MAXT; ++k) t.v[k] = k < T ? tau[k] : 0.0f;
    int64_t per = (n + ST_MAXB - 1) / ST_MAXB;
    if (per < ST_PER_BLOCK) per = ST_PER_BLOCK;
    const int nblk = (int)((n + per - 1) / per);
    double* part = (double*)ws;
    if (nblk > 0) {
        hipLaunchKernelGGL(st_part_kernel, dim3(nblk), dim3(THREADS), 0, st, dist, idx, normals ? na : nullptr,
                           normals ? nb : nullptr, n, per, t, T, part);
        PRIMX_CHECK_LAUNCH(name);
    }
    hipLaunchKernelGGL(st_final_kernel, dim3(1), dim3(64), 0, st, (const double*)part, nblk, T, out);
    PRIMX_CHECK_LAUNCH(name);
    return PRIMX_OK;
}
