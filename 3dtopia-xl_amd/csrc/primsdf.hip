// PrimSDF field query: the O(points x primitives) evaluation behind mesh / texture extraction
// (models/primsdf.py:52-109, driven by inference.py:106-116 over 256^3 points and 180-193 over the visible texels).
//
//   w_i(x)   = relu(1 - ||(x - pos_i) / scale_i||_inf)                        (prim_weight, primsdf.py:103-107)
//              = relu(1 - max_d |x_d - pos_d| / |scale_i|): a negative scale weighs as |scale| and samples at the signed
//              (x - pos) / scale; a zero scale covers nothing here (the reference's weight is relu(1 - inf) = 0 there,
//              except NaN at x == pos exactly)
//   out(x)   = sum_i [w_i / (sum_j w_j + 1e-6)] * trilinear(feat_i, (x - pos_i) / scale_i)   (grid_sample_feat, 66-76;
//              grid_sample 'bilinear', align_corners=True: x -> W (fastest), y -> H, z -> D of the [6, S, S, S] volume)
//   eval mode, points no primitive covers: nearest primitive by ||x - pos||_2, nearest of its S^3 grid points,
//              sdf = s + dist * sign(s) with s the stored SDF there; the other channels stay 0               (78-100)
//   preds: sdf = out[0], tex = clip(out[1:4], 0, 1), mat = clip(out[4:6], 0, 1)                          (forward, 52-64)
//
// One thread per point, primitives (scale, pos) streamed through LDS in chunks; the feature volumes (P x 6 x S^3 fp32,
// 25 MB at P = 2048, S = 8) stay in L2 / MALL and only the handful of covering primitives of a point are sampled.
// max_d fl(|x_d - pos_d| / s) == fl(max_d |x_d - pos_d| / s) (rounding is monotonic), so the cull needs no division and
// the weight one division per covering primitive - identical values to the reference's per-axis divisions.
#include "common.h"

namespace {

constexpr int CHUNK = 1024;   // primitives per LDS chunk (16 KB)

// GRAD: also the gradient of channel 0 with respect to the point (primx_primsdf_query_grad; rules in include/primx_hip.h).  The
// forward's statements are shared, so out has the same bits in both instantiations; the gradient adds six register sums
// (ga = sum_k [sigma_k grad w_k + w_k grad sigma_k], gw = sum_k grad w_k) and the chosen grid point's offset on the fill path.
template <bool GRAD>
__global__ __launch_bounds__(256) void primsdf_query_kernel(const float* __restrict__ pts, const float* __restrict__ srt,
                                                           const float* __restrict__ feat, const float* __restrict__ lin,
                                                           float* __restrict__ out, float* __restrict__ grad, int n, int P,
                                                           int S, int C, int eval_fill) {
    __shared__ float4 prim[CHUNK];   // (scale, x, y, z)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) { x = pts[3 * (int64_t)i]; y = pts[3 * (int64_t)i + 1]; z = pts[3 * (int64_t)i + 2]; }
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float wsum = 0.f, best = 3.4e38f;
    int best_i = 0;
    float ga[3] = {0.f, 0.f, 0.f}, gw[3] = {0.f, 0.f, 0.f};
    const int S3 = S * S * S;
    const float half = 0.5f * (float)(S - 1);
    for (int p0 = 0; p0 < P; p0 += CHUNK) {
        const int cnt = min(CHUNK, P - p0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += blockDim.x) prim[t] = reinterpret_cast<const float4*>(srt)[p0 + t];
        __syncthreads();
        if (!live) continue;
        for (int t = 0; t < cnt; ++t) {
            const float4 q = prim[t];
            const float dx = x - q.y, dy = y - q.z, dz = z - q.w;
            if (eval_fill) {
                const float d2 = dx * dx + dy * dy + dz * dz;   // argmin of the L2 distance (first minimum wins)
                if (d2 < best) { best = d2; best_i = p0 + t; }
            }
            const float m = fmaxf(fabsf(dx), fmaxf(fabsf(dy), fabsf(dz)));
            const float as = fabsf(q.x);                       // ||(x - pos) / s||_inf = m / |s|: a negative scale covers
            if (!(m < as)) continue;                           // w = relu(1 - m / |s|) = 0; s = 0 covers nothing
            const float w = 1.0f - m / as;
            if (!(w > 0.f)) continue;
            wsum += w;
            // grid_sample, align_corners=True: index = (coord + 1) / 2 * (S - 1)
            const float fx = (dx / q.x + 1.0f) * half, fy = (dy / q.x + 1.0f) * half, fz = (dz / q.x + 1.0f) * half;
            int ix = min((int)floorf(fx), S - 2), iy = min((int)floorf(fy), S - 2), iz = min((int)floorf(fz), S - 2);
            ix = max(ix, 0); iy = max(iy, 0); iz = max(iz, 0);
            const float tx = fx - (float)ix, ty = fy - (float)iy, tz = fz - (float)iz;
            const float* vol = feat + (int64_t)(p0 + t) * C * S3 + (iz * S + iy) * S + ix;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (c >= C) break;
                const float* v = vol + c * S3;
                const float c00 = v[0] * (1.f - tx) + v[1] * tx;
                const float c01 = v[S] * (1.f - tx) + v[S + 1] * tx;
                const float c10 = v[S * S] * (1.f - tx) + v[S * S + 1] * tx;
                const float c11 = v[S * S + S] * (1.f - tx) + v[S * S + S + 1] * tx;
                const float s = (c00 * (1.f - ty) + c01 * ty) * (1.f - tz) + (c10 * (1.f - ty) + c11 * ty) * tz;
                acc[c] += w * s;
            }
            if constexpr (GRAD) {
                // channel 0 again, with its three cell-local derivatives (the backward's expressions)
                const float ux = 1.f - tx, uy = 1.f - ty, uz = 1.f - tz;
                const float v000 = vol[0], v001 = vol[1], v010 = vol[S], v011 = vol[S + 1];
                const float v100 = vol[S * S], v101 = vol[S * S + 1], v110 = vol[S * S + S], v111 = vol[S * S + S + 1];
                const float c00 = v000 * ux + v001 * tx, c01 = v010 * ux + v011 * tx;
                const float c10 = v100 * ux + v101 * tx, c11 = v110 * ux + v111 * tx;
                const float c0 = c00 * uy + c01 * ty, c1 = c10 * uy + c11 * ty;
                const float sig = c0 * uz + c1 * tz;
                const float hs = w * (half / q.x);                              // w_k (S - 1) / (2 s_k)
                ga[0] += hs * (((v001 - v000) * uy + (v011 - v010) * ty) * uz + ((v101 - v100) * uy + (v111 - v110) * ty) * tz);
                ga[1] += hs * ((c01 - c00) * uz + (c11 - c10) * tz);
                ga[2] += hs * (c1 - c0);
                const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
                const int j = (ax >= ay && ax >= az) ? 0 : ((ay >= az) ? 1 : 2);   // first of equals, x, y, z order
                const float dj = j == 0 ? dx : (j == 1 ? dy : dz);
                const float wj = (dj < 0.f ? 1.f : (dj > 0.f ? -1.f : 0.f)) / as;   // grad w_k = -sign(d_j) / |s| e_j
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    gw[a] += a == j ? wj : 0.f;
                    ga[a] += a == j ? sig * wj : 0.f;
                }
            }
        }
    }
    if (!live) return;
    float r[6];
    const float inv = 1.0f / (wsum + 1e-6f);
#pragma unroll
    for (int c = 0; c < 6; ++c) r[c] = acc[c] * inv;
    if (eval_fill && !(wsum > 0.f)) {
        const float4 q = reinterpret_cast<const float4*>(srt)[best_i];
        // nearest grid point of the nearest primitive: the distance is separable, so per axis
        const float px[3] = {x, y, z}, pc[3] = {q.y, q.z, q.w};
        int idx[3];
        float d2 = 0.f;
        float off[3] = {0.f, 0.f, 0.f};                                         // x - g per axis (GRAD)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            int bi = 0;
            float bd = 3.4e38f;
            for (int k = 0; k < S; ++k) {
                const float e = px[a] - (pc[a] + q.x * lin[k]);
                if (e * e < bd) {
                    bd = e * e;
                    bi = k;
                    if constexpr (GRAD) off[a] = e;
                }
            }
            idx[a] = bi;
            d2 += bd;
        }
        const float s = feat[(int64_t)best_i * C * S3 + (idx[2] * S + idx[1]) * S + idx[0]];   // channel 0, [z][y][x]
        const float sgn = (s > 0.f) ? 1.f : ((s < 0.f) ? -1.f : 0.f);
        r[0] = s + sqrtf(d2) * sgn;
        if constexpr (GRAD) {
            const float dist = sqrtf(d2);
            const float k = dist > 0.f ? sgn / dist : 0.f;                      // sign(s) (x - g) / dist; 0 at dist == 0 or s == 0
            gw[0] = gw[1] = gw[2] = 0.f;
            ga[0] = k * off[0]; ga[1] = k * off[1]; ga[2] = k * off[2];
        }
    }
    if constexpr (GRAD) {
        // covered: (ga - o gw) / (W + 1e-6); uncovered: the fill's gradient as it stands (inv multiplies 0 sums without the fill)
        const bool filled = eval_fill && !(wsum > 0.f);
        float* go = grad + 3 * (int64_t)i;
#pragma unroll
        for (int a = 0; a < 3; ++a) go[a] = filled ? ga[a] : (ga[a] - r[0] * gw[a]) * inv;
    }
    float* o = out + (int64_t)i * C;
    o[0] = r[0];
#pragma unroll
    for (int c = 1; c < 6; ++c)
        if (c < C) o[c] = fminf(fmaxf(r[c], 0.f), 1.f);
}

}  // namespace

extern "C" int primx_primsdf_query(const float* pts, const float* srt, const float* feat, const float* lin, float* out,
                                   int n, int P, int S, int C, int eval_fill, void* stream) {
    PRIMX_REQUIRE(pts && srt && feat && lin && out, "primx_primsdf_query: null pointer");
    PRIMX_REQUIRE(n > 0 && P > 0 && S >= 2 && S <= 32 && C >= 1 && C <= 6, "primx_primsdf_query: need n, P > 0, 2 <= S <= 32, 1 <= C <= 6");
    hipLaunchKernelGGL(primsdf_query_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, pts, srt, feat,
                       lin, out, (float*)nullptr, n, P, S, C, eval_fill);
    PRIMX_CHECK_LAUNCH("primx_primsdf_query");
    return PRIMX_OK;
}

extern "C" int primx_primsdf_query_grad(const float* pts, const float* srt, const float* feat, const float* lin, float* out,
                                        float* grad, int n, int P, int S, int C, int eval_fill, void* stream) {
    PRIMX_REQUIRE(pts && srt && feat && lin && out && grad, "primx_primsdf_query_grad: null pointer");
    PRIMX_REQUIRE(n > 0 && P > 0 && S >= 2 && S <= 32 && C >= 1 && C <= 6, "primx_primsdf_query_grad: need n, P > 0, 2 <= S <= 32, 1 <= C <= 6");
    hipLaunchKernelGGL(primsdf_query_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, pts, srt, feat,
                       lin, out, grad, n, P, S, C, eval_fill);
    PRIMX_CHECK_LAUNCH("primx_primsdf_query_grad");
    return PRIMX_OK;
}

// ---------------------------------------------------------------------------------------------
// Backward of the training-mode query (ABI 34; rules in include/primx_hip.h next to the forward's).  One thread per point,
// primitives streamed through LDS as in the forward, in two sweeps over the covering primitives of the point:
//   sweep 1: sum_k w_k and o_c = inv * sum_k w_k sigma_kc with the forward's own cull, weight and cell expressions, then the
//            clip mask on gout (channel 0 passes; c >= 1 passes where 0 <= o_c <= 1);
//   sweep 2: per covering primitive the 8 corner weights, sigma_kc and its three cell-local derivatives; 8 * C adds into
//            gfeat and 4 into gsrt (the weight path and the sample path summed in registers first).
// The adds are global fp32 atomicAdd (one vector global_atomic_add_f32 each, no compare-and-swap loop): sums depend on the
// arrival order, so the results are NOT bitwise reproducible from run to run.  A point no primitive covers, or whose masked
// gout is all zero, adds nothing.
namespace {

__global__ __launch_bounds__(256) void primsdf_query_backward_kernel(const float* __restrict__ pts, const float* __restrict__ srt,
                                                                    const float* __restrict__ feat,
                                                                    const float* __restrict__ gout, float* __restrict__ gsrt,
                                                                    float* __restrict__ gfeat, int n, int P, int S, int C) {
    __shared__ float4 prim[CHUNK];   // (scale, x, y, z)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool live = i < n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) { x = pts[3 * (int64_t)i]; y = pts[3 * (int64_t)i + 1]; z = pts[3 * (int64_t)i + 2]; }
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // sweep 1: sum_k w_k sigma_kc; then o_c
    float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // the masked gout
    float wsum = 0.f, inv = 0.f;
    const int S3 = S * S * S;
    const float half = 0.5f * (float)(S - 1);
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int p0 = 0; p0 < P; p0 += CHUNK) {
            const int cnt = min(CHUNK, P - p0);
            __syncthreads();
            for (int t = threadIdx.x; t < cnt; t += blockDim.x) prim[t] = reinterpret_cast<const float4*>(srt)[p0 + t];
            __syncthreads();
            if (!live) continue;
            for (int t = 0; t < cnt; ++t) {
                const float4 q = prim[t];
                const float dx = x - q.y, dy = y - q.z, dz = z - q.w;
                const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
                const float m = fmaxf(ax, fmaxf(ay, az));
                const float as = fabsf(q.x);
                if (!(m < as)) continue;                        // the forward's cull ...
                const float w = 1.0f - m / as;
                if (!(w > 0.f)) continue;                       // ... and its weight test
                const float fx = (dx / q.x + 1.0f) * half, fy = (dy / q.x + 1.0f) * half, fz = (dz / q.x + 1.0f) * half;
                int ix = min((int)floorf(fx), S - 2), iy = min((int)floorf(fy), S - 2), iz = min((int)floorf(fz), S - 2);
                ix = max(ix, 0); iy = max(iy, 0); iz = max(iz, 0);
                const float tx = fx - (float)ix, ty = fy - (float)iy, tz = fz - (float)iz;
                const int64_t base = (int64_t)(p0 + t) * C * S3 + (iz * S + iy) * S + ix;
                const float* vol = feat + base;
                if (sweep == 0) {
                    wsum += w;
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        if (c >= C) break;
                        const float* v = vol + c * S3;
                        const float c00 = v[0] * (1.f - tx) + v[1] * tx;
                        const float c01 = v[S] * (1.f - tx) + v[S + 1] * tx;
                        const float c10 = v[S * S] * (1.f - tx) + v[S * S + 1] * tx;
                        const float c11 = v[S * S + S] * (1.f - tx) + v[S * S + S + 1] * tx;
                        const float s = (c00 * (1.f - ty) + c01 * ty) * (1.f - tz) + (c10 * (1.f - ty) + c11 * ty) * tz;
                        acc[c] += w * s;
                    }
                    continue;
                }
                // sweep 2: the scatter
                const float wi = w * inv;
                const float ux = 1.f - tx, uy = 1.f - ty, uz = 1.f - tz;
                float a = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
                for (int c = 0; c < 6; ++c) {
                    if (c >= C) break;
                    const float gc = g[c];
                    if (gc == 0.f) continue;
                    const float* v = vol + c * S3;
                    const float v000 = v[0], v001 = v[1], v010 = v[S], v011 = v[S + 1];
                    const float v100 = v[S * S], v101 = v[S * S + 1], v110 = v[S * S + S], v111 = v[S * S + S + 1];
                    const float c00 = v000 * ux + v001 * tx, c01 = v010 * ux + v011 * tx;
                    const float c10 = v100 * ux + v101 * tx, c11 = v110 * ux + v111 * tx;
                    const float c0 = c00 * uy + c01 * ty, c1 = c10 * uy + c11 * ty;
                    const float s = c0 * uz + c1 * tz;
                    a += gc * (s - acc[c]);
                    bx += gc * (((v001 - v000) * uy + (v011 - v010) * ty) * uz + ((v101 - v100) * uy + (v111 - v110) * ty) * tz);
                    by += gc * ((c01 - c00) * uz + (c11 - c10) * tz);
                    bz += gc * (c1 - c0);
                    if (gfeat) {
                        float* gv = gfeat + base + c * S3;
                        const float k = gc * wi;
                        atomicAdd(gv, k * (ux * uy * uz));
                        atomicAdd(gv + 1, k * (tx * uy * uz));
                        atomicAdd(gv + S, k * (ux * ty * uz));
                        atomicAdd(gv + S + 1, k * (tx * ty * uz));
                        atomicAdd(gv + S * S, k * (ux * uy * tz));
                        atomicAdd(gv + S * S + 1, k * (tx * uy * tz));
                        atomicAdd(gv + S * S + S, k * (ux * ty * tz));
                        atomicAdd(gv + S * S + S + 1, k * (tx * ty * tz));
                    }
                }
                if (gsrt) {
                    a *= inv;                                                   // dL/dw_k
                    const float bs = wi * half;
                    bx *= bs; by *= bs; bz *= bs;                               // dL/df_a
                    const int j = (ax >= ay && ax >= az) ? 0 : ((ay >= az) ? 1 : 2);   // first of equals, x, y, z order
                    const float dj = j == 0 ? dx : (j == 1 ? dy : dz);
                    const float sg = a * (dj < 0.f ? -1.f : (dj > 0.f ? 1.f : 0.f)) / as;   // a_k sign(d_j) / |s|
                    const float is = 1.0f / q.x, is2 = is * is;
                    float* gs = gsrt + 4 * (int64_t)(p0 + t);
                    atomicAdd(gs, a * m * (q.x < 0.f ? -1.f : 1.f) * is2 - (bx * dx + by * dy + bz * dz) * is2);
                    atomicAdd(gs + 1, -bx * is + (j == 0 ? sg : 0.f));
                    atomicAdd(gs + 2, -by * is + (j == 1 ? sg : 0.f));
                    atomicAdd(gs + 3, -bz * is + (j == 2 ? sg : 0.f));
                }
            }
        }
        if (sweep == 0 && live) {
            live = wsum > 0.f;
            inv = 1.0f / (wsum + 1e-6f);
            bool any = false;
            const float* go = gout + (int64_t)i * C;
#pragma unroll
            for (int c = 0; c < 6; ++c) {
                if (c >= C) break;
                acc[c] *= inv;                                                  // o_c
                g[c] = (c == 0 || (acc[c] >= 0.f && acc[c] <= 1.f)) ? go[c] : 0.f;
                any = any || g[c] != 0.f;
            }
            live = live && any;
        }
    }
}

}  // namespace

extern "C" int primx_primsdf_query_backward(const float* pts, const float* srt, const float* feat, const float* gout,
                                            float* gsrt, float* gfeat, int n, int P, int S, int C, void* stream) {
    PRIMX_REQUIRE(pts && srt && feat && gout, "primx_primsdf_query_backward: null pointer");
    PRIMX_REQUIRE(gsrt || gfeat, "primx_primsdf_query_backward: gsrt and gfeat are both null");
    PRIMX_REQUIRE(n > 0 && P > 0 && S >= 2 && S <= 32 && C >= 1 && C <= 6,
                  "primx_primsdf_query_backward: need n, P > 0, 2 <= S <= 32, 1 <= C <= 6");
    hipLaunchKernelGGL(primsdf_query_backward_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, pts, srt, feat,
                       gout, gsrt, gfeat, n, P, S, C);
    PRIMX_CHECK_LAUNCH("primx_primsdf_query_backward");
    return PRIMX_OK;
}
