// Textured meshes: the glTF metallic-roughness material of a mesh evaluated at the closest surface point of every
// query point.  Rules and the C ABI: include/primx_hip.h "Textured meshes"; float64 / float32 restatement:
// tests/material_numpy.py.
//
// The closest-point search is primx_mesh_field_query's (csrc/meshfield.hip): fit.MeshField hands it [vt | color | rm] as the
// per-vertex attributes and gets back, per point, the interpolated UV, vertex colour, roughness / metallic multipliers and the
// face.  primx_material_sample turns those into (r, g, b, roughness, metallic):
//
//   check:   one thread per entry of face_material, of the material table and of the texture table flags what lies outside its
//            range (the index-flag pattern of mf_prep_kernel).
//   sample:  one thread per point (64-bit point index), no atomics.  A thread follows face -> material -> texture -> descriptor
//            and verifies every link itself before it dereferences the next, so nothing is read out of bounds whatever the
//            tables hold; a broken link sets the flag and the point's output is 0.
//
// The host reads the flag back once, after both launches, and returns PRIMX_EINVAL if it is set.  Every floating-point expression
// is evaluated as written (no contraction) and the division by 255 is correctly rounded, so the output equals the float32
// restatement bit for bit.
#include <cmath>
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace {

#include "mesh_common.h"

constexpr int MAX_EXTENT = 65536;        // W and H at most: 2 W fits an int with room, float(W) is exact
constexpr float X_LIMIT = 1073741824.0f; // |texel coordinate| is clamped to 2^30 before it becomes an int

struct Tex {
    int64_t off;
    int W, H, flags;
};

// desc row: texel offset, W, H, flags (bits 0-1 wrapS, bits 2-3 wrapT: 0 clamp, 1 repeat, 2 mirrored repeat; bit 4 nearest)
__device__ __forceinline__ bool load_tex(const int64_t* __restrict__ desc, int t, int64_t n_texels, Tex& o) {
    const int64_t off = desc[(int64_t)4 * t], W = desc[(int64_t)4 * t + 1], H = desc[(int64_t)4 * t + 2],
                  fl = desc[(int64_t)4 * t + 3];
    if (W < 1 || W > MAX_EXTENT || H < 1 || H > MAX_EXTENT || off < 0 || off > n_texels || W * H > n_texels - off) return false;
    if (fl < 0 || fl > 31 || (fl & 3) == 3 || ((fl >> 2) & 3) == 3) return false;
    o.off = off, o.W = (int)W, o.H = (int)H, o.flags = (int)fl;
    return true;
}

__device__ __forceinline__ int wrap(int i, int n, int mode) {
    if (mode == 0) return min(max(i, 0), n - 1);
    const int period = mode == 1 ? n : 2 * n;
    int t = i % period;
    if (t < 0) t += period;
    if (mode == 1) return t;
    return t < n ? t : 2 * n - 1 - t;
}

__device__ __forceinline__ float finite_or_zero(float x) { return fabsf(x) <= 3.4028234663852886e38f ? x : 0.0f; }   // NaN compares false

__device__ __forceinline__ float clamp_x(float x) { return fminf(fmaxf(x, -X_LIMIT), X_LIMIT); }

__device__ __forceinline__ void texel(const uint8_t* __restrict__ texels, const Tex& t, int i, int j, float* c) {
    const uchar4 b = *reinterpret_cast<const uchar4*>(texels + 4 * (t.off + (int64_t)j * t.W + i));
    c[0] = (float)b.x / 255.0f, c[1] = (float)b.y / 255.0f, c[2] = (float)b.z / 255.0f;
}

// the r, g, b of texture t at (u, v)
__device__ __forceinline__ void sample(const uint8_t* __restrict__ texels, const Tex& t, float u, float v, float* c) {
    const int ws = t.flags & 3, wt = (t.flags >> 2) & 3;
    const float W = (float)t.W, H = (float)t.H;
    if (t.flags & 16) {
        const int i = (int)clamp_x(floorf(u * W)), j = (int)clamp_x(floorf(v * H));
        texel(texels, t, wrap(i, t.W, ws), wrap(j, t.H, wt), c);
        return;
    }
    const float x = clamp_x(u * W - 0.5f), y = clamp_x(v * H - 0.5f);
    const float xf = floorf(x), yf = floorf(y);
    const float fx = x - xf, fy = y - yf;
    const int i0 = (int)xf, j0 = (int)yf;
    const int ia = wrap(i0, t.W, ws), ib = wrap(i0 + 1, t.W, ws), ja = wrap(j0, t.H, wt), jb = wrap(j0 + 1, t.H, wt);
    float t00[3], t10[3], t01[3], t11[3];
    texel(texels, t, ia, ja, t00), texel(texels, t, ib, ja, t10), texel(texels, t, ia, jb, t01), texel(texels, t, ib, jb, t11);
    const float gx = 1.0f - fx, gy = 1.0f - fy;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (t00[k] * gx + t10[k] * fx) * gy + (t01[k] * gx + t11[k] * fx) * fy;
}

__global__ __launch_bounds__(THREADS) void mat_check_kernel(const int* __restrict__ face_material, int F,
                                                            const int* __restrict__ mat_tex, int M,
                                                            const int64_t* __restrict__ desc, int T, int64_t n_texels,
                                                            int* __restrict__ status) {
    const int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (t < F) {
        const int m = face_material[t];
        if (m < 0 || m >= M) atomicOr(status, 2);
    } else if (t < (int64_t)F + M) {
        const int64_t m = t - F;
        const int a = mat_tex[2 * m], b = mat_tex[2 * m + 1];
        if (a < -1 || a >= T || b < -1 || b >= T) atomicOr(status, 4);
    } else if (t < (int64_t)F + M + T) {
        Tex d;
        if (!load_tex(desc, (int)(t - F - M), n_texels, d)) atomicOr(status, 8);
    }
}

__global__ __launch_bounds__(THREADS) void mat_sample_kernel(const float* __restrict__ uv, const float* __restrict__ vattr,
                                                             const int* __restrict__ face, int64_t n,
                                                             const int* __restrict__ face_material, int F,
                                                             const float* __restrict__ mat_factor,
                                                             const int* __restrict__ mat_tex, int M,
                                                             const int64_t* __restrict__ desc, int T,
                                                             const uint8_t* __restrict__ texels, int64_t n_texels,
                                                             int* __restrict__ status, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    float* o = out + 5 * i;
    o[0] = 0.0f, o[1] = 0.0f, o[2] = 0.0f, o[3] = 0.0f, o[4] = 0.0f;
    const int fc = face[i];
    if (fc < 0 || fc >= F) {
        atomicOr(status, 1);
        return;
    }
    const int m = face_material[fc];
    if (m < 0 || m >= M) {
        atomicOr(status, 2);
        return;
    }
    const int tb = mat_tex[2 * m], tm = mat_tex[2 * m + 1];
    if (tb < -1 || tb >= T || tm < -1 || tm >= T) {
        atomicOr(status, 4);
        return;
    }
    const float u = finite_or_zero(uv[2 * i]), v = finite_or_zero(uv[2 * i + 1]);
    float base[3] = {1.0f, 1.0f, 1.0f}, mr[3] = {1.0f, 1.0f, 1.0f};
    Tex d;
    if (tb >= 0) {
        if (!load_tex(desc, tb, n_texels, d)) {
            atomicOr(status, 8);
            return;
        }
        sample(texels, d, u, v, base);
    }
    if (tm >= 0) {
        if (!load_tex(desc, tm, n_texels, d)) {
            atomicOr(status, 8);
            return;
        }
        sample(texels, d, u, v, mr);
    }
    float a[6] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
    if (vattr) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a[k] = vattr[6 * i + k];
    }
    const float* fa = mat_factor + 6 * (int64_t)m;
    o[0] = (fa[0] * a[0]) * base[0];
    o[1] = (fa[1] * a[1]) * base[1];
    o[2] = (fa[2] * a[2]) * base[2];
    o[3] = (fa[4] * a[4]) * mr[1];
    o[4] = (fa[5] * a[5]) * mr[2];
}

}  // namespace

extern "C" int primx_material_sample(const float* uv, const float* vattr, const int* face, int64_t n, const int* face_material,
                                     int F, const float* mat_factor, const int* mat_tex, int M, const int64_t* tex_desc, int T,
                                     const uint8_t* texels, int64_t n_texels, int* status, float* out, void* stream) {
    const char* name = "primx_material_sample";
    hipStream_t st = (hipStream_t)stream;
    PRIMX_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX * THREADS, "%s: n out of range", name);
    PRIMX_REQUIRE(F >= 1 && M >= 1 && T >= 0, "%s: F and M must be at least 1 and T at least 0 (got %d, %d, %d)", name, F, M, T);
    PRIMX_REQUIRE((int64_t)F + M + T <= INT32_MAX, "%s: F + M + T must stay below 2^31", name);
    PRIMX_REQUIRE(n_texels >= 0 && n_texels <= INT64_MAX / 4, "%s: n_texels out of range", name);
    PRIMX_REQUIRE(face_material && mat_factor && mat_tex && status, "%s: null pointer", name);
    PRIMX_REQUIRE(T == 0 || tex_desc, "%s: null texture table with T = %d", name, T);
    PRIMX_REQUIRE(n_texels == 0 || (texels && ((uintptr_t)texels & 3) == 0), "%s: the texel blob must be 4-byte aligned", name);
    PRIMX_REQUIRE(n == 0 || (uv && face && out), "%s: null pointer", name);
    PRIMX_TRY(zero(status, sizeof(int), st, name));
    hipLaunchKernelGGL(mat_check_kernel, dim3(nblocks((int64_t)F + M + T, THREADS)), dim3(THREADS), 0, st, face_material, F, mat_tex,
                       M, tex_desc, T, n_texels, status);
    PRIMX_CHECK_LAUNCH(name);
    if (n > 0) {
        hipLaunchKernelGGL(mat_sample_kernel, dim3(nblocks(n, THREADS)), dim3(THREADS), 0, st, uv, vattr, face, n, face_material, F,
                           mat_factor, mat_tex, M, tex_desc, T, texels, n_texels, status, out);
        PRIMX_CHECK_LAUNCH(name);
    }
    int flag = 0;
    PRIMX_TRY(readback(&flag, status, sizeof(flag), st, name));
    PRIMX_REQUIRE(!(flag & 1), "%s: a face lies outside [0, F)", name);
    PRIMX_REQUIRE(!(flag & 2), "%s: a material index lies outside [0, M)", name);
    PRIMX_REQUIRE(!(flag & 4), "%s: a texture index lies outside [-1, T)", name);
    PRIMX_REQUIRE(!(flag & 8), "%s: a texture descriptor is malformed or runs past the texel blob", name);
    return PRIMX_OK;
}
