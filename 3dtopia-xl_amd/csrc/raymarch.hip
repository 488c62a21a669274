// Volumetric primitive ray marcher, forward and backward: what RayMarcher.forward computes for the
// previews / turntable of the CLI and the app (dva/ray_marcher.py:142-229 -> compute_raydirs + mvpraymarch with
// algo = 0, chlast template, no warp field, SRT primitive transforms, additive accumulation, "fixedorder" BVH).
//
// Semantics followed (reference CUDA, dva/mvp/extensions/):
//   rays          utils/utils_kernel.cu:15-56     origin = campos / volradius, dir = normalize(R^T-rows * ((pix - princpt) / focal, 1)),
//                                                 [tmin, tmax] = slab test against [-1, 1]^3, tmin clamped to 0
//   hit list      mvpraymarch/utils.h:728-824     fixed-order tree = primitives in INDEX order; a primitive enters the list of
//                                                 every ray of the warp if any ray's local slab test passes (at most 512);
//                                                 each ray keeps the union [rtmin, rtmax] of ITS OWN intersections
//   marching      mvpraymarch_subset_kernel.h:58-86   t starts at tmin + floor((rtmin - tmin) / dt) * dt; per step, per listed
//                                                 primitive in order: y = (R (x - pos)) * scale; if |y| < 1 strictly, not
//                                                 saturated and t < rtmax + 1e-5: sample, accumulate
//   sample        primsampler.h:37-62 + utils.h:406-500   trilinear, align_corners, zero padding, channels-last float4 voxels;
//                                                 alpha *= exp(-fadescale * sum |y_d|^fadeexp)
//   accumulation  primaccum.h:63-78               newalpha = a + alpha * dt; rgba += (rgb, 1) * (min(newalpha, 1) - a); saturate at 1
//
// MI355X design: one wave = one 8 x 8 pixel tile.  There is no tree: the 64 rays of a tile test ALL K primitives (the
// primitive record is wave-uniform, so it comes through scalar loads) and build the tile's hit list in LDS with a ballot
// - 2048 primitives x 270 k rays is ~1 ms of VALU, less than the tree build + traversal it replaces; the list order is the
// index order the reference's "fixedorder" tree produces, so saturation happens at the same sample.
#include <stdio.h>
#include <stdlib.h>

#include "common.h"

namespace {

// PRIMX_RAYMARCH_STATS=1: per-wave counters [waves, sum num, marching waves, chunks, sum nsub, steps, record evaluations]
__device__ unsigned long long g_rm_stats[12];
// ... and of the backward: [taken samples of sweep 2, (step, primitive) wave sums in front of the SRT adds, flushed template entries]
__device__ unsigned long long g_rm_bwd_stats[3];

constexpr int MAXHIT = 512;   // the reference's maxhitboxes
constexpr int CHUNK = 96;     // marching steps per sub-list rebuild
constexpr int NREC = 64;      // primitives per wave and chunk with an LDS record (16 floats) and per-ray entry / exit steps

struct F3 { float x, y, z; };
__device__ __forceinline__ float fast_pow(float x, float y) { return __builtin_amdgcn_exp2f(y * __builtin_amdgcn_logf(x)); }
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ F3 ld3(const float* p) { return {p[0], p[1], p[2]}; }

__global__ __launch_bounds__(256) void raydirs_kernel(const float* __restrict__ viewpos, const float* __restrict__ viewrot,
                                                     const float* __restrict__ focal, const float* __restrict__ princpt,
                                                     const float* __restrict__ pixelcoords, float volradius,
                                                     float* __restrict__ raypos, float* __restrict__ raydir,
                                                     float* __restrict__ tminmax, int N, int H, int W) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)N * H * W) return;
    const int w = (int)(idx % W), h = (int)((idx / W) % H), n = (int)(idx / ((int64_t)W * H));
    const F3 rp = {viewpos[n * 3] / volradius, viewpos[n * 3 + 1] / volradius, viewpos[n * 3 + 2] / volradius};
    float px = (float)w, py = (float)h;
    if (pixelcoords) { px = pixelcoords[idx * 2]; py = pixelcoords[idx * 2 + 1]; }
    px = (px - princpt[n * 2]) / focal[n * 2];
    py = (py - princpt[n * 2 + 1]) / focal[n * 2 + 1];
    const float* R = viewrot + n * 9;
    F3 d = {R[0] * px + R[3] * py + R[6], R[1] * px + R[4] * py + R[7], R[2] * px + R[5] * py + R[8]};
    const float inv = rsqrtf(d.x * d.x + d.y * d.y + d.z * d.z);     // helper_math normalize(): v * rsqrtf(dot(v, v))
    d = {d.x * inv, d.y * inv, d.z * inv};
    const float t1x = (-1.f - rp.x) / d.x, t2x = (1.f - rp.x) / d.x;
    const float t1y = (-1.f - rp.y) / d.y, t2y = (1.f - rp.y) / d.y;
    const float t1z = (-1.f - rp.z) / d.z, t2z = (1.f - rp.z) / d.z;
    const float tmin = fmaxf(fminf(t1x, t2x), fmaxf(fminf(t1y, t2y), fminf(t1z, t2z)));
    const float tmax = fminf(fmaxf(t1x, t2x), fminf(fmaxf(t1y, t2y), fmaxf(t1z, t2z)));
    raypos[idx * 3] = rp.x; raypos[idx * 3 + 1] = rp.y; raypos[idx * 3 + 2] = rp.z;
    raydir[idx * 3] = d.x; raydir[idx * 3 + 1] = d.y; raydir[idx * 3 + 2] = d.z;
    tminmax[idx * 2] = fmaxf(tmin, 0.f);
    tminmax[idx * 2 + 1] = tmax;
}

// ---- the march, shared by the forward and the backward kernel -----------------------------------------------------------
// One copy of everything that decides WHICH samples a ray takes: the tile's hit list, the chunk rebuild, the per-ray step
// windows, the LDS record cache, the stepping of t and rp, the strict inside test and t < rtmax + 1e-5.  A kernel declares
// the LDS arrays (MarchLds), loads its ray (load_ray), builds the list once (tile_hit_list) and runs march_sweep with a
// visitor: `bool done()` is the lane's "saturated" flag, `sample(take, k, loc)` is called for every evaluated (step, listed
// primitive) in wave-uniform control flow, with take = this lane takes the sample.
struct Prims { const float* ppos; const float* prot; const float* pscl; };
struct Ray { F3 rp, rd; float tmin0, tmax0, rtmin, rtmax; int num; };
struct Local { F3 xm; float pr[9]; F3 s; float yx, yy, yz; };   // xm = x - pos, pr = the stored 3 x 3, s = scale, y = local position
struct MarchLds {
    int hits[4][MAXHIT];
    int subs[4][MAXHIT];
    float4 recs[4][NREC][4];   // (pos.xyz, r00) (r01 r02 r10 r11) (r12 r20 r21 r22) (scale.xyz, -)
    unsigned short span[4][NREC][64];   // per ray: first | last << 8 step of the chunk the ray can be inside
};
struct MarchStats { unsigned long long chunks = 0, nsub = 0, steps = 0, eval = 0, c_rebuild = 0; };

// block = 4 waves = 16 x 16 pixels, each wave an 8 x 8 tile with its own hit list
struct TileId { int lane, wave, n; bool valid; int64_t pix; };
__device__ __forceinline__ TileId tile_id(int H, int W) {
    TileId t;
    t.lane = threadIdx.x & 63;
    t.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    t.n = blockIdx.z;
    const int w = blockIdx.x * 16 + (t.wave & 1) * 8 + (t.lane & 7);
    const int h = blockIdx.y * 16 + (t.wave >> 1) * 8 + (t.lane >> 3);
    t.valid = w < W && h < H;
    t.pix = ((int64_t)t.n * H + min(h, H - 1)) * W + min(w, W - 1);   // out-of-image lanes shadow an edge ray
    return t;
}

// ---- hit list of the tile (index order) + this ray's own [rtmin, rtmax]
__device__ __forceinline__ void tile_hit_list(const Prims& P, int K, int lane, int* list, Ray& ray) {
    const float* ppos = P.ppos; const float* prot = P.prot; const float* pscl = P.pscl;
    const F3 rp = ray.rp, rd = ray.rd;
    int num = 0;
    float rtmin = INFINITY, rtmax = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const float* pr = prot + k * 9;
        const F3 xm = {rp.x - ppos[k * 3], rp.y - ppos[k * 3 + 1], rp.z - ppos[k * 3 + 2]};
        // PrimTransfSRT::forward2: r = (pr0 x + pr1 y + pr2 z) * scale   (pr_i = i-th row of the stored 3 x 3)
        const float sx = pscl[k * 3], sy = pscl[k * 3 + 1], sz = pscl[k * 3 + 2];
        const F3 r0 = {(pr[0] * xm.x + pr[3] * xm.y + pr[6] * xm.z) * sx, (pr[1] * xm.x + pr[4] * xm.y + pr[7] * xm.z) * sy,
                       (pr[2] * xm.x + pr[5] * xm.y + pr[8] * xm.z) * sz};
        const F3 r1 = {(pr[0] * rd.x + pr[3] * rd.y + pr[6] * rd.z) * sx, (pr[1] * rd.x + pr[4] * rd.y + pr[7] * rd.z) * sy,
                       (pr[2] * rd.x + pr[5] * rd.y + pr[8] * rd.z) * sz};
        const float ix = 1.0f / r1.x, iy = 1.0f / r1.y, iz = 1.0f / r1.z;
        const float ax = (-1.f - r0.x) * ix, bx = (1.f - r0.x) * ix;
        const float ay = (-1.f - r0.y) * iy, by = (1.f - r0.y) * iy;
        const float az = (-1.f - r0.z) * iz, bz = (1.f - r0.z) * iz;
        const float trmin = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
        const float trmax = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
        const bool hit = trmin <= trmax;
        if (hit) { rtmin = fminf(rtmin, trmin); rtmax = fmaxf(rtmax, trmax); }
        if (__any(hit) && num < MAXHIT) {       // wave-uniform
            if (lane == 0) list[num] = k;
            ++num;
        }
    }
    ray.rtmin = fmaxf(rtmin, ray.tmin0);
    ray.rtmax = fminf(rtmax, ray.tmax0);
    ray.num = num;
    __builtin_amdgcn_s_waitcnt(0xC07F);   // the list (written by lane 0) is read by the whole wave below
    __builtin_amdgcn_wave_barrier();
}

template <class Visitor>
__device__ __forceinline__ void march_sweep(const Prims& P, MarchLds& lds, int wave, int lane, const Ray& ray, float stepsize,
                                            Visitor& vis, int stats, MarchStats& st) {
    const float* ppos = P.ppos; const float* prot = P.prot; const float* pscl = P.pscl;
    const int* list = lds.hits[wave];
    int* sub = lds.subs[wave];
    const int num = ray.num;
    const float rtmin = ray.rtmin, rtmax = ray.rtmax;
    const F3 rd = ray.rd;
    F3 rp = ray.rp;
    unsigned long long c_t0 = 0;
    float t = ray.tmin0;
    rp = {rp.x + rd.x * ray.tmin0, rp.y + rd.y * ray.tmin0, rp.z + rd.z * ray.tmin0};
    const int incs = (int)floorf((rtmin - t) / stepsize);
    t += incs * stepsize;
    rp = {rp.x + rd.x * incs * stepsize, rp.y + rd.y * incs * stepsize, rp.z + rd.z * incs * stepsize};
    // The shipped step is 1e-4 of the volume: a ray takes ~10^4 steps while a primitive spans a few hundred of them.
    // Every CHUNK steps the tile's hit list is filtered down to the primitives whose (per-ray) slab interval overlaps the
    // chunk for ANY ray of the wave, with a two-step safety margin; inside the chunk only those are transformed and
    // tested.  The filter is conservative, and a listed primitive the sample is not inside fails `in` exactly as before,
    // so the image is the one the unfiltered loop produces.  The intervals are measured from the sample position rp at
    // the chunk start, not from ro + t rd: t and rp are accumulated separately in fp32 and drift apart by up to ~0.1 % of
    // a step per step (t += 1e-4 in [2, 4) advances 419 ulps instead of 419.43) - tens of steps over a 2 x 10^4-step ray,
    // far beyond the margin - while rp drifts from its own straight line by < 0.05 steps within one chunk.
    while (!__all(t > rtmax + 1e-5f || vis.done())) {
        if (stats) c_t0 = __builtin_readcyclecounter();
        const float c_end = (float)CHUNK * stepsize;     // chunk span, measured from the current sample position
        const bool live = !(t > rtmax + 1e-5f || vis.done());
        int nsub = 0;
        for (int ks = 0; ks < num; ++ks) {
            const int k = __builtin_amdgcn_readfirstlane(list[ks]);   // wave-uniform: the primitive record comes through scalar loads
            const float* pr = prot + k * 9;
            const F3 xm = {rp.x - ppos[k * 3], rp.y - ppos[k * 3 + 1], rp.z - ppos[k * 3 + 2]};
            const float sx = pscl[k * 3], sy = pscl[k * 3 + 1], sz = pscl[k * 3 + 2];
            const F3 r0 = {(pr[0] * xm.x + pr[3] * xm.y + pr[6] * xm.z) * sx, (pr[1] * xm.x + pr[4] * xm.y + pr[7] * xm.z) * sy,
                           (pr[2] * xm.x + pr[5] * xm.y + pr[8] * xm.z) * sz};
            const F3 r1 = {(pr[0] * rd.x + pr[3] * rd.y + pr[6] * rd.z) * sx, (pr[1] * rd.x + pr[4] * rd.y + pr[7] * rd.z) * sy,
                           (pr[2] * rd.x + pr[5] * rd.y + pr[8] * rd.z) * sz};
            const float ix = 1.0f / r1.x, iy = 1.0f / r1.y, iz = 1.0f / r1.z;
            const float ax = (-1.f - r0.x) * ix, bx = (1.f - r0.x) * ix;
            const float ay = (-1.f - r0.y) * iy, by = (1.f - r0.y) * iy;
            const float az = (-1.f - r0.z) * iz, bz = (1.f - r0.z) * iz;
            // the ray's interval inside primitive k, in t units from the current sample (step 0 of the chunk)
            const float trmin = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
            const float trmax = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
            // NaNs compare false everywhere: keep such a primitive.  (A ray lying in a face plane gives one bound
            // 0 * inf = NaN, but fminf / fmaxf drop it against the other bound's +-inf, so the interval stays ordered and
            // empty - the ray is not strictly inside; only non-finite inputs reach the unordered case.)
            const bool skip = (trmax < -2.f * stepsize) || (trmin > c_end + 2.f * stepsize) || (trmin > trmax + 4.f * stepsize);
            if (__any(live && !skip)) {
                if (lane == 0) sub[nsub] = k;
                if (nsub < NREC) {
                    // conservative step window of THIS ray inside primitive k during the chunk (two steps of margin each side;
                    // anything that does not compare cleanly - NaN, infinities - becomes "always")
                    float e0 = floorf(trmin / stepsize) - 2.f, e1 = ceilf(trmax / stepsize) + 2.f;
                    unsigned short w = 0x00ff;                                   // first 255 > last 0: never
                    if (live && !skip) {
                        const int i0 = (e0 >= 0.f && e0 <= 255.f) ? (int)e0 : (e0 > 255.f ? 255 : 0);
                        const int i1 = (e1 >= 0.f && e1 <= 255.f) ? (int)e1 : (e1 < 0.f ? 0 : 255);
                        w = (unsigned short)(i0 | (i1 << 8));
                        if (!(trmin <= trmax)) w = 0xff00;                       // unordered: evaluate every step
                    }
                    lds.span[wave][nsub][lane] = w;
                }
                ++nsub;
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        // The records of the chunk's cached primitives go to LDS once.  Per step a ray only compares the step index with
        // its window (2 bytes per ray per primitive, lane-linear LDS read); the record is fetched (LDS broadcast) and the
        // exact inside test / sample run only when some ray of the wave is within its window.
        st.chunks += 1; st.nsub += nsub;
        if (stats) st.c_rebuild += __builtin_readcyclecounter() - c_t0;
        const int ncache = min(nsub, NREC);
        float* recf = reinterpret_cast<float*>(lds.recs[wave]);
        for (int i = lane; i < ncache * 16; i += 64) {
            const int k = sub[i >> 4], j = i & 15;
            float v = 0.f;
            if (j < 3) v = ppos[k * 3 + j];
            else if (j < 12) v = prot[k * 9 + j - 3];
            else if (j < 15) v = pscl[k * 3 + j - 12];
            recf[i] = v;
        }
        __builtin_amdgcn_s_waitcnt(0x0070);
        __builtin_amdgcn_wave_barrier();
        for (int step = 0; step < CHUNK; ++step) {
            if (__all(t > rtmax + 1e-5f || vis.done())) break;
            st.steps += 1;
            for (int ks = 0; ks < nsub; ++ks) {
                float4 c0, c1, c2, c3;
                if (ks < NREC) {
                    const unsigned w = lds.span[wave][ks][lane];
                    const bool maybe = step >= (int)(w & 255u) && step <= (int)(w >> 8);
                    if (!__any(maybe)) continue;          // nobody near this primitive at this step: 6 instructions
                    c0 = lds.recs[wave][ks][0]; c1 = lds.recs[wave][ks][1]; c2 = lds.recs[wave][ks][2]; c3 = lds.recs[wave][ks][3];
                } else {   // beyond the cache (rare): straight from memory, every step
                    const int k = __builtin_amdgcn_readfirstlane(sub[ks]);
                    const float* pr_ = prot + k * 9;
                    c0 = {ppos[k * 3], ppos[k * 3 + 1], ppos[k * 3 + 2], pr_[0]};
                    c1 = {pr_[1], pr_[2], pr_[3], pr_[4]};
                    c2 = {pr_[5], pr_[6], pr_[7], pr_[8]};
                    c3 = {pscl[k * 3], pscl[k * 3 + 1], pscl[k * 3 + 2], 0.f};
                }
                const int k = __builtin_amdgcn_readfirstlane(sub[ks]);
                st.eval += 1;
                Local loc = {{rp.x - c0.x, rp.y - c0.y, rp.z - c0.z}, {c0.w, c1.x, c1.y, c1.z, c1.w, c2.x, c2.y, c2.z, c2.w},
                             {c3.x, c3.y, c3.z}, 0.f, 0.f, 0.f};
                const float* pr = loc.pr;
                const F3 xm = loc.xm;
                loc.yx = (pr[0] * xm.x + pr[3] * xm.y + pr[6] * xm.z) * c3.x;
                loc.yy = (pr[1] * xm.x + pr[4] * xm.y + pr[7] * xm.z) * c3.y;
                loc.yz = (pr[2] * xm.x + pr[5] * xm.y + pr[8] * xm.z) * c3.z;
                const bool in = loc.yx > -1.f && loc.yx < 1.f && loc.yy > -1.f && loc.yy < 1.f && loc.yz > -1.f && loc.yz < 1.f;
                vis.sample(in && !vis.done() && t < rtmax + 1e-5f, k, loc);
            }
            t += stepsize;
            rp = {rp.x + rd.x * stepsize, rp.y + rd.y * stepsize, rp.z + rd.z * stepsize};
        }
    }
}

// ---- what a taken sample is: the fade, the template cell and its trilinear weights (both visitors)
struct Cell { float fade, fx, fy, fz; int x0, y0, z0; };
__device__ __forceinline__ Cell cell_of(const Local& L, int TD, int TH, int TW, float fadescale, float fadeexp) {
    Cell c;
    // the reference's __powf / __expf are CUDA's fast forms 2^(y log2 x) and 2^(x log2 e); HIP's __powf is
    // the full-precision routine (~200 instructions - measured: 1900 VALU instructions per marching step)
    c.fade = fast_exp(-fadescale * (fast_pow(fabsf(L.yx), fadeexp) + fast_pow(fabsf(L.yy), fadeexp) +
                                    fast_pow(fabsf(L.yz), fadeexp)));
    const float gx = (L.yx + 1.f) * 0.5f * (float)(TW - 1), gy = (L.yy + 1.f) * 0.5f * (float)(TH - 1),
                gz = (L.yz + 1.f) * 0.5f * (float)(TD - 1);
    c.x0 = min(max((int)floorf(gx), 0), TW - 2); c.y0 = min(max((int)floorf(gy), 0), TH - 2);
    c.z0 = min(max((int)floorf(gz), 0), TD - 2);   // (no-op clamps: memory safety only)
    c.fx = gx - (float)c.x0; c.fy = gy - (float)c.y0; c.fz = gz - (float)c.z0;
    return c;
}
// |y| < 1 strictly => 0 <= x0 <= TW - 2 (and likewise y0, z0): all eight corners are inside the grid,
// the reference's zero-padding branch (utils.h:473-500) cannot trigger here
__device__ __forceinline__ float corner_weight(const Cell& c, int i) {
    return ((i & 1) ? c.fx : 1.f - c.fx) * (((i >> 1) & 1) ? c.fy : 1.f - c.fy) * ((i >> 2) ? c.fz : 1.f - c.fz);
}
__device__ __forceinline__ int corner_index(const Cell& c, int i, int sD, int sH) {
    return (c.z0 + (i >> 2)) * sD + (c.y0 + ((i >> 1) & 1)) * sH + c.x0 + (i & 1);
}

// The forward accumulation (primaccum.h:63-78).  KEEP_S: also keep the colour of the saturating sample (the backward's sweep 1).
template <bool KEEP_S>
struct AccumVisitor {
    const float4* tpl; int TD, TH, TW; float stepsize, fadescale, fadeexp; int stats;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    bool sat = false;
    F3 S = {0.f, 0.f, 0.f};
    __device__ __forceinline__ bool done() const { return sat; }
    __device__ __forceinline__ void sample(bool take, int k, const Local& L) {
        if (take) {
            const int sD = TW * TH, sH = TW;
            const Cell c = cell_of(L, TD, TH, TW, fadescale, fadeexp);
            const float4* v = tpl + (int64_t)k * TD * sD;
            float4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float wgt = corner_weight(c, i);
                const float4 q = (stats == 2) ? float4{0.5f, 0.5f, 0.5f, 5.f} : v[corner_index(c, i, sD, sH)];
                s.x += q.x * wgt; s.y += q.y * wgt; s.z += q.z * wgt; s.w += q.w * wgt;
            }
            const float alpha = s.w * c.fade;
            const float newalpha = acc.w + alpha * stepsize;
            const float contrib = fminf(newalpha, 1.f) - acc.w;
            acc.x += s.x * contrib; acc.y += s.y * contrib; acc.z += s.z * contrib; acc.w += contrib;
            if (newalpha >= 1.f) {
                sat = true;
                if (KEEP_S) S = {s.x, s.y, s.z};
            }
        }
    }
};

__global__ __launch_bounds__(256) void raymarch_kernel(const float* __restrict__ rayposim, const float* __restrict__ raydirim,
                                                      const float* __restrict__ tminmaxim, float stepsize,
                                                      const float* __restrict__ primpos, const float* __restrict__ primrot,
                                                      const float* __restrict__ primscale, const float4* __restrict__ tplate,
                                                      float4* __restrict__ rayrgba, int N, int H, int W, int K, int TD, int TH,
                                                      int TW, float fadescale, float fadeexp, int stats) {
    __shared__ MarchLds lds;
    const TileId id = tile_id(H, W);
    Ray ray;
    ray.rp = ld3(rayposim + id.pix * 3);
    ray.rd = ld3(raydirim + id.pix * 3);
    ray.tmin0 = tminmaxim[id.pix * 2]; ray.tmax0 = tminmaxim[id.pix * 2 + 1];
    const Prims P = {primpos + (int64_t)id.n * K * 3, primrot + (int64_t)id.n * K * 9, primscale + (int64_t)id.n * K * 3};

    const unsigned long long c_start = stats ? __builtin_readcyclecounter() : 0;
    tile_hit_list(P, K, id.lane, lds.hits[id.wave], ray);
    const unsigned long long c_hit = stats ? __builtin_readcyclecounter() : 0;
    AccumVisitor<false> vis = {tplate + (int64_t)id.n * K * TD * TH * TW, TD, TH, TW, stepsize, fadescale, fadeexp, stats};
    MarchStats st;
    march_sweep(P, lds, id.wave, id.lane, ray, stepsize, vis, stats, st);
    if (id.valid) rayrgba[id.pix] = vis.acc;
    if (stats && id.lane == 0) {
        atomicAdd(&g_rm_stats[0], 1ull); atomicAdd(&g_rm_stats[1], (unsigned long long)ray.num);
        atomicAdd(&g_rm_stats[2], st.chunks ? 1ull : 0ull); atomicAdd(&g_rm_stats[3], st.chunks); atomicAdd(&g_rm_stats[4], st.nsub);
        atomicAdd(&g_rm_stats[5], st.steps); atomicAdd(&g_rm_stats[6], st.eval);
        const unsigned long long c_end = __builtin_readcyclecounter();
        atomicAdd(&g_rm_stats[7], c_hit - c_start); atomicAdd(&g_rm_stats[8], st.c_rebuild); atomicAdd(&g_rm_stats[9], c_end - c_hit - st.c_rebuild);
        atomicMax(&g_rm_stats[10], c_end - c_start);
    }
}

// ---- backward (primaccum.h:81-98, PrimSamplerTW::backward, PrimTransfSRT::backward; the rules are in include/primx_hip.h)
// Sum over the wave's 64 lanes in a fixed butterfly order; every lane ends with the same bits.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// Template adds are run-length merged per lane: the lane keeps one (primitive, cell) entry with its 8 x 4 partial sums in
// registers and flushes it (32 atomic adds) when the primitive or the cell changes, and at the end of the ray.  A ray stays in
// one cell of one primitive for on the order of a hundred shipped steps, but where primitives overlap its samples alternate
// between them step by step and the single entry is flushed each time (DESIGN.md "Differentiable ray marcher": measured).
struct GradVisitor {
    const float4* tpl; float* gtpl; float* gpos; float* grot; float* gscl;   // this batch item's arrays; the four may be null
    int TD, TH, TW; float stepsize, fadescale, fadeexp; int lane;
    float4 dL; bool raysat; F3 S;                                            // from the ray's grad_rayrgba and sweep 1
    float A = 0.f;
    bool sat = false;
    unsigned n_taken = 0, n_sums = 0, n_flush = 0;                           // PRIMX_RAYMARCH_STATS
    int64_t cell = -1;                                                       // the entry's first corner (float4 index), -1: none
    float part[8][4];
    __device__ __forceinline__ void flush() {
        if (cell >= 0) {
            const int sD = TW * TH, sH = TW;
            n_flush += 1;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float* g = gtpl + (cell + (i >> 2) * sD + ((i >> 1) & 1) * sH + (i & 1)) * 4;
                atomicAdd(g, part[i][0]); atomicAdd(g + 1, part[i][1]); atomicAdd(g + 2, part[i][2]); atomicAdd(g + 3, part[i][3]);
            }
        }
        cell = -1;
    }
    __device__ __forceinline__ bool done() const { return sat; }
    __device__ __forceinline__ void sample(bool take, int k, const Local& L) {
        if (!__any(take)) return;
        const bool srt = gpos || grot || gscl;                               // wave-uniform
        float gyx = 0.f, gyy = 0.f, gyz = 0.f;
        n_sums += 1;
        if (take) {
            n_taken += 1;
            const int sD = TW * TH, sH = TW;
            const Cell c = cell_of(L, TD, TH, TW, fadescale, fadeexp);
            const int64_t base = (int64_t)k * TD * sD;
            float4 q[8];
            float4 raw = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float wgt = corner_weight(c, i);
                q[i] = tpl[base + corner_index(c, i, sD, sH)];
                raw.x += q[i].x * wgt; raw.y += q[i].y * wgt; raw.z += q[i].z * wgt; raw.w += q[i].w * wgt;
            }
            const float a = raw.w * c.fade;
            const float newalpha = A + a * stepsize;                         // the forward's expressions: the same decisions
            const bool sat_now = newalpha >= 1.f;
            const float weight = sat_now ? 1.f - A : a * stepsize;
            const float grx = weight * dL.x, gry = weight * dL.y, grz = weight * dL.z;
            float ga = 0.f;
            if (!sat_now)
                ga = stepsize * ((raw.x - S.x) * dL.x + (raw.y - S.y) * dL.y + (raw.z - S.z) * dL.z + (raysat ? 0.f : dL.w));
            A += fminf(newalpha, 1.f) - A;
            if (sat_now) sat = true;
            const float gw = ga * c.fade;                                    // gradient of raw.w
            if (gtpl) {
                const int64_t here = base + corner_index(c, 0, sD, sH);
                if (here != cell) {
                    flush();
                    cell = here;
#pragma unroll
                    for (int i = 0; i < 8; ++i) part[i][0] = part[i][1] = part[i][2] = part[i][3] = 0.f;
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float wgt = corner_weight(c, i);
                    part[i][0] += wgt * grx; part[i][1] += wgt * gry; part[i][2] += wgt * grz; part[i][3] += wgt * gw;
                }
            }
            if (srt) {
                // d raw / d f along each axis inside the cell: sum_c dw_c/df (raw_c . G), G = (g_rgb, gw)
                float dx = 0.f, dy = 0.f, dz = 0.f;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float d = q[i].x * grx + q[i].y * gry + q[i].z * grz + q[i].w * gw;
                    const float wx = (i & 1) ? c.fx : 1.f - c.fx, wy = ((i >> 1) & 1) ? c.fy : 1.f - c.fy, wz = (i >> 2) ? c.fz : 1.f - c.fz;
                    dx += ((i & 1) ? d : -d) * wy * wz;
                    dy += (((i >> 1) & 1) ? d : -d) * wx * wz;
                    dz += ((i >> 2) ? d : -d) * wx * wy;
                }
                // d fade / d y_d = fade (-fs fe |y_d|^(fe-1) sign(y_d)), sign(0) = 0
                const float f = -fadescale * fadeexp * a * ga;
                const float ax = fabsf(L.yx), ay = fabsf(L.yy), az = fabsf(L.yz);
                gyx = dx * 0.5f * (float)(TW - 1) + (L.yx != 0.f ? f * copysignf(fast_pow(ax, fadeexp - 1.f), L.yx) : 0.f);
                gyy = dy * 0.5f * (float)(TH - 1) + (L.yy != 0.f ? f * copysignf(fast_pow(ay, fadeexp - 1.f), L.yy) : 0.f);
                gyz = dz * 0.5f * (float)(TD - 1) + (L.yz != 0.f ? f * copysignf(fast_pow(az, fadeexp - 1.f), L.yz) : 0.f);
            }
        }
        if (srt) {
            // y_i = u_i s_i, u_i = sum_j rot[j][i] xm_j (rot[j][i] = pr[3 j + i]); lanes that do not take the sample hold g_y = 0
            const float* pr = L.pr;
            const float xm[3] = {L.xm.x, L.xm.y, L.xm.z};
            const float s[3] = {L.s.x, L.s.y, L.s.z};
            const float gy[3] = {gyx, gyy, gyz};
            float v[15];
#pragma unroll
            for (int i = 0; i < 3; ++i) v[i] = (pr[i] * xm[0] + pr[3 + i] * xm[1] + pr[6 + i] * xm[2]) * gy[i];      // gscale_i
#pragma unroll
            for (int j = 0; j < 3; ++j) {
#pragma unroll
                for (int i = 0; i < 3; ++i) v[3 + 3 * j + i] = xm[j] * s[i] * gy[i];                                 // grot[j][i]
                v[12 + j] = -(pr[3 * j] * s[0] * gy[0] + pr[3 * j + 1] * s[1] * gy[1] + pr[3 * j + 2] * s[2] * gy[2]);   // gpos_j
            }
#pragma unroll
            for (int i = 0; i < 15; ++i) v[i] = wave_sum(v[i]);
            if (lane == 0) {
                if (gscl) for (int i = 0; i < 3; ++i) atomicAdd(gscl + k * 3 + i, v[i]);
                if (grot) for (int i = 0; i < 9; ++i) atomicAdd(grot + k * 9 + i, v[3 + i]);
                if (gpos) for (int i = 0; i < 3; ++i) atomicAdd(gpos + k * 3 + i, v[12 + i]);
            }
        }
    }
};

__global__ __launch_bounds__(256) void raymarch_backward_kernel(const float* __restrict__ rayposim, const float* __restrict__ raydirim,
                                                               const float* __restrict__ tminmaxim, float stepsize,
                                                               const float* __restrict__ primpos, const float* __restrict__ primrot,
                                                               const float* __restrict__ primscale, const float4* __restrict__ tplate,
                                                               const float4* __restrict__ grad_rayrgba, float* gtemplate,
                                                               float* gprimpos, float* gprimrot, float* gprimscale, int N, int H,
                                                               int W, int K, int TD, int TH, int TW, float fadescale, float fadeexp,
                                                               int stats) {
    __shared__ MarchLds lds;
    const TileId id = tile_id(H, W);
    const float4 dL = grad_rayrgba[id.pix];
    const bool active = id.valid && (dL.x != 0.f || dL.y != 0.f || dL.z != 0.f || dL.w != 0.f);
    if (!__any(active)) return;                                              // wave-uniform: nothing to add from this tile
    Ray ray;
    ray.rp = ld3(rayposim + id.pix * 3);
    ray.rd = ld3(raydirim + id.pix * 3);
    ray.tmin0 = tminmaxim[id.pix * 2]; ray.tmax0 = tminmaxim[id.pix * 2 + 1];
    const Prims P = {primpos + (int64_t)id.n * K * 3, primrot + (int64_t)id.n * K * 9, primscale + (int64_t)id.n * K * 3};
    const float4* tpl = tplate + (int64_t)id.n * K * TD * TH * TW;
    tile_hit_list(P, K, id.lane, lds.hits[id.wave], ray);                    // every lane, shadow lanes included, as in the forward
    MarchStats st;
    // sweep 1: the forward accumulation -> does the ray saturate, and with which colour.  An inactive lane is "done" from the
    // start in both sweeps: it takes no sample, and the filters stay conservative for the lanes that do.
    AccumVisitor<true> fwd = {tpl, TD, TH, TW, stepsize, fadescale, fadeexp, 0};
    fwd.sat = !active;
    march_sweep(P, lds, id.wave, id.lane, ray, stepsize, fwd, 0, st);
    // sweep 2: the gradients
    GradVisitor g = {tpl, gtemplate ? gtemplate + (int64_t)id.n * K * TD * TH * TW * 4 : nullptr,
                     gprimpos ? gprimpos + (int64_t)id.n * K * 3 : nullptr, gprimrot ? gprimrot + (int64_t)id.n * K * 9 : nullptr,
                     gprimscale ? gprimscale + (int64_t)id.n * K * 3 : nullptr, TD, TH, TW, stepsize, fadescale, fadeexp, id.lane,
                     dL, active && fwd.sat, fwd.S};
    g.sat = !active;
    march_sweep(P, lds, id.wave, id.lane, ray, stepsize, g, 0, st);
    if (g.gtpl) g.flush();
    if (stats) {
        unsigned taken = g.n_taken, flushes = g.n_flush;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) { taken += __shfl_xor(taken, m, 64); flushes += __shfl_xor(flushes, m, 64); }
        if (id.lane == 0) {
            atomicAdd(&g_rm_bwd_stats[0], (unsigned long long)taken); atomicAdd(&g_rm_bwd_stats[1], (unsigned long long)g.n_sums);
            atomicAdd(&g_rm_bwd_stats[2], (unsigned long long)flushes);
        }
    }
}

}  // namespace

extern "C" int primx_compute_raydirs(const float* viewpos, const float* viewrot, const float* focal, const float* princpt,
                                     const float* pixelcoords, float volradius, float* raypos, float* raydir, float* tminmax,
                                     int N, int H, int W, void* stream) {
    PRIMX_REQUIRE(viewpos && viewrot && focal && princpt && raypos && raydir && tminmax, "primx_compute_raydirs: null pointer");
    PRIMX_REQUIRE(N > 0 && H > 0 && W > 0 && volradius > 0.f, "primx_compute_raydirs: empty problem");
    const int64_t n = (int64_t)N * H * W;
    hipLaunchKernelGGL(raydirs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, viewpos, viewrot,
                       focal, princpt, pixelcoords, volradius, raypos, raydir, tminmax, N, H, W);
    PRIMX_CHECK_LAUNCH("primx_compute_raydirs");
    return PRIMX_OK;
}

extern "C" int primx_raymarch(const float* raypos, const float* raydir, const float* tminmax, float stepsize,
                              const float* primpos, const float* primrot, const float* primscale, const float* tplate,
                              float* rayrgba, int N, int H, int W, int K, int TD, int TH, int TW, float fadescale,
                              float fadeexp, void* stream) {
    PRIMX_REQUIRE(raypos && raydir && tminmax && primpos && primrot && primscale && tplate && rayrgba,
                  "primx_raymarch: null pointer");
    PRIMX_REQUIRE(N > 0 && H > 0 && W > 0 && K > 0 && TD > 1 && TH > 1 && TW > 1 && stepsize > 0.f,
                  "primx_raymarch: empty problem / non-positive step");
    static const int stats = [] { const char* e = getenv("PRIMX_RAYMARCH_STATS"); return e ? atoi(e) : 0; }();   // 2: no template fetch
    unsigned long long z[12] = {0}, r[12];
    if (stats) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_rm_stats), z, sizeof(z));
    hipLaunchKernelGGL(raymarch_kernel, dim3((W + 15) / 16, (H + 15) / 16, N), dim3(256), 0, (hipStream_t)stream, raypos,
                       raydir, tminmax, stepsize, primpos, primrot, primscale, (const float4*)tplate, (float4*)rayrgba, N, H, W,
                       K, TD, TH, TW, fadescale, fadeexp, stats);
    if (stats) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)hipMemcpyFromSymbol(r, HIP_SYMBOL(g_rm_stats), sizeof(r));
        const double w = r[0] ? (double)r[0] : 1.0, mw = r[2] ? (double)r[2] : 1.0;
        fprintf(stderr, "raymarch stats: %llu waves, hit list %.1f per wave; %llu marching waves: %.1f chunks, %.1f listed per chunk, "
                        "%.0f steps, %.1f record evaluations per step; cycles per wave: hit list %.0f, rebuilds %.0f (per marching wave), "
                        "marching %.0f (per marching wave), slowest wave %llu\n", r[0], r[1] / w, r[2], r[3] / mw, r[4] / (r[3] ? (double)r[3] : 1.0),
                r[5] / mw, r[6] / (r[5] ? (double)r[5] : 1.0), r[7] / w, r[8] / mw, r[9] / mw, r[10]);
    }
    PRIMX_CHECK_LAUNCH("primx_raymarch");
    return PRIMX_OK;
}

extern "C" int primx_raymarch_backward(const float* raypos, const float* raydir, const float* tminmax, float stepsize,
                                       const float* primpos, const float* primrot, const float* primscale, const float* tplate,
                                       const float* grad_rayrgba, float* gtemplate, float* gprimpos, float* gprimrot,
                                       float* gprimscale, int N, int H, int W, int K, int TD, int TH, int TW, float fadescale,
                                       float fadeexp, void* stream) {
    PRIMX_REQUIRE(raypos && raydir && tminmax && primpos && primrot && primscale && tplate && grad_rayrgba,
                  "primx_raymarch_backward: null pointer");
    PRIMX_REQUIRE(gtemplate || gprimpos || gprimrot || gprimscale, "primx_raymarch_backward: all four gradient arrays are null");
    PRIMX_REQUIRE(N > 0 && H > 0 && W > 0 && K > 0 && TD > 1 && TH > 1 && TW > 1 && stepsize > 0.f,
                  "primx_raymarch_backward: empty problem / non-positive step");
    PRIMX_REQUIRE((int64_t)TD * TH * TW < ((int64_t)1 << 31) && 9 * (int64_t)K < ((int64_t)1 << 31),
                  "primx_raymarch_backward: TD * TH * TW and 9 * K must be < 2^31 (got K = %d, template %d x %d x %d)", K, TD, TH, TW);
    // PRIMX_RAYMARCH_STATS != 0 (tools/raymarch_grad_bench.py): count the launch's atomic adds; synchronises, so never set it in production
    static const int stats = [] { const char* e = getenv("PRIMX_RAYMARCH_STATS"); return e ? atoi(e) : 0; }();
    unsigned long long z[3] = {0, 0, 0}, r[3];
    if (stats) (void)hipMemcpyToSymbol(HIP_SYMBOL(g_rm_bwd_stats), z, sizeof(z));
    hipLaunchKernelGGL(raymarch_backward_kernel, dim3((W + 15) / 16, (H + 15) / 16, N), dim3(256), 0, (hipStream_t)stream, raypos,
                       raydir, tminmax, stepsize, primpos, primrot, primscale, (const float4*)tplate, (const float4*)grad_rayrgba,
                       gtemplate, gprimpos, gprimrot, gprimscale, N, H, W, K, TD, TH, TW, fadescale, fadeexp, stats);
    if (stats) {
        (void)hipStreamSynchronize((hipStream_t)stream);
        (void)hipMemcpyFromSymbol(r, HIP_SYMBOL(g_rm_bwd_stats), sizeof(r));
        const unsigned long long per_sum = (gprimscale ? 3 : 0) + (gprimrot ? 9 : 0) + (gprimpos ? 3 : 0);
        fprintf(stderr, "raymarch backward stats: %llu taken samples (%llu template atomic adds unmerged), %llu template atomic adds, %llu wave sums, "
                        "%llu SRT atomic adds\n", r[0], gtemplate ? 32 * r[0] : 0ull,
                gtemplate ? 32 * r[2] : 0ull, per_sum ? r[1] : 0ull, per_sum * r[1]);
    }
    PRIMX_CHECK_LAUNCH("primx_raymarch_backward");
    return PRIMX_OK;
}
