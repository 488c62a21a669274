// The per-ray and per-pair arithmetic of the mesh ray query (meshbvh.hip): the watertight ray / triangle test of Woop, Benthin
// and Wald 2013 ("Watertight ray/triangle intersection") on the face records of meshfield_pair.h, and the box test that is
// conservative with respect to it.  Rules: include/primx_hip.h "Mesh rays" (R1-R6); restatement: tests/meshray_numpy.py.
// Include inside the translation unit's anonymous namespace, after meshfield_pair.h, with contraction off: every expression is
// evaluated as written.
#pragma once

constexpr float RAY_T_MARGIN = 0x1p-20f;     // R5: the node's t interval is widened by this times its larger |end|

__device__ __forceinline__ float sel3(int k, float x, float y, float z) { return k == 0 ? x : (k == 1 ? y : z); }

// R1: the ray in its own frame.  kz = the direction's largest |component| (the first of equals), kx and ky the next two in
// cyclic order, swapped when d[kz] < 0; the shear S = (d[kx] / d[kz], d[ky] / d[kz], 1 / d[kz]).
struct Ray {
    float ox, oy, oz;                        // the origin, permuted: (o[kx], o[ky], o[kz])
    float sx, sy, sz;
    int kx, ky, kz;
    bool ok;                                 // finite origin and direction, 1 / d[kz] finite
};

__device__ __forceinline__ Ray ray_setup(float ox, float oy, float oz, float dx, float dy, float dz) {
    Ray r;
    const float ax = fabsf(dx), ay = fabsf(dy), az = fabsf(dz);
    r.kz = 0;
    if (ay > ax) r.kz = 1;
    if (az > fmaxf(ax, ay)) r.kz = 2;
    r.kx = r.kz == 2 ? 0 : r.kz + 1;
    r.ky = r.kx == 2 ? 0 : r.kx + 1;
    const float dk = sel3(r.kz, dx, dy, dz);
    if (dk < 0.0f) {
        const int s = r.kx;
        r.kx = r.ky, r.ky = s;
    }
    r.sx = sel3(r.kx, dx, dy, dz) / dk;
    r.sy = sel3(r.ky, dx, dy, dz) / dk;
    r.sz = 1.0f / dk;
    r.ox = sel3(r.kx, ox, oy, oz), r.oy = sel3(r.ky, ox, oy, oz), r.oz = sel3(r.kz, ox, oy, oz);
    const float big = INFINITY;
    r.ok = fabsf(ox) < big && fabsf(oy) < big && fabsf(oz) < big && ax < big && ay < big && az < big && fabsf(r.sz) < big;
    return r;
}

// R2, R3: the record against the ray -> accepted; t, and the barycentrics (v, w) of hit = a + v ab + w ac
__device__ __forceinline__ bool ray_pair(const Ray& q, const Rec& r, float tmin, float tmax, float& t, float& v, float& w) {
    if (r.kind != 0) return false;
    const float az = sel3(q.kz, r.ax, r.ay, r.az) - q.oz, bz = sel3(q.kz, r.bx, r.by, r.bz) - q.oz,
                cz = sel3(q.kz, r.cx, r.cy, r.cz) - q.oz;
    const float ax = (sel3(q.kx, r.ax, r.ay, r.az) - q.ox) - q.sx * az, ay = (sel3(q.ky, r.ax, r.ay, r.az) - q.oy) - q.sy * az;
    const float bx = (sel3(q.kx, r.bx, r.by, r.bz) - q.ox) - q.sx * bz, by = (sel3(q.ky, r.bx, r.by, r.bz) - q.oy) - q.sy * bz;
    const float cx = (sel3(q.kx, r.cx, r.cy, r.cz) - q.ox) - q.sx * cz, cy = (sel3(q.ky, r.cx, r.cy, r.cz) - q.oy) - q.sy * cz;
    float U = cx * by - cy * bx, V = ax * cy - ay * cx, W = bx * ay - by * ax;
    bool neg = U < 0.0f || V < 0.0f || W < 0.0f, pos = U > 0.0f || V > 0.0f || W > 0.0f;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {               // on an edge or a vertex to fp32: the signs from float64
        const double Ud = (double)cx * (double)by - (double)cy * (double)bx;
        const double Vd = (double)ax * (double)cy - (double)ay * (double)cx;
        const double Wd = (double)bx * (double)ay - (double)by * (double)ax;
        neg = Ud < 0.0 || Vd < 0.0 || Wd < 0.0, pos = Ud > 0.0 || Vd > 0.0 || Wd > 0.0;
        U = (float)Ud, V = (float)Vd, W = (float)Wd;
    }
    if (neg && pos) return false;
    const float det = (U + V) + W;
    if (det == 0.0f || !(fabsf(det) < INFINITY)) return false;
    const float T = (U * (q.sz * az) + V * (q.sz * bz)) + W * (q.sz * cz);
    t = T / det;
    v = V / det, w = W / det;
    return tmin <= t && t <= tmax;                           // (a NaN is refused)
}

// R5: the node's box (lo.x, lo.y, lo.z, hi.x) (hi.y, hi.z, ..) against the ray, in the ray's frame -> whether a record below it
// can be accepted in [tmin, best]; tn = where its interval starts
__device__ __forceinline__ bool ray_box(const Ray& q, const float4& q0, const float4& q1, float tmin, float best, float& tn) {
    const float z0 = sel3(q.kz, q0.x, q0.y, q0.z) - q.oz, z1 = sel3(q.kz, q0.w, q1.x, q1.y) - q.oz;
    const float x0 = sel3(q.kx, q0.x, q0.y, q0.z) - q.ox, x1 = sel3(q.kx, q0.w, q1.x, q1.y) - q.ox;
    const float y0 = sel3(q.ky, q0.x, q0.y, q0.z) - q.oy, y1 = sel3(q.ky, q0.w, q1.x, q1.y) - q.oy;
    const float mx0 = fminf(q.sx * z0, q.sx * z1), mx1 = fmaxf(q.sx * z0, q.sx * z1);
    const float my0 = fminf(q.sy * z0, q.sy * z1), my1 = fmaxf(q.sy * z0, q.sy * z1);
    const float zl = fminf(q.sz * z0, q.sz * z1), zh = fmaxf(q.sz * z0, q.sz * z1);
    const float m = fmaxf(fabsf(zl), fabsf(zh)) * RAY_T_MARGIN;
    tn = zl - m;
    const float tf = zh + m;
    // every comparison is written so that a NaN keeps the node
    return !(x0 - mx1 > 0.0f) && !(x1 - mx0 < 0.0f) && !(y0 - my1 > 0.0f) && !(y1 - my0 < 0.0f) && !(tn > best) && !(tf < tmin);
}
