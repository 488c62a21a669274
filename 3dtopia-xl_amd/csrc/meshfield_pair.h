// The per-pair arithmetic of the mesh field query, stated once for the brute-force query (meshfield.hip) and the BVH query
// (meshbvh.hip): Ericson's seven regions, the zero-area rule, the Van Oosterom-Strackee term, the 64-byte face record and the
// preparation launch that writes it.  Rules: include/primx_hip.h "Primitive fitting".  Include inside the translation unit's
// anonymous namespace, after mesh_common.h, with contraction off: every expression is evaluated as written, so both queries
// get the same bits from the same (point, face).
#pragma once

constexpr int64_t WS_HEAD = 64;          // bytes in front of the records: the index-check flag

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// kind: 0 triangle; 1 / 2 / 3 zero-area, measured as the segment ab / ac / bc (the longest edge, the first of equals; a
// point is the segment ab of length 0); -1 an index outside [0, V) (the host refuses the call: never evaluated)
struct Rec {
    float ax, ay, az, bx, by, bz, cx, cy, cz, abx, aby, abz, acx, acy, acz;
    int kind;
};

__device__ __forceinline__ Rec unpack(const float4* r) {
    const float4 r0 = r[0], r1 = r[1], r2 = r[2], r3 = r[3];
    Rec o;
    o.ax = r0.x, o.ay = r0.y, o.az = r0.z, o.bx = r0.w, o.by = r1.x, o.bz = r1.y, o.cx = r1.z, o.cy = r1.w, o.cz = r2.x;
    o.abx = r2.y, o.aby = r2.z, o.abz = r2.w, o.acx = r3.x, o.acy = r3.y, o.acz = r3.z;
    o.kind = __float_as_int(r3.w);
    return o;
}

// squared distance to the record's closest point q = a + v ab + w ac, and the Van Oosterom-Strackee atan2 term
__device__ __forceinline__ void pair(float px, float py, float pz, const Rec& r, int kind, float& d2, float& v, float& w,
                                     float& term) {
    const float apx = px - r.ax, apy = py - r.ay, apz = pz - r.az;
    const float bpx = px - r.bx, bpy = py - r.by, bpz = pz - r.bz;
    const float cpx = px - r.cx, cpy = py - r.cy, cpz = pz - r.cz;
    if (kind != 0) {
        term = 0.0f;
        v = 0.0f, w = 0.0f, d2 = INFINITY;
        if (kind < 0) return;
        float ex = r.abx, ey = r.aby, ez = r.abz, ox = apx, oy = apy, oz = apz;
        if (kind == 2) ex = r.acx, ey = r.acy, ez = r.acz;
        if (kind == 3) ex = r.cx - r.bx, ey = r.cy - r.by, ez = r.cz - r.bz, ox = bpx, oy = bpy, oz = bpz;
        const float l = dot3(ex, ey, ez, ex, ey, ez);
        float t = l > 0.0f ? dot3(ox, oy, oz, ex, ey, ez) / l : 0.0f;
        t = fminf(fmaxf(t, 0.0f), 1.0f);
        if (kind == 1) v = t;
        if (kind == 2) w = t;
        if (kind == 3) v = 1.0f - t, w = t;
        const float qx = (r.ax + r.abx * v) + r.acx * w, qy = (r.ay + r.aby * v) + r.acy * w, qz = (r.az + r.abz * v) + r.acz * w;
        const float dx = px - qx, dy = py - qy, dz = pz - qz;
        d2 = dot3(dx, dy, dz, dx, dy, dz);
        return;
    }
    const float la2 = dot3(apx, apy, apz, apx, apy, apz), lb2 = dot3(bpx, bpy, bpz, bpx, bpy, bpz),
                lc2 = dot3(cpx, cpy, cpz, cpx, cpy, cpz);
    const float d1 = dot3(r.abx, r.aby, r.abz, apx, apy, apz), d2a = dot3(r.acx, r.acy, r.acz, apx, apy, apz);
    const float d3 = dot3(r.abx, r.aby, r.abz, bpx, bpy, bpz), d4 = dot3(r.acx, r.acy, r.acz, bpx, bpy, bpz);
    const float d5 = dot3(r.abx, r.aby, r.abz, cpx, cpy, cpz), d6 = dot3(r.acx, r.acy, r.acz, cpx, cpy, cpz);
    const float vc = d1 * d4 - d3 * d2a, vb = d5 * d2a - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    // the seven Voronoi regions in Ericson's order A, B, AB, C, AC, BC, face: the later assignment wins
    float nv = vb, nw = vc, den = (va + vb) + vc;
    int region = 6;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) nv = 0.0f, nw = e43, den = e43 + e56, region = 5;
    if (vb <= 0.0f && d2a >= 0.0f && d6 <= 0.0f) nv = 0.0f, nw = d2a, den = d2a - d6, region = 4;
    if (d6 >= 0.0f && d5 <= d6) region = 3;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) nv = d1, nw = 0.0f, den = d1 - d3, region = 2;
    if (d3 >= 0.0f && d4 <= d3) region = 1;
    if (d1 <= 0.0f && d2a <= 0.0f) region = 0;
    const float inv = den != 0.0f ? 1.0f / den : 0.0f;
    v = nv * inv, w = nw * inv;
    if (region == 5) v = 1.0f - w;
    const float qx = (r.ax + r.abx * v) + r.acx * w, qy = (r.ay + r.aby * v) + r.acy * w, qz = (r.az + r.abz * v) + r.acz * w;
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    d2 = dot3(dx, dy, dz, dx, dy, dz);
    if (region == 0) d2 = la2, v = 0.0f, w = 0.0f;
    if (region == 1) d2 = lb2, v = 1.0f, w = 0.0f;
    if (region == 3) d2 = lc2, v = 0.0f, w = 1.0f;
    const float la = sqrtf(la2), lb = sqrtf(lb2), lc = sqrtf(lc2);
    const float nx = bpy * cpz - bpz * cpy, ny = bpz * cpx - bpx * cpz, nz = bpx * cpy - bpy * cpx;
    const float num = -dot3(apx, apy, apz, nx, ny, nz);
    const float dn = (((la * lb) * lc + dot3(apx, apy, apz, bpx, bpy, bpz) * lc) + dot3(bpx, bpy, bpz, cpx, cpy, cpz) * la) +
                     dot3(cpx, cpy, cpz, apx, apy, apz) * lb;
    term = atan2f(num, dn);
}

// record t of face t, or (ORDERED) of face order[t]: the BVH keeps its records in the order of its leaves.  An entry of
// `order` outside [0, F) sets bit 1 of the status and leaves a record of kind -1, as an index outside [0, V) sets bit 0.
template <bool ORDERED>
__global__ __launch_bounds__(THREADS) void mf_prep_kernel(const float* __restrict__ v, const int* __restrict__ f, int V, int F,
                                                          const int* __restrict__ order, float4* __restrict__ recs,
                                                          int* __restrict__ status) {
    const int t = blockIdx.x * THREADS + threadIdx.x;
    if (t >= F) return;
    float4* o = recs + (int64_t)4 * t;
    int face = t;
    if (ORDERED) {
        face = order[t];
        if (face < 0 || face >= F) {
            atomicOr(status, 2);
            const float4 z = {0.0f, 0.0f, 0.0f, 0.0f};
            o[0] = z, o[1] = z, o[2] = z;
            o[3] = float4{0.0f, 0.0f, 0.0f, __int_as_float(-1)};
            return;
        }
    }
    const int i0 = f[(int64_t)3 * face], i1 = f[(int64_t)3 * face + 1], i2 = f[(int64_t)3 * face + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
        atomicOr(status, 1);
        const float4 z = {0.0f, 0.0f, 0.0f, 0.0f};
        o[0] = z, o[1] = z, o[2] = z;
        o[3] = float4{0.0f, 0.0f, 0.0f, __int_as_float(-1)};
        return;
    }
    const float ax = v[(int64_t)3 * i0], ay = v[(int64_t)3 * i0 + 1], az = v[(int64_t)3 * i0 + 2];
    const float bx = v[(int64_t)3 * i1], by = v[(int64_t)3 * i1 + 1], bz = v[(int64_t)3 * i1 + 2];
    const float cx = v[(int64_t)3 * i2], cy = v[(int64_t)3 * i2 + 1], cz = v[(int64_t)3 * i2 + 2];
    const float abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
    const float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
    int kind = 0;
    if (nx == 0.0f && ny == 0.0f && nz == 0.0f) {
        const float bcx = cx - bx, bcy = cy - by, bcz = cz - bz;
        float best = dot3(abx, aby, abz, abx, aby, abz);
        const float lac = dot3(acx, acy, acz, acx, acy, acz), lbc = dot3(bcx, bcy, bcz, bcx, bcy, bcz);
        kind = 1;
        if (lac > best) best = lac, kind = 2;
        if (lbc > best) kind = 3;
    }
    o[0] = float4{ax, ay, az, bx};
    o[1] = float4{by, bz, cx, cy};
    o[2] = float4{cz, abx, aby, abz};
    o[3] = float4{acx, acy, acz, __int_as_float(kind)};
}


inline int check_mesh(const char* name, const void* v, const void* f, int V, int F) {
    PRIMX_REQUIRE(v && f, "%s: null pointer", name);
    PRIMX_REQUIRE(V >= 1 && F >= 1, "%s: V and F must be at least 1 (got %d, %d)", name, V, F);
    PRIMX_REQUIRE(V <= INT32_MAX / 3 && F <= INT32_MAX / 4, "%s: 3 V and 4 F must stay below 2^31", name);
    return PRIMX_OK;
}
