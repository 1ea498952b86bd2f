// gut_render_common.inl - what both compositing units (gut_render.hip, gut_render_k.hip) need: rays, tile entries and their staging, the accept
// test and the response of a pixel pair, the image stores, the sorted hit buffer that the SH kernels (gut_render_k.hip) share with the
// feature kernels behind it (gut_render.hip), the launch grids and the degree / K dispatch.  Templates, __forceinline__ device functions and
// static host helpers only: including this file emits no code.
#pragma once
#include <hip/hip_fp16.h>

#include "gut_internal.hpp"

namespace grut {

namespace {

// ---------------------------------------------------------------------------------------------
// rays (rayPayload.cuh:75-108, bounding_box.h:89-140)
// ---------------------------------------------------------------------------------------------
struct Ray {
    f3 o, d;
    float tmin, tmax;
    bool valid;
    bool inside;   // pixel lies in the image (a ray that misses the scene box is inside but not valid)
};
__device__ __forceinline__ void swapf(float& a, float& b) { const float t = a; a = b; b = t; }
// (a.x b.x + a.y b.y) + a.z b.z with every product and sum rounded on its own (the checker's v3_dot under -ffp-contract=off)
__device__ __forceinline__ float rn_dot3(float ax, float ay, float az, f3 b) { return add_rn(add_rn(mul_rn(ax, b.x), mul_rn(ay, b.y)), mul_rn(az, b.z)); }
__device__ __forceinline__ float rn_dot3(f3 a, f3 b) { return rn_dot3(a.x, a.y, a.z, b); }
__device__ __forceinline__ Ray init_ray(const GutParams& P, const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                        int px, int py) {
    Ray r;
    r.valid = false;
    r.inside = false;
    r.o = mk3(0.f, 0.f, 0.f);
    r.d = mk3(0.f, 0.f, 1.f);
    r.tmin = r.tmax = 0.f;
    if (px >= P.W || py >= P.H) return r;
    r.inside = true;
    const size_t pix = (size_t)py * P.W + px;
    const f3 so = mk3(ray_o[3 * pix], ray_o[3 * pix + 1], ray_o[3 * pix + 2]);
    const f3 sd = mk3(ray_d[3 * pix], ray_d[3 * pix + 1], ray_d[3 * pix + 2]);
    const FramePoses& FP = frame_poses(P);
    const float* R = FP.s2w_R;
    // world-space ray = pose . (o, d) (rayPayload.cuh:75-108) in the checker's operation order - rows dotted left to right, separately
    // rounded, then the translation: the sorted mode orders hits by distances computed from these bits (oracle_order_hit_t)
    r.o = mk3(add_rn(rn_dot3(R[0], R[1], R[2], so), FP.s2w_t[0]), add_rn(rn_dot3(R[3], R[4], R[5], so), FP.s2w_t[1]),
              add_rn(rn_dot3(R[6], R[7], R[8], so), FP.s2w_t[2]));
    r.d = mk3(rn_dot3(R[0], R[1], R[2], sd), rn_dot3(R[3], R[4], R[5], sd), rn_dot3(R[6], R[7], R[8], sd));
    const float lo = -1e6f, hi = 1e6f, big = 3.4028234663852886e+38f;
    float tmin = (lo - r.o.x) / r.d.x, tmax = (hi - r.o.x) / r.d.x;
    if (tmin > tmax) swapf(tmin, tmax);
    float tymin = (lo - r.o.y) / r.d.y, tymax = (hi - r.o.y) / r.d.y;
    if (tymin > tymax) swapf(tymin, tymax);
    bool miss = (tmin > tymax) || (tymin > tmax);
    if (tymin > tmin) tmin = tymin;
    if (tymax < tmax) tmax = tymax;
    float tzmin = (lo - r.o.z) / r.d.z, tzmax = (hi - r.o.z) / r.d.z;
    if (tzmin > tzmax) swapf(tzmin, tzmax);
    miss = miss || (tmin > tzmax) || (tzmin > tmax);
    if (tzmin > tmin) tmin = tzmin;
    if (tzmax < tmax) tmax = tzmax;
    if (miss) { tmin = big; tmax = big; }
    r.tmin = fmaxf(tmin, 0.f);
    r.tmax = tmax;
    r.valid = r.tmax > r.tmin;
    return r;
}

// The pixel pair of a lane and the wave-level facts about its rays.
struct RayPair {
    p3 o, d;
    v2f tmin, tmax;
    bool valid0, valid1;
    bool inside0, inside1;
    int px, py0, py1;
    bool uniform_origin;  // every valid ray of the wave starts at `origin`
    f3 origin;
};
__device__ __forceinline__ RayPair init_ray_pair(const GutParams& P, const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                 uint32_t tile, uint32_t half, int lane) {
    RayPair rp;
    rp.px = (int)(tile % P.gx) * 16 + (lane & 15);
    rp.py0 = (int)(tile / P.gx) * 16 + (int)half * 8 + (lane >> 4);
    rp.py1 = rp.py0 + 4;
    const Ray a = init_ray(P, ray_o, ray_d, rp.px, rp.py0), b = init_ray(P, ray_o, ray_d, rp.px, rp.py1);
    rp.o = p3{v2f{a.o.x, b.o.x}, v2f{a.o.y, b.o.y}, v2f{a.o.z, b.o.z}};
    rp.d = p3{v2f{a.d.x, b.d.x}, v2f{a.d.y, b.d.y}, v2f{a.d.z, b.d.z}};
    rp.tmin = v2f{a.tmin, b.tmin};
    rp.tmax = v2f{a.tmax, b.tmax};
    rp.valid0 = a.valid;
    rp.valid1 = b.valid;
    rp.inside0 = a.inside;
    rp.inside1 = b.inside;
    // wave-uniform origin?  take the first valid ray as the candidate
    const unsigned long long m0 = __ballot(a.valid), m1 = __ballot(b.valid);
    f3 cand = mk3(0.f, 0.f, 0.f);
    if (m0) {
        const int src = __ffsll((long long)m0) - 1;
        cand = mk3(__shfl(a.o.x, src, 64), __shfl(a.o.y, src, 64), __shfl(a.o.z, src, 64));
    } else if (m1) {
        const int src = __ffsll((long long)m1) - 1;
        cand = mk3(__shfl(b.o.x, src, 64), __shfl(b.o.y, src, 64), __shfl(b.o.z, src, 64));
    }
    const bool same0 = !a.valid || (a.o.x == cand.x && a.o.y == cand.y && a.o.z == cand.z);
    const bool same1 = !b.valid || (b.o.x == cand.x && b.o.y == cand.y && b.o.z == cand.z);
    rp.uniform_origin = __all(same0 && same1);
    rp.origin = cand;
    return rp;
}

// block -> (virtual tile, half) with both halves of a tile on one XCD (block b runs on XCD b % 8)
// i -> (i * k') mod n with k' the first number >= k coprime to n: a bijection of [0, n) that sends neighbours far apart.  Launch
// order = memory order keeps the waves in flight on one band of the image, all heavy or all light at a time; a strided order mixes them.
__device__ __forceinline__ uint32_t stride_permute(uint32_t i, uint32_t n, uint32_t k) {
    if (n < 3u) return i;
    k %= n;
    if (k < 2u) k = 2u;
    while (true) {
        uint32_t a = k, b = n;
        while (b) { const uint32_t t = a % b; a = b; b = t; }
        if (a == 1u) break;
        ++k;
    }
    return (uint32_t)(((unsigned long long)i * k) % n);
}
__device__ __forceinline__ void half_mapping(uint32_t b, uint32_t& vtile, uint32_t& half) {
    const uint32_t xcd = b & 7u, slot = b >> 3;
    vtile = ((slot >> 1) << 3) + xcd;
    half = slot & 1u;
}

// ---------------------------------------------------------------------------------------------
// staged tile entry: 6 x float4 in LDS
//   r0 = M.r0, pos.x | r1 = M.r1, pos.y | r2 = M.r2, pos.z      M = diag(1/scale) R^T  (gaussianParticles.slang:96-110)
//   r3 = scale.xyz (fwd) or 1/scale.xyz (bwd), density
//   r4 = clamped radiance rgb, g_max
//   r5 = u0 = M (origin - pos) (uniform-origin waves), as_float(expansion position of the entry)
// Padding entries (index 0xFFFFFFFF) get M = I and g_max = 0: finite everywhere, never accepted.
// ---------------------------------------------------------------------------------------------
constexpr int kRecQuads = 6;

struct RawEntry {
    uint32_t idx, pos;   // particle, expansion position of the entry (its gradient slot)
    float4 a, q, s;
    f3 rgb;
};
// the sorted lists carry expansion positions; pos_particle maps them to particles (0xFFFFFFFF = padding)
// direct lists (rec64 != null, GutParams::rec64): the sorted payloads ARE the particles, one 64-byte record each; the gradient slot
// of an entry is the particle's part_offset (in the record) + the ordinal in the upper key bits
struct EntryLists {
    const uint32_t* __restrict__ sorted_pos;
    const uint32_t* __restrict__ pos_particle;
    const float4* __restrict__ rec64;
    const uint32_t* __restrict__ sorted_keys;
    uint32_t ord_shift;
};
__host__ __device__ inline EntryLists entry_lists(const GutParams& P, const uint32_t* sorted_pos, const uint32_t* pos_particle) {
    return EntryLists{sorted_pos, P.rec64 ? nullptr : pos_particle, P.rec64, P.sorted_keys, P.ord_shift};
}
template <bool WITH_POS = true>
__device__ __forceinline__ RawEntry load_entry(uint32_t e, uint32_t end, const EntryLists& lists,
                                               const float4* __restrict__ density12, const float* __restrict__ rgb) {
    RawEntry r;
    r.idx = 0xFFFFFFFFu;
    r.pos = 0u;
    r.a = r.q = r.s = make_float4(0.f, 0.f, 0.f, 0.f);
    r.rgb = mk3(0.f, 0.f, 0.f);
    if (e < end && lists.rec64) {
        r.idx = lists.sorted_pos[e];
        if (r.idx != 0xFFFFFFFFu) {
            const float4* rec = lists.rec64 + 4 * (size_t)r.idx;
            r.a = rec[0]; r.q = rec[1]; r.s = rec[2];
            const float4 c = rec[3];
            r.rgb = mk3(c.x, c.y, c.z);
            if (WITH_POS) r.pos = __float_as_uint(r.s.w) + (lists.sorted_keys[e] >> lists.ord_shift);
        }
    } else if (e < end) {
        r.pos = lists.sorted_pos[e];
        r.idx = lists.pos_particle[r.pos];
        if (r.idx != 0xFFFFFFFFu) {
            r.a = density12[3 * (size_t)r.idx + 0];
            r.q = density12[3 * (size_t)r.idx + 1];
            r.s = density12[3 * (size_t)r.idx + 2];
            if (rgb) r.rgb = mk3(rgb[3 * (size_t)r.idx], rgb[3 * (size_t)r.idx + 1], rgb[3 * (size_t)r.idx + 2]);
        }
    }
    return r;
}
// a loaded entry's ordinal among its particle's tile entries (gradient sweeps: GutGradSlots); padding = 0
__device__ __forceinline__ uint32_t entry_ordinal(const RawEntry& r, const EntryLists& lists, const uint32_t* __restrict__ part_offset) {
    if (r.idx == 0xFFFFFFFFu) return 0u;
    return r.pos - (lists.rec64 ? __float_as_uint(r.s.w) : part_offset[r.idx]);
}
// mark a written gradient slot: one bit of the particle's word for its first 32 tile entries (set by waves anywhere on the device:
// a return-less atomic OR), the slot's byte beyond
__device__ __forceinline__ void mark_slot(const GutGradSlots& slots, uint32_t particle, uint32_t ordinal, uint32_t half, size_t slot) {
    const uint32_t bit = 2u * ordinal + half;
    if (bit < kGutTouchBits) atomicOr(&slots.touched[particle], 1ull << bit);
    else slots.flag[slot] = 1;
}
template <int DEG, bool INVERSE_SCALE>
__device__ __forceinline__ void stage_entry(const GutParams& P, const RawEntry& r, bool uniform_origin, f3 origin, float4* __restrict__ rec) {
    float4 r0 = make_float4(1.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 1.f, 0.f, 0.f), r2 = make_float4(0.f, 0.f, 1.f, 0.f);
    float4 r3 = make_float4(1.f, 1.f, 1.f, 0.f), r4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 r5 = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xFFFFFFFFu));
    if (r.idx != 0xFFFFFFFFu) {
        const m3 rt = quat_wxyz_to_rotT(r.q.x, r.q.y, r.q.z, r.q.w);
        const float ix = __builtin_amdgcn_rcpf(r.s.x), iy = __builtin_amdgcn_rcpf(r.s.y), iz = __builtin_amdgcn_rcpf(r.s.z);
        r0 = make_float4(rt.r0.x * ix, rt.r0.y * ix, rt.r0.z * ix, r.a.x);
        r1 = make_float4(rt.r1.x * iy, rt.r1.y * iy, rt.r1.z * iy, r.a.y);
        r2 = make_float4(rt.r2.x * iz, rt.r2.y * iz, rt.r2.z * iz, r.a.z);
        r3 = INVERSE_SCALE ? make_float4(ix, iy, iz, r.a.w) : make_float4(r.s.x, r.s.y, r.s.z, r.a.w);
        const float need = fmaxf(P.min_response, P.min_alpha / r.a.w);   // response must exceed this
        const float gmax = (P.max_alpha > P.min_alpha && r.a.w > 0.f) ? response_gray_limit<DEG>(need) : 0.f;
        r4 = make_float4(fmaxf(r.rgb.x, 0.f), fmaxf(r.rgb.y, 0.f), fmaxf(r.rgb.z, 0.f), gmax);
        if (uniform_origin) {
            const f3 dl = origin - mk3(r.a.x, r.a.y, r.a.z);
            r5.x = dot(mk3(r0.x, r0.y, r0.z), dl);
            r5.y = dot(mk3(r1.x, r1.y, r1.z), dl);
            r5.z = dot(mk3(r2.x, r2.y, r2.z), dl);
        }
        r5.w = __uint_as_float(r.pos);
    }
    rec[0] = r0; rec[1] = r1; rec[2] = r2; rec[3] = r3; rec[4] = r4; rec[5] = r5;
}

// ---------------------------------------------------------------------------------------------
// Half-tile culling of staged entries (round 4).  A tile's list is binned for the 16x16 tile by the reference's 2-D test; the wave owns
// 16x8 of it, and 36 % of the entries a wave evaluates on the bench frame are accepted by none of its 128 pixels - each
// of them costs the pair geometry.  The accept test is a LINE - sphere test in the particle's canonical frame (|v x u|^2 < gmax |v|^2:
// the line through u along v passes the origin closer than r = sqrt(gmax)), so an entry whose sphere misses every line of the wave can
// be dropped when it is staged, and no result changes.  The lines of a wave are bounded, for ANY camera model, by the pyramid of its
// own rays: in a frame (a, e1, e2) around the first valid ray every ray is a + x e1 + y e2 up to scale, and the wave reduces
// [x0, x1] x [y0, y1] once.  M maps the pyramid's four faces to planes through u spanned by (M c, M e2) / (M c, M e1) with c a corner
// direction; det[M c, M e1, M e2] = det M > 0 fixes which side is out.  The lines also extend BEHIND the apex; that mirror pyramid lies
// behind the plane through u with normal M e1 x M e2 (the image of the camera plane normal to a), so the entry is dropped only if its
// sphere is wholly in front of that plane and wholly outside one face.  All comparisons carry r' = 1.001 r + 1e-5 |u| (the accept test
// and these triple products both cancel to ~1e-7 |u|).
// ---------------------------------------------------------------------------------------------
struct WavePyramid {
    bool on;          // wave-uniform: the bound exists (>= 1 valid ray, every ray within 60 degrees of the first)
    f3 c00, e1, e2;   // corner direction a + x0 e1 + y0 e2 and the frame's tangents
    float dx, dy;     // x1 - x0, y1 - y0
};
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float uniform(float v) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v))); }
// (up to two rays per lane: the pixel pair of the half-tile waves, one ray of the quarter-tile waves with valid1 = false)
__device__ __forceinline__ WavePyramid wave_pyramid(bool valid0, f3 d0, bool valid1, f3 d1) {
    WavePyramid w;
    w.on = false;
    w.c00 = w.e1 = w.e2 = mk3(0.f, 0.f, 0.f);
    w.dx = w.dy = 0.f;
    const unsigned long long m0 = __ballot(valid0), m1 = __ballot(valid1);
    if (!(m0 | m1)) return w;
    f3 a;
    if (m0) { const int src = __ffsll((long long)m0) - 1; a = mk3(__shfl(d0.x, src, 64), __shfl(d0.y, src, 64), __shfl(d0.z, src, 64)); }
    else { const int src = __ffsll((long long)m1) - 1; a = mk3(__shfl(d1.x, src, 64), __shfl(d1.y, src, 64), __shfl(d1.z, src, 64)); }
    a = a * __builtin_amdgcn_rsqf(dot(a, a));
    a = mk3(uniform(a.x), uniform(a.y), uniform(a.z));
    // any unit tangent pair: e1 = a x (the axis a is least aligned with), e2 = a x e1
    const float ax = fabsf(a.x), ay = fabsf(a.y), az = fabsf(a.z);
    const f3 k = (ax <= ay && ax <= az) ? mk3(1.f, 0.f, 0.f) : (ay <= az ? mk3(0.f, 1.f, 0.f) : mk3(0.f, 0.f, 1.f));
    f3 e1 = cross(a, k);
    e1 = e1 * __builtin_amdgcn_rsqf(dot(e1, e1));
    const f3 e2 = cross(a, e1);
    const float q0 = dot(d0, a), q1 = dot(d1, a);
    const float l0 = __builtin_amdgcn_sqrtf(dot(d0, d0)), l1 = __builtin_amdgcn_sqrtf(dot(d1, d1));
    const bool ok0 = !valid0 || q0 > 0.5f * l0, ok1 = !valid1 || q1 > 0.5f * l1;
    if (!__all(ok0 && ok1)) return w;
    const float big = 3.0e38f;
    const float i0 = 1.f / q0, i1 = 1.f / q1;
    const float x_0 = dot(d0, e1) * i0, y_0 = dot(d0, e2) * i0, x_1 = dot(d1, e1) * i1, y_1 = dot(d1, e2) * i1;
    const float xlo = wave_min(fminf(valid0 ? x_0 : big, valid1 ? x_1 : big)), xhi = -wave_min(fminf(valid0 ? -x_0 : big, valid1 ? -x_1 : big));
    const float ylo = wave_min(fminf(valid0 ? y_0 : big, valid1 ? y_1 : big)), yhi = -wave_min(fminf(valid0 ? -y_0 : big, valid1 ? -y_1 : big));
    const float pad = 1e-6f;   // tangent units (a pixel is ~1e-3): the rounding of x, y themselves
    const float x0 = uniform(xlo) - pad, x1 = uniform(xhi) + pad, y0 = uniform(ylo) - pad, y1 = uniform(yhi) + pad;
    w.on = true;
    w.c00 = a + e1 * x0 + e2 * y0;
    w.e1 = mk3(uniform(e1.x), uniform(e1.y), uniform(e1.z));
    w.e2 = mk3(uniform(e2.x), uniform(e2.y), uniform(e2.z));
    w.c00 = mk3(uniform(w.c00.x), uniform(w.c00.y), uniform(w.c00.z));
    w.dx = x1 - x0;
    w.dy = y1 - y0;
    return w;
}
__device__ __forceinline__ WavePyramid wave_pyramid(const RayPair& rp) {
    return wave_pyramid(rp.valid0, mk3(rp.d.x.x, rp.d.y.x, rp.d.z.x), rp.valid1, mk3(rp.d.x.y, rp.d.y.y, rp.d.z.y));
}
// does the staged record's sphere miss every line of the wave?  (rec as stage_entry builds it, uniform-origin form: r5.xyz = u)
__device__ __forceinline__ bool pyramid_misses(const WavePyramid& w, float4 r0, float4 r1, float4 r2, float gmax, float4 r5) {
    const f3 m0 = mk3(r0.x, r0.y, r0.z), m1 = mk3(r1.x, r1.y, r1.z), m2 = mk3(r2.x, r2.y, r2.z);
    const f3 u = mk3(r5.x, r5.y, r5.z);
    const f3 v00 = mk3(dot(m0, w.c00), dot(m1, w.c00), dot(m2, w.c00));
    const f3 f1 = mk3(dot(m0, w.e1), dot(m1, w.e1), dot(m2, w.e1)), f2 = mk3(dot(m0, w.e2), dot(m1, w.e2), dot(m2, w.e2));
    const f3 v10 = v00 + f1 * w.dx, v01 = v00 + f2 * w.dy;
    const float rr = 1.001f * __builtin_amdgcn_sqrtf(gmax) + 1e-5f * __builtin_amdgcn_sqrtf(dot(u, u));
    const float r2lim = rr * rr;
    // signed distance of the sphere's centre (the origin) OUT of the face, times |n|:  s = -(u . n_out)
    const f3 nx0 = cross(v00, f2), nx1 = cross(v10, f2), ny0 = cross(v00, f1), ny1 = cross(v01, f1), wf = cross(f1, f2);
    const float sx0 = -dot(u, nx0), sx1 = dot(u, nx1), sy0 = dot(u, ny0), sy1 = -dot(u, ny1), sf = -dot(u, wf);
    const bool front = sf > 0.f && sf * sf > r2lim * dot(wf, wf);
    const bool out = (sx0 > 0.f && sx0 * sx0 > r2lim * dot(nx0, nx0)) || (sx1 > 0.f && sx1 * sx1 > r2lim * dot(nx1, nx1)) ||
                     (sy0 > 0.f && sy0 * sy0 > r2lim * dot(ny0, ny0)) || (sy1 > 0.f && sy1 * sy1 > r2lim * dot(ny1, ny1));
    return front && out;
}

// canonical-frame ray of the pixel pair against one staged entry, and the accept test
struct PairGeom {
    p3 u, v;        // canonical origin, canonical (un-normalised) direction
    p3 c;           // v x u (the SH gradient sweep rebuilds the closest point's offset from it)
    v2f l2, cc;     // |v|^2, |v x u|^2  (grayDist = cc / l2)
    bool acc0, acc1;
};
template <bool UNI>
__device__ __forceinline__ PairGeom pair_geometry(const RayPair& rp, const float4* __restrict__ rec) {
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    PairGeom g;
    const f3 m0 = mk3(r0.x, r0.y, r0.z), m1 = mk3(r1.x, r1.y, r1.z), m2 = mk3(r2.x, r2.y, r2.z);
    g.v = p3{pdot(m0, rp.d), pdot(m1, rp.d), pdot(m2, rp.d)};
    if (UNI) {
        const float4 r5 = rec[5];
        g.u = p3{splat(r5.x), splat(r5.y), splat(r5.z)};
    } else {
        const p3 dl = p3{rp.o.x - r0.w, rp.o.y - r1.w, rp.o.z - r2.w};
        g.u = p3{pdot(m0, dl), pdot(m1, dl), pdot(m2, dl)};
    }
    g.l2 = pdot(g.v, g.v);
    g.c = pcross(g.v, g.u);
    g.cc = pdot(g.c, g.c);
    const v2f lim = rec[4].w * g.l2;
    g.acc0 = g.cc.x < lim.x;
    g.acc1 = g.cc.y < lim.y;
    return g;
}

// particle_response<DEG> for a pixel pair (one v_exp_f32 per pixel, the polynomial part packed)
template <int DEG>
__device__ __forceinline__ v2f pair_response(v2f g) {
    constexpr float kLog2e = 1.4426950408889634f;
    if constexpr (DEG == 2) {
        const v2f e = g * (-0.5f * kLog2e);
        return v2f{__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
    } else if constexpr (DEG == 4) {
        const v2f e = (g * g) * (-0.0555555555556f * kLog2e);
        return v2f{__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
    } else {
        return v2f{particle_response<DEG>(g.x), particle_response<DEG>(g.y)};
    }
}

// the [H,W,4] image: fp32, or IEEE half with FEATURE_OUTPUT_HALF (rayPayload.cuh:176-186 writes __float2half of every component;
// rayPayloadBackward.cuh:50-58 reads them back)
__device__ __forceinline__ void store_fd(const GutParams& P, float4* __restrict__ out_fd, size_t pix, float4 o) {
    if (P.out_half) {
        __half* h = reinterpret_cast<__half*>(out_fd) + 4 * pix;
        h[0] = __float2half(o.x); h[1] = __float2half(o.y); h[2] = __float2half(o.z); h[3] = __float2half(o.w);
    } else {
        out_fd[pix] = o;
    }
}
__device__ __forceinline__ float4 load_fd(const GutParams& P, const float4* __restrict__ fd, size_t pix) {
    if (P.out_half) {
        const __half* h = reinterpret_cast<const __half*>(fd) + 4 * pix;
        return make_float4(__half2float(h[0]), __half2float(h[1]), __half2float(h[2]), __half2float(h[3]));
    }
    return fd[pix];
}
// the plugin's `pred_features` / `pred_opacity` as contiguous tensors of their own (GutFrame::out_features / out_opacity)
__device__ __forceinline__ void write_split_outputs(const GutParams& P, size_t pix, float4 o) {
    if (P.out_features) { P.out_features[3 * pix] = o.x; P.out_features[3 * pix + 1] = o.y; P.out_features[3 * pix + 2] = o.z; }
    if (P.out_opacity) P.out_opacity[pix] = o.w;
}

// ---------------------------------------------------------------------------------------------
// The sorted hit buffer (K > 0), shared by gut_render_k_body and the feature kernel behind the buffer (gut_render_nht_k_kernel): run-time
// degree dispatch of the response, the hit distance in the checker's operation order (the buffer's sort key) and the buffer itself.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float gray_limit_rt(int deg, float x) {
    switch (deg) {
    case 8: return response_gray_limit<8>(x);
    case 5: return response_gray_limit<5>(x);
    case 4: return response_gray_limit<4>(x);
    case 3: return response_gray_limit<3>(x);
    case 1: return response_gray_limit<1>(x);
    case 0: return response_gray_limit<0>(x);
    default: return response_gray_limit<2>(x);
    }
}
__device__ __forceinline__ float response_rt(int deg, float g) {
    switch (deg) {
    case 8: return particle_response<8>(g);
    case 5: return particle_response<5>(g);
    case 4: return particle_response<4>(g);
    case 3: return particle_response<3>(g);
    case 1: return particle_response<1>(g);
    case 0: return particle_response<0>(g);
    default: return particle_response<2>(g);
    }
}
__device__ __forceinline__ float response_grd_rt(int deg, float g, float gres, float gresGrd) {
    switch (deg) {
    case 8: return particle_response_grd<8>(g, gres, gresGrd);
    case 5: return particle_response_grd<5>(g, gres, gresGrd);
    case 4: return particle_response_grd<4>(g, gres, gresGrd);
    case 3: return particle_response_grd<3>(g, gres, gresGrd);
    case 1: return particle_response_grd<1>(g, gres, gresGrd);
    case 0: return particle_response_grd<0>(g, gres, gresGrd);
    default: return particle_response_grd<2>(g, gres, gresGrd);
    }
}

// Sorted mode: the k-buffer ORDERS a ray's hits by their fp32 hit distance, so two implementations agree on the order only if they agree on
// the distance's bits.  The hit distance of an accepted hit is therefore evaluated in the CHECKER's operation order (the checker's gut_oracle.c:
// density_hit_ex, itself the source order of gaussianParticles.slang:96-110, 181-190): every product and sum rounded on its own, correctly
// rounded 1/x and sqrt - ~70 instructions per ACCEPTED hit on top of the accept test, which keeps the fast pre-transformed form (its flips
// are identified per pixel by the parity tests; an order tie could not be).  rt* = rows of R^T from the quaternion, gis = 1 / scale.
__device__ __forceinline__ float sub_rn(float a, float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ void rn_rotT(float r, float x, float y, float z, f3& r0, f3& r1, f3& r2) {   // quat_wxyz_to_rotT, uncontracted
    const float xx = mul_rn(x, x), yy = mul_rn(y, y), zz = mul_rn(z, z), xy = mul_rn(x, y), xz = mul_rn(x, z), yz = mul_rn(y, z);
    const float rx = mul_rn(r, x), ry = mul_rn(r, y), rz = mul_rn(r, z);
    r0 = mk3(sub_rn(1.f, mul_rn(2.f, add_rn(yy, zz))), mul_rn(2.f, add_rn(xy, rz)), mul_rn(2.f, sub_rn(xz, ry)));
    r1 = mk3(mul_rn(2.f, sub_rn(xy, rz)), sub_rn(1.f, mul_rn(2.f, add_rn(xx, zz))), mul_rn(2.f, add_rn(yz, rx)));
    r2 = mk3(mul_rn(2.f, add_rn(xz, ry)), mul_rn(2.f, sub_rn(yz, rx)), sub_rn(1.f, mul_rn(2.f, add_rn(xx, yy))));
}
__device__ __forceinline__ float oracle_order_hit_t(const Ray& ray, f3 pos, f3 scl, f3 rt0, f3 rt1, f3 rt2, f3 gis) {
    const f3 gposc = mk3(sub_rn(ray.o.x, pos.x), sub_rn(ray.o.y, pos.y), sub_rn(ray.o.z, pos.z));
    const f3 gro = mk3(mul_rn(gis.x, rn_dot3(rt0, gposc)), mul_rn(gis.y, rn_dot3(rt1, gposc)), mul_rn(gis.z, rn_dot3(rt2, gposc)));
    const f3 grdu = mk3(mul_rn(gis.x, rn_dot3(rt0, ray.d)), mul_rn(gis.y, rn_dot3(rt1, ray.d)), mul_rn(gis.z, rn_dot3(rt2, ray.d)));
    const float inv = 1.f / sqrtf(rn_dot3(grdu, grdu));            // (IEEE division and square root: neither unit is built with fast-math)
    const f3 grd = mk3(mul_rn(grdu.x, inv), mul_rn(grdu.y, inv), mul_rn(grdu.z, inv));
    const float along = rn_dot3(grd, mk3(-gro.x, -gro.y, -gro.z));
    const f3 grds = mk3(mul_rn(scl.x, mul_rn(grd.x, along)), mul_rn(scl.y, mul_rn(grd.y, along)), mul_rn(scl.z, mul_rn(grd.z, along)));
    return sqrtf(rn_dot3(grds, grds));
}

template <int K>
struct KBuffer {   // ascending in hitT: slot 0 = nearest pending hit, empty slots hold hitT = -1 at the front
    float hitT[K], alpha[K];
    uint32_t idx[K];
    int num;
    __device__ __forceinline__ void clear() {
        num = 0;
#pragma unroll
        for (int i = 0; i < K; ++i) { hitT[i] = -1.f; alpha[i] = 0.f; idx[i] = 0xFFFFFFFFu; }
    }
    // HitParticleKBufferT::insert (:76-91); the caller has already consumed slot 0 when the buffer was full
    // branch-free: the keys move with min / max (no swap on equal keys, like the reference's strict `>`), the payloads
    // with selects
    __device__ __forceinline__ void insert(float t, float a, uint32_t id) {
#pragma unroll
        for (int i = K - 1; i >= 0; --i) {
            const bool up = t > hitT[i];
            const float lo = fminf(t, hitT[i]), hi = fmaxf(t, hitT[i]);
            const float aa = up ? alpha[i] : a;
            const uint32_t ii = up ? idx[i] : id;
            alpha[i] = up ? a : alpha[i];
            idx[i] = up ? id : idx[i];
            hitT[i] = hi;
            t = lo; a = aa; id = ii;
        }
    }
};

// gradient of sum_ij (b_i e_j) rotT_ij(q) w.r.t. q = (r,x,y,z)  (matmul_bw_quat, mathUtils.cuh:458-521)
__device__ __forceinline__ float4 quat_outer_contract(f3 b, f3 e, float4 q) {
    const float r = 2.f * q.x, x = 2.f * q.y, y = 2.f * q.z, z = 2.f * q.w;
    const float m00 = b.x * e.x, m01 = b.x * e.y, m02 = b.x * e.z, m10 = b.y * e.x, m11 = b.y * e.y, m12 = b.y * e.z, m20 = b.z * e.x,
                m21 = b.z * e.y, m22 = b.z * e.z;
    const float s01 = m01 + m10, s02 = m02 + m20, s12 = m12 + m21, a01 = m01 - m10, a02 = m20 - m02, a12 = m12 - m21;
    return make_float4(z * a01 + y * a02 + x * a12, y * s01 + z * s02 + r * a12 - 2.f * x * (m11 + m22),
                       x * s01 + z * s12 + r * a02 - 2.f * y * (m00 + m22), x * s02 + y * s12 + r * a01 - 2.f * z * (m00 + m11));
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// launch grids and dispatch (host)
// ---------------------------------------------------------------------------------------------
static uint32_t half_grid(const GutParams& P) {
    const uint32_t tiles = (uint32_t)(P.gx * P.gy);
    return ((tiles + 7u) & ~7u) * 2u;
}
// tile-first segments + one task set per segment boundary, padded to the 8-XCD interleave
static uint32_t segment_grid(const GutParams& P, uint32_t num_boundaries) {
    const uint32_t tiles = (uint32_t)(P.gx * P.gy);
    const uint32_t vtiles = ((tiles + 7u) & ~7u) + ((num_boundaries + 7u) & ~7u);
    return vtiles * 2u;
}

#define GRUT_DISPATCH_DEGREE(DEG, ...)                         \
    switch (DEG) {                                             \
    case 0: { constexpr int D_ = 0; __VA_ARGS__; } break;      \
    case 1: { constexpr int D_ = 1; __VA_ARGS__; } break;      \
    case 3: { constexpr int D_ = 3; __VA_ARGS__; } break;      \
    case 4: { constexpr int D_ = 4; __VA_ARGS__; } break;      \
    case 5: { constexpr int D_ = 5; __VA_ARGS__; } break;      \
    case 8: { constexpr int D_ = 8; __VA_ARGS__; } break;      \
    default: { constexpr int D_ = 2; __VA_ARGS__; } break;     \
    }

static uint32_t strip_grid(const GutParams& P) {
    const uint32_t tiles = (uint32_t)(P.gx * P.gy);
    return ((tiles + 7u) & ~7u) * 4u;
}
#define GRUT_DISPATCH_K(KK, ...)                               \
    switch (KK) {                                              \
    case 4: { constexpr int K_ = 4; __VA_ARGS__; } break;      \
    case 8: { constexpr int K_ = 8; __VA_ARGS__; } break;      \
    default: { constexpr int K_ = 16; __VA_ARGS__; } break;    \
    }

}  // namespace grut
