// gut_render_k.hip - 3DGUT compositing through the sorted hit buffer (K > 0) with SH radiance.  A translation unit of its own: these kernels
// are built with the backend's default scheduling strategy, the unsorted sweeps of gut_render.hip with max-ILP (3dgrut_amd/build.py).
//
// K > 0 ("sorted") compositing — HitParticleKBufferT<K> + evalKBuffer (gutKBufferRenderer.cuh:62-122, 273-352) and its
// backward processHitParticle<Backward> (:158-198; Slang reverse mode of the back-to-front lerp form,
// shRadiativeParticles.slang:210-256, gaussianParticles.slang:420-479).
// Every pixel keeps the K nearest pending hits (by hitT) in registers and composites the nearest one when the buffer is
// full, so neighbouring pixels pop DIFFERENT particles at the same step: there is nothing to reduce across the wave, and
// the gradient is accumulated per hit with atomics exactly like the reference does in this mode.  One pixel per lane,
// one wave64 per 16x4 strip; correctness-first kernel (the unsorted K = 0 path of gut_render.hip is the tuned one).
#include "gut_render_common.inl"

namespace grut {

namespace {

struct KFwdState {
    float T, D, Cr, Cg, Cb, cnt;
};
struct KBwdState {
    float T;                 // forward running transmittance (termination only)
    float Tb, Db, gT, gD;    // "behind" values and running upstream gradients
    f3 Cb, gC;
};

__device__ __forceinline__ void k_process_fwd(const GutParams& P, const float* __restrict__ rgb, float hitT, float alpha, uint32_t idx,
                                              KFwdState& s, bool& alive) {
    const float w = alpha * s.T;
    s.D = fmaf(hitT, w, s.D);
    s.T *= (1.f - alpha);
    if (w > 0.f) {
        s.Cr = fmaf(fmaxf(rgb[3 * (size_t)idx], 0.f), w, s.Cr);
        s.Cg = fmaf(fmaxf(rgb[3 * (size_t)idx + 1], 0.f), w, s.Cg);
        s.Cb = fmaf(fmaxf(rgb[3 * (size_t)idx + 2], 0.f), w, s.Cb);
        s.cnt += 1.f;
    }
    if (s.T < P.min_transmittance) alive = false;
}

// One hit of one pixel in the sorted mode's backward: updates the running state and returns the hit's 14 gradient terms
// (position 0-2, density 3, quaternion 4-7, scale 8-10, rgb 11-13) instead of adding them to memory; `k_bwd_flush` adds
// them wave by wave.  Returns whether the hit contributed.
__device__ __forceinline__ bool k_bwd_terms(const GutParams& P, const Ray& ray, const float4* __restrict__ density12, const float* __restrict__ rgb,
                                            float hitT, float alpha, uint32_t idx, KBwdState& s, bool& alive, float (&terms)[16]) {
    const bool contributes = alpha > 0.f;
    if (contributes) {
        const float w = __builtin_amdgcn_rcpf(1.f - alpha);
        const f3 feat = mk3(fmaxf(rgb[3 * (size_t)idx], 0.f), fmaxf(rgb[3 * (size_t)idx + 1], 0.f), fmaxf(rgb[3 * (size_t)idx + 2], 0.f));
        s.Cb = (s.Cb - feat * alpha) * w;
        float dalpha = (feat.x - s.Cb.x) * s.gC.x + (feat.y - s.Cb.y) * s.gC.y + (feat.z - s.Cb.z) * s.gC.z;
        terms[11] = alpha * s.gC.x; terms[12] = alpha * s.gC.y; terms[13] = alpha * s.gC.z;
        s.gC = s.gC * (1.f - alpha);
        s.Tb *= w;
        s.Db = (s.Db - hitT * alpha) * w;
        dalpha += (hitT - s.Db) * s.gD - s.Tb * s.gT;
        const float ddepth = alpha * s.gD;
        s.gD *= (1.f - alpha);
        s.gT *= (1.f - alpha);

        const float4 a = density12[3 * (size_t)idx], q = density12[3 * (size_t)idx + 1], sc = density12[3 * (size_t)idx + 2];
        const m3 rotT = quat_wxyz_to_rotT(q.x, q.y, q.z, q.w);
        const f3 gscl = mk3(sc.x, sc.y, sc.z), giscl = mk3(__builtin_amdgcn_rcpf(sc.x), __builtin_amdgcn_rcpf(sc.y), __builtin_amdgcn_rcpf(sc.z));
        const f3 gposc = ray.o - mk3(a.x, a.y, a.z);
        const f3 gposcr = mul_rows(rotT, gposc);
        const f3 gro = giscl * gposcr;
        const f3 rdr = mul_rows(rotT, ray.d);
        const f3 grdu = giscl * rdr;
        const float l2 = dot(grdu, grdu);
        const float il = __builtin_amdgcn_rsqf(l2);
        const f3 grd = grdu * il;
        const f3 gcrod = cross(grd, gro);
        const float gray = dot(gcrod, gcrod);
        const float gres = response_rt(P.degree, gray);
        float dres = 0.f, ddens = 0.f;  // reverse mode of min(MaxAlpha, .): only the smaller argument receives the gradient
        if (gres * a.w < P.max_alpha) { dres = a.w * dalpha; ddens = gres * dalpha; }
        const float grayGrd = response_grd_rt(P.degree, gray, gres, dres);
        const float pdot = -dot(grd, gro);
        const f3 grdd = grd * pdot;
        const f3 grds = gscl * grdd;
        const float gsq = dot(grds, grds);
        const float gdist = __builtin_amdgcn_sqrtf(gsq);
        const f3 grdsGrd = gsq > 0.f ? grds * (ddepth * __builtin_amdgcn_rcpf(gdist)) : mk3(0.f, 0.f, 0.f);
        const f3 gsclHit = grdd * grdsGrd;
        const float sdot = dot(grdsGrd * gscl, grd);
        const f3 grdHit = gscl * grdsGrd * pdot - gro * sdot;
        const f3 groHit = grd * (-sdot);
        const f3 gcrodGrd = gcrod * (2.f * grayGrd);
        const f3 grdGrd = mk3(gcrodGrd.z * gro.y - gcrodGrd.y * gro.z, gcrodGrd.x * gro.z - gcrodGrd.z * gro.x, gcrodGrd.y * gro.x - gcrodGrd.x * gro.y);
        const f3 groGrd = mk3(gcrodGrd.y * grd.z - gcrodGrd.z * grd.y, gcrodGrd.z * grd.x - gcrodGrd.x * grd.z, gcrodGrd.x * grd.y - gcrodGrd.y * grd.x);
        const f3 groTot = groGrd + groHit;
        const f3 is2 = giscl * giscl;
        const f3 gsclGro = mk3(-gposcr.x * is2.x, -gposcr.y * is2.y, -gposcr.z * is2.z) * groTot;
        const f3 gposcrGrd = giscl * groTot;
        const f3 gposcGrd = mul_cols(rotT, gposcrGrd);
        const f3 dn = grdGrd + grdHit;
        const f3 grduGrd = dn * il - grdu * (il * il * il * dot(dn, grdu));   // normalize backward
        const f3 sclGrd = gsclHit + gsclGro + mk3(-rdr.x * is2.x, -rdr.y * is2.y, -rdr.z * is2.z) * grduGrd;
        const float4 gq1 = quat_outer_contract(gposcrGrd, gposc, q), gq2 = quat_outer_contract(giscl * grduGrd, ray.d, q);
        terms[0] = -gposcGrd.x; terms[1] = -gposcGrd.y; terms[2] = -gposcGrd.z; terms[3] = ddens;
        terms[4] = gq1.x + gq2.x; terms[5] = gq1.y + gq2.y; terms[6] = gq1.z + gq2.z; terms[7] = gq1.w + gq2.w;
        terms[8] = sclGrd.x; terms[9] = sclGrd.y; terms[10] = sclGrd.z;
    }
    s.T *= (1.f - alpha);
    if (s.T < P.min_transmittance) alive = false;
    return contributes;
}
// Adds the terms of the lanes with `have` to the gradient buffers: lanes that processed the SAME particle in this step
// (neighbouring pixels usually do) are summed with a DPP reduce-scatter first, one set of 14 atomics per (wave, particle)
// instead of one per (pixel, particle) — the reference's per-hit atomics (gutKBufferRenderer.cuh:158-198) cost this path
// 147 ms per 1080p frame on MI355X.  (A further level — a per-wave LDS cache of per-particle totals across steps, evicted
// to memory — was measured and dropped: 8.0 -> 9.6 ms; the atomics are not what bounds this kernel.)
__device__ __forceinline__ void k_bwd_flush(bool have, uint32_t idx, const float (&terms)[16], int lane, float* __restrict__ g_density12,
                                            float* __restrict__ g_rgb) {
    unsigned long long m = __ballot(have);
    while (m) {
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t pid = (uint32_t)__builtin_amdgcn_readlane((int)idx, leader);
        const bool part = have && (idx == pid);
        float t[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) t[k] = (part && k < 14) ? terms[k] : 0.f;
        const float tot = wave_reduce_scatter16(t, lane);
        if (lane < 11) atomicAdd(g_density12 + 12 * (size_t)pid + lane, tot);
        else if (lane < 14) atomicAdd(g_rgb + 3 * (size_t)pid + (lane - 11), tot);
        m &= ~__ballot(part);
    }
}

// Round 5: the same sums through LDS instead of the DPP reduce-scatter (GRUT_K_FLUSH_LDS, default on).  A step's popping lanes hold
// DIFFERENT particles more often than not (a pop is an OLD pending hit; neighbouring pixels' buffers drift apart), so the loop above runs
// once per distinct particle at ~100 instructions each (16 selects + the 30-step reduce-scatter + the atomics).  Here every popping lane
// parks its 14 terms in LDS (stride 15: conflict-free both ways) and lanes 0..13 ARE the 14 words of a particle's gradient: per distinct
// particle the members' words are added from LDS (one read + one add per member) and leave as ONE atomic instruction - the hit-major
// transposition of the 3DGRT replay backward (grt_replay_bwd_kernel).
#ifndef GRUT_K_FLUSH_LDS
#define GRUT_K_FLUSH_LDS 1
#endif
#ifndef GRUT_K_FLUSH_MINK
#define GRUT_K_FLUSH_MINK 8    // smallest K that takes the LDS flush and the three-waves allocation that goes with it (K = 4 runs three waves
                               // on the DPP reduce-scatter already; measured at 1 M / 1080p, step: K = 16 11.89 -> 10.90 ms, K = 8 8.89 -> 8.41 ms)
#endif
constexpr int kKTermStride = 15;
__device__ __forceinline__ void k_bwd_flush_lds(bool have, uint32_t idx, const float (&terms)[16], int lane, float* __restrict__ s_terms,
                                                float* __restrict__ g_density12, float* __restrict__ g_rgb) {
    if (have) {
#pragma unroll
        for (int k = 0; k < 14; ++k) s_terms[lane * kKTermStride + k] = terms[k];
    }
    __syncthreads();   // single-wave workgroup: orders the LDS hand-off
    unsigned long long m = __ballot(have);
    float* const row = lane < 11 ? g_density12 + lane : g_rgb + (lane < 14 ? lane - 11 : 0);
    const uint32_t stride = lane < 11 ? 12u : 3u;
    while (m) {
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t pid = (uint32_t)__builtin_amdgcn_readlane((int)idx, leader);
        unsigned long long same = __ballot(have && idx == pid);
        m &= ~same;
        float v = 0.f;
        while (same) {
            const int s2 = __ffsll((long long)same) - 1;
            same &= same - 1;
            v += s_terms[s2 * kKTermStride + (lane < 14 ? lane : 0)];
        }
        if (lane < 14 && v != 0.f) atomicAdd(row + (size_t)pid * stride, v);
    }
    __syncthreads();   // the next step overwrites s_terms.  (Two buffers used alternately - one barrier per step - were measured SLOWER: 15.9 KB of
                       // LDS per wave leave room for 10 waves per CU, i.e. two per SIMD again: backward 9.5 instead of 7.6 ms.)
}

template <int K, bool BWD>
__device__ __forceinline__ void gut_render_k_body(const GutParams& P, const uint2* __restrict__ ranges, const EntryLists& lists,
                                                  const float4* __restrict__ density12, const float* __restrict__ rgb,
                                                  const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                  float4* __restrict__ out_fd, float* __restrict__ out_dist, float* __restrict__ out_cnt,
                                                  const float4* __restrict__ g_fd, const float* __restrict__ g_dist,
                                                  float* __restrict__ g_density12, float* __restrict__ g_rgb) {
    constexpr int kQ = 8;   // quads per staged entry: 0-2 M rows | pos, 3 scale | density, 4 particle | accept limit, 5-7 rows of R^T | 1 / scale
    __shared__ float4 s_rec[64 * kQ];
    constexpr bool kLdsFlush = BWD && GRUT_K_FLUSH_LDS && K >= GRUT_K_FLUSH_MINK;
    __shared__ float s_kterms[kLdsFlush ? 64 * kKTermStride : 1];
    // strip -> (tile, strip-in-tile) with all four strips of a tile on one XCD
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const uint32_t tile = ((slot >> 2) << 3) + xcd, strip = slot & 3u;
    if (tile >= (uint32_t)(P.gx * P.gy)) return;
    const int lane = threadIdx.x;
    const int px = (int)(tile % P.gx) * 16 + (lane & 15);
    const int py = (int)(tile / P.gx) * 16 + (int)strip * 4 + (lane >> 4);
    const Ray ray = init_ray(P, ray_o, ray_d, px, py);
    bool alive = ray.valid;
    const size_t pix = ray.valid ? (size_t)py * P.W + px : 0;
    KFwdState fs{1.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    KBwdState bs;
    bs.T = 1.f; bs.Tb = 0.f; bs.Db = 0.f; bs.gT = 0.f; bs.gD = 0.f; bs.Cb = mk3(0.f, 0.f, 0.f); bs.gC = mk3(0.f, 0.f, 0.f);
    if (BWD && alive) {   // initializeBackwardRay (rayPayloadBackward.cuh:30-73); out_* hold the forward results here
        const float4 f = load_fd(P, out_fd, pix), g = g_fd[pix];
        bs.Cb = mk3(f.x, f.y, f.z); bs.gC = mk3(g.x, g.y, g.z);
        bs.Tb = 1.f - f.w; bs.gT = -g.w;
        bs.Db = out_dist[pix]; bs.gD = g_dist ? g_dist[pix] : 0.f;
    }
    KBuffer<K> kb;
    kb.clear();
    const uint2 range = ranges[tile];
    for (uint32_t b = range.x; b < range.y; b += 64) {
        if (!__any(alive)) break;
        {   // stage up to 64 entries
            const RawEntry e = load_entry(b + lane, range.y, lists, density12, rgb);
            float4 r0 = make_float4(1.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 1.f, 0.f, 0.f), r2 = make_float4(0.f, 0.f, 1.f, 0.f);
            float4 r3 = make_float4(1.f, 1.f, 1.f, 0.f), r4 = make_float4(__uint_as_float(0xFFFFFFFFu), 0.f, 0.f, 0.f);
            float4 r5 = r0, r6 = r1, r7 = r2;
            if (e.idx != 0xFFFFFFFFu) {
                {   // the hit-distance inputs in the checker's operation order (oracle_order_hit_t)
                    f3 t0, t1, t2;
                    rn_rotT(e.q.x, e.q.y, e.q.z, e.q.w, t0, t1, t2);
                    r5 = make_float4(t0.x, t0.y, t0.z, 1.f / e.s.x);
                    r6 = make_float4(t1.x, t1.y, t1.z, 1.f / e.s.y);
                    r7 = make_float4(t2.x, t2.y, t2.z, 1.f / e.s.z);
                }
                const m3 rt = quat_wxyz_to_rotT(e.q.x, e.q.y, e.q.z, e.q.w);
                const float ix = __builtin_amdgcn_rcpf(e.s.x), iy = __builtin_amdgcn_rcpf(e.s.y), iz = __builtin_amdgcn_rcpf(e.s.z);
                r0 = make_float4(rt.r0.x * ix, rt.r0.y * ix, rt.r0.z * ix, e.a.x);
                r1 = make_float4(rt.r1.x * iy, rt.r1.y * iy, rt.r1.z * iy, e.a.y);
                r2 = make_float4(rt.r2.x * iz, rt.r2.y * iz, rt.r2.z * iz, e.a.z);
                r3 = make_float4(e.s.x, e.s.y, e.s.z, e.a.w);
                r4.x = __uint_as_float(e.idx);
                // accept test on grayDist itself, as in the unsorted sweeps (stage_entry)
                const float need = fmaxf(P.min_response, P.min_alpha / e.a.w);
                r4.y = (P.max_alpha > P.min_alpha && e.a.w > 0.f) ? gray_limit_rt(P.degree, need) : 0.f;
            }
            float4* rec = &s_rec[lane * kQ];
            rec[0] = r0; rec[1] = r1; rec[2] = r2; rec[3] = r3; rec[4] = r4; rec[5] = r5; rec[6] = r6; rec[7] = r7;
        }
        __syncthreads();
        const int n = (int)min(64u, range.y - b);
        for (int j = 0; j < n; ++j) {
            if (!__any(alive)) break;
            const float4* rec = &s_rec[j * kQ];
            const uint32_t idx = __float_as_uint(rec[4].x);
            if (idx == 0xFFFFFFFFu) break;   // padding closes the list (gutKBufferRenderer.cuh:312-315)
            bool pop = false;
            float pop_t = 0.f, pop_a = 0.f;
            uint32_t pop_i = 0u;
            if (alive) {
                const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
                const f3 dl = ray.o - mk3(q0.w, q1.w, q2.w);
                const f3 gro = mk3(dot(mk3(q0.x, q0.y, q0.z), dl), dot(mk3(q1.x, q1.y, q1.z), dl), dot(mk3(q2.x, q2.y, q2.z), dl));
                const f3 grdu = mk3(dot(mk3(q0.x, q0.y, q0.z), ray.d), dot(mk3(q1.x, q1.y, q1.z), ray.d), dot(mk3(q2.x, q2.y, q2.z), ray.d));
                const float l2 = dot(grdu, grdu);
                const f3 gc = cross(grdu, gro);
                const float cc = dot(gc, gc);
                if (cc < rec[4].y * l2) {   // response > min_response && alpha > min_alpha
                    const float il2 = __builtin_amdgcn_rcpf(l2);
                    const float resp = response_rt(P.degree, cc * il2);
                    const float alpha = fminf(P.max_alpha, resp * q3.w);
                    // hit distance |S n (n.-u)| (gaussianParticles.slang:181-190), bits = the checker's: it is the k-buffer's sort key
                    const float4 q5 = rec[5], q6 = rec[6], q7 = rec[7];
                    const float hitT = oracle_order_hit_t(ray, mk3(q0.w, q1.w, q2.w), mk3(q3.x, q3.y, q3.z), mk3(q5.x, q5.y, q5.z), mk3(q6.x, q6.y, q6.z),
                                                          mk3(q7.x, q7.y, q7.z), mk3(q5.w, q6.w, q7.w));
                    if ((hitT > ray.tmin) && (hitT < ray.tmax)) {
                        if (kb.num == K) {   // full: the nearest pending hit is composited (below), the new one takes its slot
                            pop = true; pop_t = kb.hitT[0]; pop_a = kb.alpha[0]; pop_i = kb.idx[0];
                            kb.hitT[0] = -1.f;
                        } else {
                            kb.num++;
                        }
                        kb.insert(hitT, alpha, idx);
                    }
                }
            }
            if (BWD) {
                if (__any(pop)) {   // wave-level: gradients of lanes that popped the same particle are summed before the atomics
                    float terms[16];
                    const bool have = pop && k_bwd_terms(P, ray, density12, rgb, pop_t, pop_a, pop_i, bs, alive, terms);
                    if (kLdsFlush) k_bwd_flush_lds(have, pop_i, terms, lane, s_kterms, g_density12, g_rgb);
                    else k_bwd_flush(have, pop_i, terms, lane, g_density12, g_rgb);
                }
            } else if (pop) {
                k_process_fwd(P, rgb, pop_t, pop_a, pop_i, fs, alive);
            }
        }
        __syncthreads();
    }
    // drain what is left, nearest first (:343-351).  The buffer is ascending with the empty slots (hitT = -1) in front: K steps
    // that each take slot 0 and shift the rest down visit the pending hits in order; one copy of the per-hit code instead of K
    // (the gradient terms alone are ~600 instructions).
#pragma unroll 1
    for (int step = 0; step < K; ++step) {
        const float t0 = kb.hitT[0], a0 = kb.alpha[0];
        const uint32_t i0 = kb.idx[0];
#pragma unroll
        for (int i = 0; i + 1 < K; ++i) { kb.hitT[i] = kb.hitT[i + 1]; kb.alpha[i] = kb.alpha[i + 1]; kb.idx[i] = kb.idx[i + 1]; }
        kb.hitT[K - 1] = -1.f;
        const bool act = alive && (t0 >= 0.f);
        if (BWD) {
            if (__any(act)) {
                float terms[16];
                const bool have = act && k_bwd_terms(P, ray, density12, rgb, t0, a0, i0, bs, alive, terms);
                if (kLdsFlush) k_bwd_flush_lds(have, i0, terms, lane, s_kterms, g_density12, g_rgb);
                else k_bwd_flush(have, i0, terms, lane, g_density12, g_rgb);
            }
        } else if (act) {
            k_process_fwd(P, rgb, t0, a0, i0, fs, alive);
        }
    }
    if (!BWD && ray.inside) {
        const size_t opix = (size_t)py * P.W + px;
        const float4 o = ray.valid ? make_float4(fs.Cr, fs.Cg, fs.Cb, 1.f - fs.T) : make_float4(0.f, 0.f, 0.f, 0.f);
        store_fd(P, out_fd, opix, o);
        write_split_outputs(P, opix, o);
        out_dist[opix] = ray.valid ? fs.D : 1e6f;
        if (P.hitcounts) out_cnt[opix] = ray.valid ? fs.cnt : 0.f;
    }
}

// The forward fits three waves per SIMD when told to (1.96 vs 2.5 ms at K = 16); the backward needs its 231 registers
// (8.0 ms at two waves, 9.6 at three, 13.3 at four).
#ifndef GRUT_K_FWD_WAVES
#define GRUT_K_FWD_WAVES 3   // (measured again in round 5 with the exact-order hit distance: forward 3.07 / 2.61 / 3.08 ms at 2 / 3 / 4 waves)
#endif
template <int K>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(GRUT_K_FWD_WAVES))) void gut_render_k_fwd_kernel(
    GutParams P, const uint2* __restrict__ ranges, EntryLists lists, const float4* __restrict__ density12, const float* __restrict__ rgb,
    const float* __restrict__ ray_o, const float* __restrict__ ray_d, float4* __restrict__ out_fd, float* __restrict__ out_dist,
    float* __restrict__ out_cnt) {
    gut_render_k_body<K, false>(P, ranges, lists, density12, rgb, ray_o, ray_d, out_fd, out_dist, out_cnt, nullptr, nullptr, nullptr, nullptr);
}
// K = 16 with the LDS flush: 209 VGPRs where the DPP reduce-scatter needed 231 - held to 168 (116 B of scratch) the kernel runs three waves
// per SIMD: backward 8.59 -> 7.60 ms (A/B on one box; the LDS flush at two waves: 8.98, the DPP flush at three: 9.6 in round 2).  K = 8: 177 ->
// 161 VGPRs, three waves without scratch, backward 6.53 -> 6.06 ms.
#ifndef GRUT_K_BWD_WAVES
#define GRUT_K_BWD_WAVES 3
#endif
template <int K>
__global__ __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu((K >= GRUT_K_FLUSH_MINK && GRUT_K_FLUSH_LDS) ? GRUT_K_BWD_WAVES : 1, (K >= GRUT_K_FLUSH_MINK && GRUT_K_FLUSH_LDS) ? GRUT_K_BWD_WAVES : 8)))
void gut_render_k_bwd_kernel(GutParams P, const uint2* __restrict__ ranges, EntryLists lists,
                                                              const float4* __restrict__ density12, const float* __restrict__ rgb,
                                                              const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                              float4* __restrict__ fd, float* __restrict__ dist, const float4* __restrict__ g_fd,
                                                              const float* __restrict__ g_dist, float* __restrict__ g_density12,
                                                              float* __restrict__ g_rgb) {
    gut_render_k_body<K, true>(P, ranges, lists, density12, rgb, ray_o, ray_d, fd, dist, nullptr, g_fd, g_dist, g_density12, g_rgb);
}

}  // namespace

void launch_render_k_fwd(hipStream_t s, const GutParams& P, const uint32_t* ranges, const uint32_t* sorted_pos, const uint32_t* pos_particle,
                         const float* density12, const float* rgb, const float* ray_o, const float* ray_d, float* out_fd, float* out_dist,
                         float* out_cnt) {
    const EntryLists lists = entry_lists(P, sorted_pos, pos_particle);
    GRUT_DISPATCH_K(P.k_buffer, hipLaunchKernelGGL((gut_render_k_fwd_kernel<K_>), dim3(strip_grid(P)), dim3(64), 0, s, P,
                                                   reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12), rgb,
                                                   ray_o, ray_d, reinterpret_cast<float4*>(out_fd), out_dist, out_cnt));
}
void launch_render_k_bwd(hipStream_t s, const GutParams& P, const uint32_t* ranges, const uint32_t* sorted_pos, const uint32_t* pos_particle,
                         const float* density12, const float* rgb, const float* ray_o, const float* ray_d, const float* fd, const float* g_fd,
                         const float* dist, const float* g_dist, float* g_density12, float* g_rgb) {
    const EntryLists lists = entry_lists(P, sorted_pos, pos_particle);
    GRUT_DISPATCH_K(P.k_buffer, hipLaunchKernelGGL((gut_render_k_bwd_kernel<K_>), dim3(strip_grid(P)), dim3(64), 0, s, P,
                                                   reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12), rgb,
                                                   ray_o, ray_d, reinterpret_cast<float4*>(const_cast<float*>(fd)), const_cast<float*>(dist),
                                                   reinterpret_cast<const float4*>(g_fd), g_dist, g_density12, g_rgb));
}

}  // namespace grut
