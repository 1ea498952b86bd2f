// gut_render.hip — 3DGUT compositing for gfx950: front-to-back alpha compositing of the sorted tile lists and its
// gradient sweep.
//
// Reference behaviour restated (not translated): gutKBufferRenderer.cuh:199-352 (render, K = 0), :642-716
// (evalBackwardNoKBuffer, SH branch), common/rayPayload.cuh:75-193, rayPayloadBackward.cuh:30-73,
// models/gaussianParticles.cuh:350-422 (processHitFwd), :484-751 (processHitBwd).
//
// CDNA4 design.  Both sweeps are bound by fp32 VALU issue (one wave64 VALU instruction per 4 cycles per SIMD), not by
// HBM, so the kernels are organised around instruction count:
//   * one wave64 owns a 16x8 half tile and every lane carries a PAIR of pixels (rows y and y+4) in float2 registers,
//     so the multiply/add bulk of the per-(pixel, particle) math issues as v_pk_fma/mul/add_f32; per-particle operands
//     are wave-uniform LDS broadcasts selected by the packed instructions' op_sel;
//   * the accept test runs on the un-normalised quantities |v x u|^2 < g_max |v|^2 (u, v = ray origin / direction in
//     the particle's canonical frame, g_max = per-particle limit on grayDist derived from min_response and
//     min_alpha / density when the entry is staged): no transcendental on the reject path;
//   * when every ray of the wave shares its origin (pinhole / fisheye batches: rays_ori = 0 in camera space) the
//     canonical origin u is per particle and is staged with the record instead of being recomputed per pixel;
//   * gradient sweep: with a = u - v (v.u)/|v|^2 every geometric gradient is a multiple of a, so per hit a lane
//     produces  B = dL/d(R^T(o-mu))  (3),  M = B (x) (o - mu - t d)  (9, d rotT = M),  d density (1), d radiance (3)
//     = 16 terms; the two pixels are folded in-lane, summed over the wave through a transposition in LDS (lane l ends
//     up with a quarter of the wave total of term l mod 16) and written to the tile entry's own SLOT (one per entry and
//     half tile, no atomics: gradients are bitwise reproducible); quaternion, scale and position gradients are
//     contracted from (B, M) once per particle by the gather kernel, not per pixel.
#include "gut_render_common.inl"

// tuning switch of the gradient sweep (scripts/build_variant.sh NAME gut_render.hip -D...)
#ifndef GRUT_BWD_WAVES
#define GRUT_BWD_WAVES 4   // waves per SIMD the register allocator is held to (0: its own choice, 130 VGPRs = 3 waves); measured r02b:
#endif                     // rows / 3 waves 0.917 ms, rows / 4 waves 0.910, lane-swap reduce / 3 waves 0.936, lane-swap reduce / 4 waves 0.891
                           // ("rows" and "lane-swap reduce": the two retired forms of the per-entry reduction, GRUT_BWD_FULL_REDUCE 0 / 1 in
                           // profiles/r06_experiments_not_kept.txt; the kept transposition through LDS took the 4-wave build from 0.887 to 0.85 ms)

namespace grut {

namespace {

// ---------------------------------------------------------------------------------------------
// K7: compositing forward — GUTKBufferRenderer::evalKBuffer, K = 0 (gutKBufferRenderer.cuh:273-352)
// Rounds are aligned to multiples of 64 in the global sorted list, so every segment boundary (multiple of
// kGutSegment) is a round start, where the running state is checkpointed for the gradient sweep.
// ---------------------------------------------------------------------------------------------
#ifndef GRUT_FWD_HALF_TILE_CULL
#define GRUT_FWD_HALF_TILE_CULL 1   // staged entries whose sphere misses the wave's ray pyramid are dropped (see WavePyramid)
#endif
struct FwdState {
    v2f T, D, Cr, Cg, Cb, cnt;
    unsigned long long t_stage;   // instrumented build: ticks spent staging rounds
};
template <int DEG, bool CKPT, bool UNI, bool COUNT = false>
__device__ __forceinline__ void render_fwd_sweep(const GutParams& P, const RayPair& rp, uint2 range, uint32_t half, int lane,
                                                 const EntryLists& lists, const float4* __restrict__ density12,
                                                 const float* __restrict__ rgb, const GutCheckpoints& ck, float4* __restrict__ s_rec,
                                                 FwdState& st) {
    bool alive0 = rp.valid0, alive1 = rp.valid1;
    v2f T = splat(1.f), D = splat(0.f), Cr = splat(0.f), Cg = splat(0.f), Cb = splat(0.f), cnt = splat(0.f);
    uint32_t n_eval = 0u, n_acc = 0u, n_rounds = 0u;   // wave-uniform work counters (scalar registers), reported when P.work is set
    const unsigned long long t_sweep = COUNT ? wall_clock64() : 0ull;
    unsigned long long t_first = 0ull, t_stage = 0ull;
    uint32_t b = range.x;
    RawEntry next = load_entry<false>(b + lane, min(range.y, (b & ~63u) + 64u), lists, density12, rgb);
    constexpr bool CULL = GRUT_FWD_HALF_TILE_CULL != 0;
    WavePyramid pyr;
    if (UNI && CULL) pyr = wave_pyramid(rp);
    while (b < range.y) {
        if (!__any(alive0 || alive1)) break;
        const uint32_t bend = min(range.y, (b & ~63u) + 64u);
        if (CKPT && b > range.x && (b % kGutSegment) == 0) {
            const size_t slot = (((size_t)(b / kGutSegment) * 2 + half) * 64 + lane) * 2;
            // dead pixels restart dead (T = 0 < min_transmittance)
            ck.tc[slot] = make_float4(alive0 ? T.x : 0.f, Cr.x, Cg.x, Cb.x);
            ck.tc[slot + 1] = make_float4(alive1 ? T.y : 0.f, Cr.y, Cg.y, Cb.y);
            ck.d[slot] = D.x;
            ck.d[slot + 1] = D.y;
            if (lane == 0) ck.reached[(size_t)(b / kGutSegment) * 2 + half] = 3;   // (one bit per quarter of the half tile: both arrive together here)
        }
        int n = (int)(bend - b);
        if (COUNT) ++n_rounds;
        const unsigned long long t_round = COUNT ? wall_clock64() : 0ull;
        if (UNI && CULL) {
            // stage to a private record, drop it if its sphere misses the wave's pyramid, pack the survivors (order kept)
            float4 q[kRecQuads];
            stage_entry<DEG, false>(P, next, true, rp.origin, q);
            const bool keep = lane < n && next.idx != 0xFFFFFFFFu && !(pyr.on && pyramid_misses(pyr, q[0], q[1], q[2], q[4].w, q[5]));
            const unsigned long long km = __ballot(keep);
            if (keep) {
                float4* dst = &s_rec[__builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u)) * kRecQuads];
#pragma unroll
                for (int k = 0; k < kRecQuads; ++k) dst[k] = q[k];
            }
            n = __popcll(km);
        } else {
            stage_entry<DEG, false>(P, next, UNI, rp.origin, &s_rec[lane * kRecQuads]);
        }
        __syncthreads();  // single-wave workgroup: orders the LDS hand-off
        if (COUNT && n_rounds == 1u) t_first = wall_clock64() - t_sweep;
        if (COUNT) t_stage += wall_clock64() - t_round;
        // fetch the following round while this one is being composited
        next = load_entry<false>(bend + lane, min(range.y, bend + 64u), lists, density12, rgb);
        for (int j = 0; j < n; ++j) {
            if (!__any(alive0 || alive1)) break;   // the rest of the round is behind every pixel's termination
            const float4* rec = &s_rec[j * kRecQuads];
            const PairGeom g = pair_geometry<UNI>(rp, rec);
            const bool c0 = g.acc0 && alive0, c1 = g.acc1 && alive1;
            if (COUNT) ++n_eval;
            if (!__any(c0 || c1)) continue;
            if (COUNT) ++n_acc;
            const float4 r3 = rec[3], r4 = rec[4];
            const v2f il2 = prcp(g.l2);
            const v2f gray = g.cc * il2;
            const v2f resp = pair_response<DEG>(gray);
            const v2f ad = resp * r3.w;
            // hit distance |S n (n.-u)| = |v.u| |S v| / |v|^2   (gaussianParticles.slang:181-190)
            const v2f vu = pdot(g.v, g.u);
            const p3 sv = p3{r3.x * g.v.x, r3.y * g.v.y, r3.z * g.v.z};
            const v2f ss = pdot(sv, sv) * (vu * vu);
            const v2f hitT = v2f{__builtin_amdgcn_sqrtf(ss.x), __builtin_amdgcn_sqrtf(ss.y)} * il2;
            const bool h0 = c0 && (hitT.x > rp.tmin.x) && (hitT.x < rp.tmax.x);
            const bool h1 = c1 && (hitT.y > rp.tmin.y) && (hitT.y < rp.tmax.y);
            const v2f alpha = psel(h0, h1, v2f{fminf(P.max_alpha, ad.x), fminf(P.max_alpha, ad.y)}, splat(0.f));
            const v2f hT = psel(h0, h1, hitT, splat(0.f));
            const v2f w = alpha * T;
            D = pfma(hT, w, D);
            T = T * (1.f - alpha);
            Cr = pfma(r4.x, w, Cr);
            Cg = pfma(r4.y, w, Cg);
            Cb = pfma(r4.z, w, Cb);
            cnt += psel(w.x > 0.f, w.y > 0.f, splat(1.f), splat(0.f));
            alive0 = alive0 && !(T.x < P.min_transmittance);
            alive1 = alive1 && !(T.y < P.min_transmittance);
        }
        __syncthreads();
        b = bend;
    }
    st = FwdState{T, D, Cr, Cg, Cb, cnt, 0ull};
    if (COUNT && P.work && lane == 0) {   // per-wave words, summed on the host (atomics on two shared counters would serialise the waves' exits)
        P.work[16 + 4 * (size_t)blockIdx.x + 2] = ((unsigned long long)n_acc << 32) | n_eval;
        st.t_stage = t_stage;
        // [0, 24) list length, [24, 34) staged rounds, [34, 49) first round staged, [49, 64) sweep over - both in 10 ns ticks since the sweep began
        const unsigned long long t_done = wall_clock64() - t_sweep;
        P.work[16 + 4 * (size_t)blockIdx.x + 3] = (unsigned long long)min(range.y - range.x, 0xFFFFFFu) | ((unsigned long long)min(n_rounds, 1023u) << 24) |
                                                  (min(t_first, 32767ull) << 34) | (min(t_done, 32767ull) << 49);
    }
}

#ifndef GRUT_FWD_WAVES
#define GRUT_FWD_WAVES 6   // held to 80 VGPRs (12 B of scratch): r02v 0.485 -> 0.472 ms; 0 = the allocator's own choice (90 VGPRs, 5 waves): 4 waves 0.508
#endif
template <int DEG, bool CKPT, bool COUNT = false>
__global__ __launch_bounds__(64)
#if GRUT_FWD_WAVES > 0
__attribute__((amdgpu_waves_per_eu(GRUT_FWD_WAVES, GRUT_FWD_WAVES)))
#endif
void gut_render_fwd_kernel(GutParams P, const uint2* __restrict__ ranges, EntryLists lists,
                                                            const float4* __restrict__ density12, const float* __restrict__ rgb,
                                                            const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                            float4* __restrict__ out_fd, float* __restrict__ out_dist,
                                                            float* __restrict__ out_cnt, GutCheckpoints ck) {
    __shared__ float4 s_rec[64 * kRecQuads];
    uint32_t tile, half;
    half_mapping(blockIdx.x, tile, half);
    if (tile >= (uint32_t)(P.gx * P.gy)) return;
#ifndef GRUT_FWD_TILE_STRIDE
#define GRUT_FWD_TILE_STRIDE 997   // tiles visited with a stride: r02t/r02u rows only, stride 21 of 68: 0.517 -> 0.490 ms; r02ah every tile,
#endif                             // stride 997 of 8160: another 0.017 ms (strides 61 / 499 / 1777 / 3001: no better than the rows)
    if (GRUT_FWD_TILE_STRIDE > 1) tile = stride_permute(tile, (uint32_t)(P.gx * P.gy), GRUT_FWD_TILE_STRIDE);
    const int lane = threadIdx.x;
    const unsigned long long t_begin = COUNT ? wall_clock64() : 0ull;   // constant-rate (100 MHz) counter shared by the whole chip
    const RayPair rp = init_ray_pair(P, ray_o, ray_d, tile, half, lane);
    const uint2 range = ranges[tile];
    const unsigned long long t_rays = COUNT ? wall_clock64() : 0ull;
    FwdState st;
    // two copies of the sweep: the shared-origin one keeps the canonical origin out of the per-pixel math
    if (rp.uniform_origin) render_fwd_sweep<DEG, CKPT, true, COUNT>(P, rp, range, half, lane, lists, density12, rgb, ck, s_rec, st);
    else render_fwd_sweep<DEG, CKPT, false, COUNT>(P, rp, range, half, lane, lists, density12, rgb, ck, s_rec, st);
    if (COUNT && P.work && lane == 0) {   // diagnostics: this wave's lifetime (shader-clock ticks) and start time, for the balance analysis
        const unsigned long long t_end = wall_clock64();
        // lifetime | rays ready << 32 | time spent staging << 48 (10 ns ticks)
        P.work[16 + 4 * (size_t)blockIdx.x] = (t_end - t_begin) | (min(t_rays - t_begin, 0xFFFFull) << 32) | (min(st.t_stage, 0xFFFFull) << 48);
        P.work[16 + 4 * (size_t)blockIdx.x + 1] = t_begin;
    }
    // every pixel of the image is written (the caller does not pre-fill): rays that miss the scene box get the reference's
    // initial values (splatRaster.cpp:211-214)
    if (rp.inside0) {
        const size_t pix = (size_t)rp.py0 * P.W + rp.px;
        const float4 o = rp.valid0 ? make_float4(st.Cr.x, st.Cg.x, st.Cb.x, 1.f - st.T.x) : make_float4(0.f, 0.f, 0.f, 0.f);
        store_fd(P, out_fd, pix, o);
        write_split_outputs(P, pix, o);
        out_dist[pix] = rp.valid0 ? st.D.x : 1e6f;
        if (P.hitcounts) out_cnt[pix] = rp.valid0 ? st.cnt.x : 0.f;
    }
    if (rp.inside1) {
        const size_t pix = (size_t)rp.py1 * P.W + rp.px;
        const float4 o = rp.valid1 ? make_float4(st.Cr.y, st.Cg.y, st.Cb.y, 1.f - st.T.y) : make_float4(0.f, 0.f, 0.f, 0.f);
        store_fd(P, out_fd, pix, o);
        write_split_outputs(P, pix, o);
        out_dist[pix] = rp.valid1 ? st.D.y : 1e6f;
        if (P.hitcounts) out_cnt[pix] = rp.valid1 ? st.cnt.y : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// K7q: the forward for launches that fit the chip at once (round 4).  When every wave of the launch is resident from the start
// (BASELINE configs 1 and 2: 1 250 / 5 000 half tiles for 6 144 slots) the longest wave IS the kernel, and a lone wave pays ~8 cycles per
// dependent instruction whatever its lane count: what shortens it is fewer instructions per entry.  One pixel per lane - a QUARTER tile
// (16 x 4 pixels) per wave, the .x pixels (quarter 0) or the .y pixels (quarter 1) of the half-tile wave's lanes - runs the same entry in
// ~0.6x the instructions (plain instead of packed arithmetic), walks the same list only as far as ITS 64 pixels need, and culls staged
// entries against a pyramid half as high.  Every expression below is the pair sweep's, component by component (same fused
// multiply-adds, same order): for frames with one ray origin - every frame of the static cameras - images, hit counts, checkpoints and
// with them all gradients are bit-identical to the half-tile kernel's; with per-pixel ray origins the two builds differ by an ulp per hit
// somewhere the source does not show (1.2e-7 median on the image; tests/test_gut_gpu.py::test_quarter_tile_forward_equals_the_half_tile_forward).  Checkpoints keep the pair layout
// (slot + quarter); `reached` carries one bit per quarter, set atomically, and the gradient sweep starts the pixels of a quarter that
// did not arrive dead.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float qdot(f3 a, f3 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, a.z * b.z)); }
template <int DEG>
__device__ __forceinline__ float response1(float g) {
    constexpr float kLog2e = 1.4426950408889634f;
    if constexpr (DEG == 2) return __builtin_amdgcn_exp2f(g * (-0.5f * kLog2e));
    else if constexpr (DEG == 4) return __builtin_amdgcn_exp2f((g * g) * (-0.0555555555556f * kLog2e));
    else return particle_response<DEG>(g);
}
template <int DEG, bool CKPT, bool UNI>
__device__ __forceinline__ void render_fwd_sweep_quarter(const GutParams& P, const Ray& ry, f3 origin, uint2 range, uint32_t half, uint32_t quarter, int lane,
                                                         const EntryLists& lists, const float4* __restrict__ density12, const float* __restrict__ rgb,
                                                         const GutCheckpoints& ck, float4* __restrict__ s_rec, float (&st)[6]) {
    bool alive = ry.valid;
    float T = 1.f, D = 0.f, Cr = 0.f, Cg = 0.f, Cb = 0.f, cnt = 0.f;
    uint32_t b = range.x;
    RawEntry next = load_entry<false>(b + lane, min(range.y, (b & ~63u) + 64u), lists, density12, rgb);
    WavePyramid pyr;
    if (UNI) pyr = wave_pyramid(ry.valid, ry.d, false, ry.d);
    while (b < range.y) {
        if (!__any(alive)) break;
        const uint32_t bend = min(range.y, (b & ~63u) + 64u);
        if (CKPT && b > range.x && (b % kGutSegment) == 0) {
            const size_t idx = (size_t)(b / kGutSegment) * 2 + half;
            const size_t slot = (idx * 64 + lane) * 2 + quarter;
            ck.tc[slot] = make_float4(alive ? T : 0.f, Cr, Cg, Cb);   // dead pixels restart dead
            ck.d[slot] = D;
            if (lane == 0) atomicOr(reinterpret_cast<uint32_t*>(ck.reached) + (idx >> 2), (1u << quarter) << (8u * (uint32_t)(idx & 3)));
        }
        int n = (int)(bend - b);
        if (UNI) {
            float4 q[kRecQuads];
            stage_entry<DEG, false>(P, next, true, origin, q);
            const bool keep = lane < n && next.idx != 0xFFFFFFFFu && !(pyr.on && pyramid_misses(pyr, q[0], q[1], q[2], q[4].w, q[5]));
            const unsigned long long km = __ballot(keep);
            if (keep) {
                float4* dst = &s_rec[__builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u)) * kRecQuads];
#pragma unroll
                for (int k = 0; k < kRecQuads; ++k) dst[k] = q[k];
            }
            n = __popcll(km);
        } else {
            stage_entry<DEG, false>(P, next, false, origin, &s_rec[lane * kRecQuads]);
        }
        __syncthreads();
        next = load_entry<false>(bend + lane, min(range.y, bend + 64u), lists, density12, rgb);
        for (int j = 0; j < n; ++j) {
            if (!__any(alive)) break;
            const float4* rec = &s_rec[j * kRecQuads];
            const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
            const f3 m0 = mk3(r0.x, r0.y, r0.z), m1 = mk3(r1.x, r1.y, r1.z), m2 = mk3(r2.x, r2.y, r2.z);
            const f3 v = mk3(qdot(m0, ry.d), qdot(m1, ry.d), qdot(m2, ry.d));
            f3 u;
            if (UNI) { const float4 r5 = rec[5]; u = mk3(r5.x, r5.y, r5.z); }
            else { const f3 dl = mk3(ry.o.x - r0.w, ry.o.y - r1.w, ry.o.z - r2.w); u = mk3(qdot(m0, dl), qdot(m1, dl), qdot(m2, dl)); }
            const float l2 = qdot(v, v);
            const f3 c = mk3(fmaf(v.y, u.z, -(v.z * u.y)), fmaf(v.z, u.x, -(v.x * u.z)), fmaf(v.x, u.y, -(v.y * u.x)));
            const float cc = qdot(c, c);
            const float4 r4 = rec[4];
            const bool acc = cc < r4.w * l2;
            const bool ca = acc && alive;
            if (!__any(ca)) continue;
            const float4 r3 = rec[3];
            const float il2 = __builtin_amdgcn_rcpf(l2);
            const float gray = cc * il2;
            const float resp = response1<DEG>(gray);
            const float ad = resp * r3.w;
            const float vu = qdot(v, u);
            const f3 sv = mk3(r3.x * v.x, r3.y * v.y, r3.z * v.z);
            const float ss = qdot(sv, sv) * (vu * vu);
            const float hitT = __builtin_amdgcn_sqrtf(ss) * il2;
            const bool h = ca && (hitT > ry.tmin) && (hitT < ry.tmax);
            const float alpha = h ? fminf(P.max_alpha, ad) : 0.f;
            const float hT = h ? hitT : 0.f;
            const float w = alpha * T;
            D = fmaf(hT, w, D);
            T = T * (1.f - alpha);
            Cr = fmaf(r4.x, w, Cr);
            Cg = fmaf(r4.y, w, Cg);
            Cb = fmaf(r4.z, w, Cb);
            cnt += w > 0.f ? 1.f : 0.f;
            alive = alive && !(T < P.min_transmittance);
        }
        __syncthreads();
        b = bend;
    }
    st[0] = T; st[1] = D; st[2] = Cr; st[3] = Cg; st[4] = Cb; st[5] = cnt;
}
// block -> (virtual tile, half, quarter): the four waves of a tile on one XCD, like half_mapping
template <int DEG, bool CKPT>
__global__ __launch_bounds__(64) void gut_render_fwd_quarter_kernel(GutParams P, const uint2* __restrict__ ranges, EntryLists lists,
                                                                    const float4* __restrict__ density12, const float* __restrict__ rgb,
                                                                    const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                                    float4* __restrict__ out_fd, float* __restrict__ out_dist,
                                                                    float* __restrict__ out_cnt, GutCheckpoints ck) {
    __shared__ float4 s_rec[64 * kRecQuads];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    uint32_t tile = ((slot >> 2) << 3) + xcd;
    const uint32_t half = (slot >> 1) & 1u, quarter = slot & 1u;
    if (tile >= (uint32_t)(P.gx * P.gy)) return;
    if (GRUT_FWD_TILE_STRIDE > 1) tile = stride_permute(tile, (uint32_t)(P.gx * P.gy), GRUT_FWD_TILE_STRIDE);
    const int lane = threadIdx.x;
    const int px = (int)(tile % P.gx) * 16 + (lane & 15), py = (int)(tile / P.gx) * 16 + (int)half * 8 + (int)quarter * 4 + (lane >> 4);
    const Ray ry = init_ray(P, ray_o, ray_d, px, py);
    // wave-uniform origin?  (as init_ray_pair)
    const unsigned long long m = __ballot(ry.valid);
    f3 cand = mk3(0.f, 0.f, 0.f);
    if (m) {
        const int src = __ffsll((long long)m) - 1;
        cand = mk3(__shfl(ry.o.x, src, 64), __shfl(ry.o.y, src, 64), __shfl(ry.o.z, src, 64));
    }
    const bool uniform_origin = __all(!ry.valid || (ry.o.x == cand.x && ry.o.y == cand.y && ry.o.z == cand.z));
    const uint2 range = ranges[tile];
    float st[6];
    if (uniform_origin) render_fwd_sweep_quarter<DEG, CKPT, true>(P, ry, cand, range, half, quarter, lane, lists, density12, rgb, ck, s_rec, st);
    else render_fwd_sweep_quarter<DEG, CKPT, false>(P, ry, cand, range, half, quarter, lane, lists, density12, rgb, ck, s_rec, st);
    if (ry.inside) {
        const size_t pix = (size_t)py * P.W + px;
        const float4 o = ry.valid ? make_float4(st[2], st[3], st[4], 1.f - st[0]) : make_float4(0.f, 0.f, 0.f, 0.f);
        store_fd(P, out_fd, pix, o);
        write_split_outputs(P, pix, o);
        out_dist[pix] = ry.valid ? st[1] : 1e6f;
        if (P.hitcounts) out_cnt[pix] = ry.valid ? st[5] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// K8: compositing backward — evalBackwardNoKBuffer SH branch (gutKBufferRenderer.cuh:642-716) with
// processHitBwd (models/gaussianParticles.cuh:484-751).
//
// With u = gro, v = grdu (un-normalised), t = (v.u)/|v|^2, a = u - t v:  grayDist = |a|^2 and
//   d gray / d u = 2 a,      d gray / d v = -2 t a
// so with wg = dL/d gray:  uGrd = 2 wg a,  vGrd = -t uGrd,  B = uGrd / scale = dL/d(R^T (o - mu)),
//   dL/d rotT = B (x) (o - mu) + (-t B) (x) d = B (x) e,   e = (o - mu) - t d
//   dL/d position = -R B,     dL/d scale_i = -(1/s_i) sum_j rotT_ij M_ij,    M = sum over pixels of B (x) e
// which is the reference's chain (two cross-product backward passes, safe_normalize_bw, matmul_bw_vec/quat) collapsed.
// For uniform-origin waves  M = (sum B) (x) (o - mu) - sum (t B) (x) d  and only the second sum is reduced.
// When a depth gradient flows in (HAS_GDIST) the hit-distance terms (gaussianParticles.cuh:545-580) are added in
// their generic form: B (x) (o-mu) and Bv (x) d are accumulated separately and the direct scale term is reduced in a
// second pass.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kBwdBatch = 32;  // staged entries per round of the gradient sweep

struct BwdPixels {
    v2f T, D, Cr, Cg, Cb;           // running state
    v2f T_fin, D_fin, gT, gD;       // forward results and upstream gradients
    p3 C_fin, gC;
    bool alive0, alive1;
};
template <int DEG, bool HAS_GDIST, bool UNI, bool COUNT = false>
__device__ __forceinline__ void render_bwd_sweep(const GutParams& P, const RayPair& rp, uint32_t seg_begin, uint32_t seg_end, int lane,
                                                 uint32_t half, const EntryLists& lists, const float4* __restrict__ density12,
                                                 const float* __restrict__ rgb, const GutGradSlots& slots,
                                                 float4* __restrict__ s_rec, float* __restrict__ s_acc, float* __restrict__ s_acc2,
                                                 float* __restrict__ s_tr, uint2* __restrict__ s_who, const BwdPixels& px) {
    constexpr uint32_t kBatch = kBwdBatch;
    v2f T = px.T, D = px.D, Cr = px.Cr, Cg = px.Cg, Cb = px.Cb;
    const v2f T_fin = px.T_fin, D_fin = px.D_fin, gT = px.gT, gD = px.gD;
    const p3 C_fin = px.C_fin, gC = px.gC;
    bool alive0 = px.alive0, alive1 = px.alive1;
    uint32_t n_eval = 0u, n_acc = 0u;
    v2f iT = prcp(T);   // running 1 / T (a dead pixel restarts with T = 0: its reciprocal is never used, see inextT)
    uint32_t b = seg_begin;
    RawEntry next = load_entry(b + lane, min(seg_end, (b & ~(kBatch - 1u)) + kBatch), lists, density12, rgb);
    while (b < seg_end) {
        if (!__any(alive0 || alive1)) break;
        const uint32_t bend = min(seg_end, (b & ~(kBatch - 1u)) + kBatch);
        if (lane < (int)kBatch) {
            stage_entry<DEG, true>(P, next, UNI, rp.origin, &s_rec[lane * kRecQuads]);
            // the flush marks the entry's slot under its particle and ordinal: parked here, `next` is about to be overwritten
            s_who[lane] = make_uint2(next.idx, entry_ordinal(next, lists, slots.part_offset));
        }
        __syncthreads();
        next = load_entry(bend + lane, min(seg_end, bend + kBatch), lists, density12, rgb);
        const int n = (int)(bend - b);
        uint32_t hit_entries = 0u;  // wave-uniform: staged entries with >= 1 hit in this wave
        for (int j = 0; j < n; ++j) {
            if (!__any(alive0 || alive1)) break;
            const float4* rec = &s_rec[j * kRecQuads];
            const PairGeom g = pair_geometry<UNI>(rp, rec);
            const bool h0 = g.acc0 && alive0, h1 = g.acc1 && alive1;
            if (COUNT) ++n_eval;
            if (!__any(h0 || h1)) continue;
            if (COUNT) ++n_acc;
            hit_entries |= (1u << j);
            const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3], r4 = rec[4];
            const v2f il2 = prcp(g.l2);
            const v2f gray = g.cc * il2;
            const v2f resp = pair_response<DEG>(gray);
            const v2f ad = resp * r3.w;
            const v2f alpha = psel(h0, h1, v2f{fminf(P.max_alpha, ad.x), fminf(P.max_alpha, ad.y)}, splat(0.f));
            const v2f weight = alpha * T;
            const v2f oma = 1.f - alpha;
            const v2f nextT = oma * T;
            // 1 / nextT = (1 / T) (1 / (1 - alpha)): the running reciprocal iT is refreshed from T at every segment start,
            // which keeps its rounding drift below 1e-5 relative and saves two quarter-rate v_rcp_f32 per entry
            const v2f ioma = prcp(oma);
            const v2f inextT_raw = iT * ioma;
            const v2f inextT = psel(nextT.x <= P.min_transmittance, nextT.y <= P.min_transmittance, splat(0.f), inextT_raw);
            const v2f resTrm = psel(alpha.x < 0.999999f, alpha.y < 0.999999f, T_fin * ioma, T);
            v2f dalpha = -(resTrm * gT);  // d L / d alpha
            const p3 dc = p3{gC.x * weight, gC.y * weight, gC.z * weight};
            Cr = pfma(r4.x, weight, Cr); Cg = pfma(r4.y, weight, Cg); Cb = pfma(r4.z, weight, Cb);
            const v2f rr = pmax0((C_fin.x - Cr) * inextT), rg = pmax0((C_fin.y - Cg) * inextT), rb = pmax0((C_fin.z - Cb) * inextT);
            dalpha = pfma(T, pfma(r4.x - rr, gC.x, pfma(r4.y - rg, gC.y, (r4.z - rb) * gC.z)), dalpha);

            const v2f vu = pdot(g.v, g.u);
            const v2f t = vu * il2;
            // a = u - t v as (v x u) x v / |v|^2, the reference's own form (d gray / d gro = 2 (grd x gro) x grd): the difference loses
            // |u| / |a| in relative accuracy - |u| is the ray origin's distance in units of the particle's scales, several hundred for
            // a thin particle, |a| < 3 on every accepted hit - and the error goes straight into B, i.e. the position gradient
            // (1e-4 relative per hit at |u| = 490, tests/test_row_gradients_gpu.py); the cross product is already there for the
            // accept test and is orthogonal to v, so the second product cancels nothing.  (a is left un-normalised here,
            // a = |v|^2 (u - t v): its only use is a * wg2, and wg2 takes the 1 / |v|^2)
            const p3 a = pcross(g.c, g.v);
            // canonical-frame offsets of the ray origin, needed un-scaled for the rotation gradient
            p3 dl;
            if (UNI) dl = p3{splat(rp.origin.x - r0.w), splat(rp.origin.y - r1.w), splat(rp.origin.z - r2.w)};
            else dl = p3{rp.o.x - r0.w, rp.o.y - r1.w, rp.o.z - r2.w};

            p3 uX = p3{splat(0.f), splat(0.f), splat(0.f)}, vX = uX, sX = uX;   // hit-distance extras
            if (HAS_GDIST) {
                // n = v/|v|, pdot = -(n.u), grds = s * n * pdot, hitT = |grds|  (gaussianParticles.cuh:545-580)
                const v2f il = v2f{__builtin_amdgcn_rsqf(g.l2.x), __builtin_amdgcn_rsqf(g.l2.y)};
                const p3 nrm = p3{g.v.x * il, g.v.y * il, g.v.z * il};
                const v2f nu = vu * il;
                const v2f pdt = -nu;
                const p3 gscl = p3{prcp(splat(r3.x)), prcp(splat(r3.y)), prcp(splat(r3.z))};
                const p3 grdd = p3{nrm.x * pdt, nrm.y * pdt, nrm.z * pdt};
                const p3 grds = p3{gscl.x * grdd.x, gscl.y * grdd.y, gscl.z * grdd.z};
                const v2f gsq = pdot(grds, grds);
                const v2f gdist = v2f{__builtin_amdgcn_sqrtf(gsq.x), __builtin_amdgcn_sqrtf(gsq.y)};
                D = pfma(weight, gdist, D);
                const v2f resHitT = pmax0((D_fin - D) * inextT);
                dalpha = pfma((gdist - resHitT) * T, gD, dalpha);
                const v2f k = psel(gsq.x > 0.f, gsq.y > 0.f, weight * prcp(gdist) * gD, splat(0.f));
                const p3 grdsGrd = p3{grds.x * k, grds.y * k, grds.z * k};
                sX = p3{grdd.x * grdsGrd.x, grdd.y * grdsGrd.y, grdd.z * grdsGrd.z};     // direct d hitT / d scale
                const p3 sg = p3{gscl.x * grdsGrd.x, gscl.y * grdsGrd.y, gscl.z * grdsGrd.z};
                const v2f sd = pdot(sg, nrm);
                const p3 nGrd = p3{pfma(sg.x, pdt, -(g.u.x * sd)), pfma(sg.y, pdt, -(g.u.y * sd)), pfma(sg.z, pdt, -(g.u.z * sd))};
                uX = p3{-(nrm.x * sd), -(nrm.y * sd), -(nrm.z * sd)};                    // d / d gro
                const v2f ng = pdot(nrm, nGrd);                                          // safe_normalize_bw
                vX = p3{(nGrd.x - nrm.x * ng) * il, (nGrd.y - nrm.y * ng) * il, (nGrd.z - nrm.z * ng) * il};
            }

            dalpha = psel(h0, h1, dalpha, splat(0.f));
            const v2f dn = resp * dalpha;
            const v2f dresp = r3.w * dalpha;
            const v2f wg2 = psel(h0, h1, 2.f * v2f{particle_response_grd<DEG>(gray.x, resp.x, dresp.x),
                                                    particle_response_grd<DEG>(gray.y, resp.y, dresp.y)}, splat(0.f)) * il2;
            p3 uGrd = p3{a.x * wg2, a.y * wg2, a.z * wg2};                 // d L / d gro
            float terms[16], extra[16];
            if (!HAS_GDIST) {
                const p3 B = p3{r3.x * uGrd.x, r3.y * uGrd.y, r3.z * uGrd.z};   // d L / d (R^T (o - mu))
                p3 e;   // second factor of the rank-1 rotation gradient
                v2f s;  // ... and its scale on B
                if (UNI) { e = rp.d; s = -t; }                    // (sum B) (x) (o - mu) is added at flush
                else { e = p3{pfma(-t, rp.d.x, dl.x), pfma(-t, rp.d.y, dl.y), pfma(-t, rp.d.z, dl.z)}; s = splat(1.f); }
                const p3 Bs = p3{B.x * s, B.y * s, B.z * s};
                const v2f m[9] = {Bs.x * e.x, Bs.x * e.y, Bs.x * e.z, Bs.y * e.x, Bs.y * e.y, Bs.y * e.z, Bs.z * e.x, Bs.z * e.y, Bs.z * e.z};
                terms[0] = B.x.x + B.x.y; terms[1] = B.y.x + B.y.y; terms[2] = B.z.x + B.z.y; terms[3] = dn.x + dn.y;
#pragma unroll
                for (int k = 0; k < 9; ++k) terms[4 + k] = m[k].x + m[k].y;
                terms[13] = dc.x.x + dc.x.y; terms[14] = dc.y.x + dc.y.y; terms[15] = dc.z.x + dc.z.y;
            } else {
                const v2f mt = psel(h0, h1, splat(1.f), splat(0.f));
                uGrd = p3{pfma(uX.x, mt, uGrd.x), pfma(uX.y, mt, uGrd.y), pfma(uX.z, mt, uGrd.z)};
                const p3 vGrd = p3{pfma(vX.x, mt, -(t * a.x * wg2)), pfma(vX.y, mt, -(t * a.y * wg2)), pfma(vX.z, mt, -(t * a.z * wg2))};
                const p3 B = p3{r3.x * uGrd.x, r3.y * uGrd.y, r3.z * uGrd.z};
                const p3 Bv = p3{r3.x * vGrd.x, r3.y * vGrd.y, r3.z * vGrd.z};
                const v2f m[9] = {pfma(B.x, dl.x, Bv.x * rp.d.x), pfma(B.x, dl.y, Bv.x * rp.d.y), pfma(B.x, dl.z, Bv.x * rp.d.z),
                                  pfma(B.y, dl.x, Bv.y * rp.d.x), pfma(B.y, dl.y, Bv.y * rp.d.y), pfma(B.y, dl.z, Bv.y * rp.d.z),
                                  pfma(B.z, dl.x, Bv.z * rp.d.x), pfma(B.z, dl.y, Bv.z * rp.d.y), pfma(B.z, dl.z, Bv.z * rp.d.z)};
                terms[0] = B.x.x + B.x.y; terms[1] = B.y.x + B.y.y; terms[2] = B.z.x + B.z.y; terms[3] = dn.x + dn.y;
#pragma unroll
                for (int k = 0; k < 9; ++k) terms[4 + k] = m[k].x + m[k].y;
                terms[13] = dc.x.x + dc.x.y; terms[14] = dc.y.x + dc.y.y; terms[15] = dc.z.x + dc.z.y;
                const p3 sXm = p3{sX.x * mt, sX.y * mt, sX.z * mt};
#pragma unroll
                for (int k = 0; k < 16; ++k) extra[k] = 0.f;
                extra[0] = sXm.x.x + sXm.x.y; extra[1] = sXm.y.x + sXm.y.y; extra[2] = sXm.z.x + sXm.z.y;
            }
            // transpose through LDS instead of the DPP butterfly: the sweep is bound by VALU issue and the LDS pipe is idle, so the
            // 16 x 64 -> 16 reduction is moved there: every lane parks its 16 terms (term-major, rows padded to 65 words: conflict-free
            // both ways), lane l then sums 16 of the 64 values of term l & 15 and two lane-swap steps add the four quarters
            {
#pragma unroll
                for (int k = 0; k < 16; ++k) s_tr[k * 65 + lane] = terms[k];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                const float* col = &s_tr[(lane & 15) * 65 + (lane >> 4) * 16];
                float part = col[0];
#pragma unroll
                for (int k = 1; k < 16; ++k) part += col[k];
                typedef unsigned v2u __attribute__((ext_vector_type(2)));
                const v2u sa = __builtin_amdgcn_permlane32_swap(__float_as_uint(part), __float_as_uint(part), false, false);
                const float s2 = __uint_as_float(sa.x) + __uint_as_float(sa.y);
                const v2u sb = __builtin_amdgcn_permlane16_swap(__float_as_uint(s2), __float_as_uint(s2), false, false);
                const float tot = __uint_as_float(sb.x) + __uint_as_float(sb.y);
                if (lane < 16) s_acc[j * 16 + lane] = tot;
                __builtin_amdgcn_wave_barrier();   // the next entry overwrites s_tr
            }
            if (HAS_GDIST) {
                const float tot2 = wave_reduce_scatter16_all(extra, lane);
                if (lane < 16) s_acc2[j * 16 + lane] = tot2;
            }
            T = nextT;
            iT = inextT_raw;
            alive0 = alive0 && !(T.x < P.min_transmittance);
            alive1 = alive1 && !(T.y < P.min_transmittance);
        }
        __syncthreads();
        // flush: lane j owns staged entry j and stores the wave totals of its 16 (+3) terms to the entry's gradient slot
        if (lane < (int)kBatch && ((hit_entries >> lane) & 1u)) {
            const float4* rec = &s_rec[lane * kRecQuads];
            const uint32_t pos = __float_as_uint(rec[5].w);
            const float4* acc = reinterpret_cast<const float4*>(&s_acc[lane * 16]);
            float4 a0 = acc[0], a1 = acc[1], a2 = acc[2], a3 = acc[3];
            if (!HAS_GDIST && UNI) {  // complete M = (sum B) (x) (o - mu) - sum (t B) (x) d
                const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
                const f3 dl = rp.origin - mk3(r0.w, r1.w, r2.w);
                a1.x += a0.x * dl.x; a1.y += a0.x * dl.y; a1.z += a0.x * dl.z;
                a1.w += a0.y * dl.x; a2.x += a0.y * dl.y; a2.y += a0.y * dl.z;
                a2.z += a0.z * dl.x; a2.w += a0.z * dl.y; a3.x += a0.z * dl.z;
            }
            const size_t slot = 2 * (size_t)pos + half;
            float4* out = reinterpret_cast<float4*>(slots.partial + slot * (HAS_GDIST ? 20 : 16));
            out[0] = a0; out[1] = a1; out[2] = a2; out[3] = a3;
            if (HAS_GDIST) out[4] = make_float4(s_acc2[lane * 16], s_acc2[lane * 16 + 1], s_acc2[lane * 16 + 2], 0.f);
            const uint2 who = s_who[lane];
            mark_slot(slots, who.x, who.y, half, slot);
        }
        __syncthreads();
        b = bend;
    }
    if (COUNT && P.work && lane == 0) { atomicAdd(&P.work[2], (unsigned long long)n_eval); atomicAdd(&P.work[3], (unsigned long long)n_acc); }
}

template <int DEG, bool HAS_GDIST, bool COUNT = false>
#if GRUT_BWD_WAVES   // the depth-gradient variant (not the training path) needs ~160 registers: it keeps its 3 waves per SIMD
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(HAS_GDIST ? 3 : GRUT_BWD_WAVES, HAS_GDIST ? 3 : GRUT_BWD_WAVES))) void gut_render_bwd_kernel(
#else
__global__ __launch_bounds__(64) void gut_render_bwd_kernel(
#endif
                                                            GutParams P, const uint2* __restrict__ ranges, EntryLists lists,
                                                            const float4* __restrict__ density12, const float* __restrict__ rgb,
                                                            const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                            const float4* __restrict__ fd, GutGradIn g_in,
                                                            const float* __restrict__ dist, const float* __restrict__ g_dist,
                                                            GutGradSlots slots, GutCheckpoints ck) {
    constexpr uint32_t kBatch = kBwdBatch;
    __shared__ float4 s_rec[kBatch * kRecQuads];
    __shared__ float s_tr[16 * 65];                            // transposition buffer of the per-entry reduction
    __shared__ float s_acc[kBatch * 16];                       // per staged entry: the wave totals of its 16 terms
    __shared__ float s_acc2[HAS_GDIST ? kBatch * 16 : 1];      // depth-gradient extras (3 terms used)
    __shared__ uint2 s_who[kBatch];                            // per staged entry: {particle, ordinal among the particle's tile entries}
    // task = (virtual tile, half).  Virtual tiles [0, bndPad) are the segments that start at segment boundary b (sorted
    // index b * kGutSegment): they are the long, dense tasks and are dispatched first so that the tail of the launch
    // is made of the short first segments of each tile list, virtual tiles [bndPad, bndPad + tiles).  Only a quarter of the
    // launched workgroups find work on the bench frame (the forward reached 26 k of the ~106 k possible tasks alive); compacting
    // them into a task list first (persistent workers, or one workgroup per real task) was measured and is NOT faster: the empty
    // workgroups retire in the shadow of the running ones (DESIGN.md "Gradient sweep: task dispatch").  Measured again in round 4 with 64-entry
    // segments (376 k workgroups for ~100 k tasks; launching them all EMPTY takes 82 us): a compacted task list built by a small kernel, the grid
    // sized from the previous frame's count - gradient sweep 0.825-0.829 ms against 0.810-0.816 ms with the direct mapping.  Not kept.
    const uint32_t num_tiles = (uint32_t)(P.gx * P.gy), bnd_pad = (ck.num_boundaries + 7u) & ~7u;
    uint32_t vtile, half;
    half_mapping(blockIdx.x, vtile, half);
    uint32_t tile, seg_begin;
    bool from_checkpoint = false;
    uint32_t boundary = 0, reached_bits = 3u;   // bit q: quarter q of the half tile (pixel .x / .y of the lanes) arrived at the boundary alive
    if (vtile >= bnd_pad) {
        tile = vtile - bnd_pad;
        if (tile >= num_tiles) return;
        seg_begin = ranges[tile].x;
    } else {
        boundary = vtile;
        if (boundary == 0 || boundary >= ck.num_boundaries) return;
        reached_bits = ck.reached[(size_t)boundary * 2 + half];
        if (!reached_bits) return;                                   // the forward sweep never got here alive
        tile = ck.boundary_tile[boundary];
        if (tile >= num_tiles) return;
        seg_begin = boundary * kGutSegment;
        if (seg_begin <= ranges[tile].x) return;                     // the boundary is this tile's own list start
        from_checkpoint = true;
    }
    const int lane = threadIdx.x;
    const uint32_t seg_end = min(ranges[tile].y, (seg_begin / kGutSegment + 1u) * kGutSegment);
    const unsigned long long t_begin = COUNT ? wall_clock64() : 0ull;
    const RayPair rp = init_ray_pair(P, ray_o, ray_d, tile, half, lane);
    bool alive0 = rp.valid0, alive1 = rp.valid1;

    v2f T = splat(1.f), D = splat(0.f), Cr = splat(0.f), Cg = splat(0.f), Cb = splat(0.f);
    v2f T_fin = splat(0.f), D_fin = splat(0.f), gT = splat(0.f), gD = splat(0.f);
    p3 C_fin = p3{splat(0.f), splat(0.f), splat(0.f)}, gC = C_fin;
    if (alive0) {
        const size_t pix = (size_t)rp.py0 * P.W + rp.px;
        const float4 f = load_fd(P, fd, pix), g = load_grad_in(g_in, pix);
        C_fin.x.x = f.x; C_fin.y.x = f.y; C_fin.z.x = f.z; gC.x.x = g.x; gC.y.x = g.y; gC.z.x = g.z;
        T_fin.x = 1.f - f.w; gT.x = -g.w;
        if (HAS_GDIST) { D_fin.x = dist[pix]; gD.x = g_dist[pix]; }
    }
    if (alive1) {
        const size_t pix = (size_t)rp.py1 * P.W + rp.px;
        const float4 f = load_fd(P, fd, pix), g = load_grad_in(g_in, pix);
        C_fin.x.y = f.x; C_fin.y.y = f.y; C_fin.z.y = f.z; gC.x.y = g.x; gC.y.y = g.y; gC.z.y = g.z;
        T_fin.y = 1.f - f.w; gT.y = -g.w;
        if (HAS_GDIST) { D_fin.y = dist[pix]; gD.y = g_dist[pix]; }
    }
    if (from_checkpoint) {
        const size_t slot = (((size_t)boundary * 2 + half) * 64 + lane) * 2;
        // (a quarter-tile forward wave that was done before this boundary left no checkpoint: its pixels restart dead)
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 c0 = (reached_bits & 1u) ? ck.tc[slot] : zero4, c1 = (reached_bits & 2u) ? ck.tc[slot + 1] : zero4;
        T = v2f{c0.x, c1.x}; Cr = v2f{c0.y, c1.y}; Cg = v2f{c0.z, c1.z}; Cb = v2f{c0.w, c1.w};
        if (HAS_GDIST) D = v2f{(reached_bits & 1u) ? ck.d[slot] : 0.f, (reached_bits & 2u) ? ck.d[slot + 1] : 0.f};
        alive0 = alive0 && !(T.x < P.min_transmittance);
        alive1 = alive1 && !(T.y < P.min_transmittance);
    }

    BwdPixels px{T, D, Cr, Cg, Cb, T_fin, D_fin, gT, gD, C_fin, gC, alive0, alive1};
    if (rp.uniform_origin)
        render_bwd_sweep<DEG, HAS_GDIST, true, COUNT>(P, rp, seg_begin, seg_end, lane, half, lists, density12, rgb, slots, s_rec, s_acc, s_acc2, s_tr, s_who, px);
    else
        render_bwd_sweep<DEG, HAS_GDIST, false, COUNT>(P, rp, seg_begin, seg_end, lane, half, lists, density12, rgb, slots, s_rec, s_acc, s_acc2, s_tr, s_who, px);
    if (COUNT && P.work && lane == 0) {   // diagnostics (after the forward sweep's block of per-wave words): lifetime and start of this task
        const size_t gid = (size_t)atomicAdd(&P.work[8], 1ull);
        const size_t base = 16 + 4 * (size_t)(((num_tiles + 7u) & ~7u) * 2u) + 2 * gid;
        if (gid < P.work_task_capacity) {   // (the block was sized from an earlier frame's list length: records beyond it are dropped)
            P.work[base] = wall_clock64() - t_begin;
            P.work[base + 1] = t_begin;
        }
    }
}

}  // namespace

void launch_render_fwd(hipStream_t s, const GutParams& P, const uint32_t* ranges, const uint32_t* sorted_pos, const uint32_t* pos_particle,
                       const float* density12, const float* rgb, const float* ray_o, const float* ray_d, float* out_fd, float* out_dist,
                       float* out_cnt, const GutCheckpoints& ck, bool write_checkpoints) {
    const EntryLists lists = entry_lists(P, sorted_pos, pos_particle);
    if (P.work && P.degree == 2 && write_checkpoints) {   // instrumented frame (gut_profile_enable level 2): the counting build of the default kernel
        hipLaunchKernelGGL((gut_render_fwd_kernel<2, true, true>), dim3(half_grid(P)), dim3(64), 0, s, P, reinterpret_cast<const uint2*>(ranges), lists,
                           reinterpret_cast<const float4*>(density12), rgb, ray_o, ray_d, reinterpret_cast<float4*>(out_fd), out_dist, out_cnt, ck);
        return;
    }
    // when every wave of the launch is resident at once (<= 5 half-tile waves per SIMD x 1024 SIMDs) the longest wave is the kernel: quarter tiles
    const char* quarter_str = getenv("GRUT_FWD_QUARTER");   // development / test switch (read per call): 0 / 1 force, default by size
    const int quarter_env = quarter_str ? atoi(quarter_str) : -1;
    // (5 waves x 4 SIMDs per compute unit, from the device's own CU count: 5120 on the 256 CUs of an MI355X)
    static const uint32_t resident_limit = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= 0) return 5120u;
        return 20u * (uint32_t)prop.multiProcessorCount;
    }();
    const bool quarter = quarter_env >= 0 ? quarter_env != 0 : half_grid(P) <= resident_limit;
    if (quarter && !(P.work && P.degree == 2 && write_checkpoints)) {
        const dim3 grid(half_grid(P) * 2u);
        if (write_checkpoints) {
            GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_fwd_quarter_kernel<D_, true>), grid, dim3(64), 0, s, P, reinterpret_cast<const uint2*>(ranges),
                                                              lists, reinterpret_cast<const float4*>(density12), rgb, ray_o, ray_d,
                                                              reinterpret_cast<float4*>(out_fd), out_dist, out_cnt, ck));
        } else {
            GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_fwd_quarter_kernel<D_, false>), grid, dim3(64), 0, s, P, reinterpret_cast<const uint2*>(ranges),
                                                              lists, reinterpret_cast<const float4*>(density12), rgb, ray_o, ray_d,
                                                              reinterpret_cast<float4*>(out_fd), out_dist, out_cnt, ck));
        }
        return;
    }
    if (write_checkpoints) {
        GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_fwd_kernel<D_, true>), dim3(half_grid(P)), dim3(64), 0, s, P,
                                                          reinterpret_cast<const uint2*>(ranges), lists,
                                                          reinterpret_cast<const float4*>(density12), rgb, ray_o, ray_d,
                                                          reinterpret_cast<float4*>(out_fd), out_dist, out_cnt, ck));
    } else {
        GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_fwd_kernel<D_, false>), dim3(half_grid(P)), dim3(64), 0, s, P,
                                                          reinterpret_cast<const uint2*>(ranges), lists,
                                                          reinterpret_cast<const float4*>(density12), rgb, ray_o, ray_d,
                                                          reinterpret_cast<float4*>(out_fd), out_dist, out_cnt, ck));
    }
}
void launch_render_bwd(hipStream_t s, const GutParams& P, const uint32_t* ranges, const uint32_t* sorted_pos, const float* density12,
                       const float* rgb, const float* ray_o, const float* ray_d, const float* fd, const GutGradIn& g_fd, const float* dist,
                       const float* g_dist, const GutGradSlots& slots, const GutCheckpoints& ck) {
    const dim3 grid(segment_grid(P, ck.num_boundaries));
    const EntryLists lists = entry_lists(P, sorted_pos, slots.pos_particle);
    if (P.work && P.degree == 2 && !g_dist) {   // instrumented frame: the counting build of the training-path kernel
        hipLaunchKernelGGL((gut_render_bwd_kernel<2, false, true>), grid, dim3(64), 0, s, P, reinterpret_cast<const uint2*>(ranges), lists,
                           reinterpret_cast<const float4*>(density12), rgb, ray_o, ray_d, reinterpret_cast<const float4*>(fd), g_fd, dist, g_dist, slots, ck);
        return;
    }
    if (g_dist) {
        GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_bwd_kernel<D_, true>), grid, dim3(64), 0, s, P,
                                                          reinterpret_cast<const uint2*>(ranges), lists,
                                                          reinterpret_cast<const float4*>(density12), rgb, ray_o, ray_d,
                                                          reinterpret_cast<const float4*>(fd), g_fd, dist,
                                                          g_dist, slots, ck));
    } else {  // no depth gradient flows in: the hit-distance terms vanish identically
        GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_bwd_kernel<D_, false>), grid, dim3(64), 0, s, P,
                                                          reinterpret_cast<const uint2*>(ranges), lists,
                                                          reinterpret_cast<const float4*>(density12), rgb, ray_o, ray_d,
                                                          reinterpret_cast<const float4*>(fd), g_fd, dist,
                                                          g_dist, slots, ck));
    }
}

// ---------------------------------------------------------------------------------------------
// Neural harmonic features, forward (model.feature_type = nht; gutKBufferRenderer.cuh:199-225, :228-352 with PerRayParticleFeatures):
// the unsorted tile loop, but a hit's features are not a per-particle colour: they are interpolated at the hit's CANONICAL INTERSECTION
// (the point of the ray closest to the particle centre, in the particle's scaled frame; gaussianParticles.slang:181-190) from the four
// feature vectors at the vertices of the canonical tetrahedron (neuralHarmonicFeaturesParticle.slang:47-66, :117-127), passed through
// the activation (:146-196) and integrated with the hit's weight into ray_dim accumulators per pixel (:198-211).  One pixel per lane,
// one wave per 16x4 strip (the k-buffer kernels' layout); the entry's K feature floats are wave-uniform and read through the scalar
// cache.  First version: correctness first, ray_dim <= 32.
// ---------------------------------------------------------------------------------------------
constexpr int kNhtMaxRay = 32, kNhtMaxIpd = 16;
// sin / cos of the activation on the hardware's v_sin_f32 / v_cos_f32 (argument in revolutions; absolute error ~1e-6 for the |angle| < 256
// this model produces — features are initialised in [-pi/2, pi/2] and multiplied by at most the frequency index): the library sinf / cosf
// cost ~40 instructions each, 48 of them per hit and pixel made up five sixths of the first version's forward
__device__ __forceinline__ float nht_sin(float x) { return __builtin_amdgcn_sinf(__builtin_amdgcn_fractf(x * 0.15915494309189535f)); }
__device__ __forceinline__ float nht_cos(float x) { return __builtin_amdgcn_cosf(__builtin_amdgcn_fractf(x * 0.15915494309189535f)); }
__global__ __launch_bounds__(64) void gut_render_nht_fwd_kernel(GutParams P, const uint2* __restrict__ ranges, EntryLists lists,
                                                                const float4* __restrict__ density12, const float* __restrict__ features,
                                                                const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                                float* __restrict__ out_fd, float* __restrict__ out_dist, float* __restrict__ out_cnt) {
    __shared__ float4 s_rec[64 * 5];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const uint32_t tile = ((slot >> 2) << 3) + xcd, strip = slot & 3u;
    if (tile >= (uint32_t)(P.gx * P.gy)) return;
    const int lane = threadIdx.x;
    const int px = (int)(tile % P.gx) * 16 + (lane & 15);
    const int py = (int)(tile / P.gx) * 16 + (int)strip * 4 + (lane >> 4);
    const Ray ray = init_ray(P, ray_o, ray_d, px, py);
    bool alive = ray.valid;
    float T = 1.f, D = 0.f, cnt = 0.f;
    float acc[kNhtMaxRay];
#pragma unroll
    for (int i = 0; i < kNhtMaxRay; ++i) acc[i] = 0.f;
    const int ipd = P.nht_ipd, nf = P.nht_nf, nr = P.nht_ray_dim;
    // the canonical tetrahedron's Cramer terms (constants of the model)
    const float edge = 4.898979485566356f, face_h = 4.242640687119285f, face_in = 1.4142135623730951f;
    const f3 v0 = mk3(0.5f * edge, -face_in, -1.f), v1 = mk3(-0.5f * edge, -face_in, -1.f), v2 = mk3(0.f, face_h - face_in, -1.f), v3 = mk3(0.f, 0.f, 3.f);
    const f3 e1 = v1 - v0, e2 = v2 - v0, e3 = v3 - v0;
    const f3 c23 = cross(e2, e3);
    const float inv_det = 1.f / dot(e1, c23);
    const uint2 range = ranges[tile];
    for (uint32_t b = range.x; b < range.y; b += 64) {
        if (!__any(alive)) break;
        {   // stage up to 64 entries (as gut_render_k_body)
            const RawEntry e = load_entry<false>(b + lane, range.y, lists, density12, nullptr);
            float4 r0 = make_float4(1.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 1.f, 0.f, 0.f), r2 = make_float4(0.f, 0.f, 1.f, 0.f);
            float4 r3 = make_float4(1.f, 1.f, 1.f, 0.f), r4 = make_float4(__uint_as_float(0xFFFFFFFFu), 0.f, 0.f, 0.f);
            if (e.idx != 0xFFFFFFFFu) {
                const m3 rt = quat_wxyz_to_rotT(e.q.x, e.q.y, e.q.z, e.q.w);
                const float ix = 1.f / e.s.x, iy = 1.f / e.s.y, iz = 1.f / e.s.z;
                r0 = make_float4(rt.r0.x * ix, rt.r0.y * ix, rt.r0.z * ix, e.a.x);
                r1 = make_float4(rt.r1.x * iy, rt.r1.y * iy, rt.r1.z * iy, e.a.y);
                r2 = make_float4(rt.r2.x * iz, rt.r2.y * iz, rt.r2.z * iz, e.a.z);
                r3 = make_float4(e.s.x, e.s.y, e.s.z, e.a.w);
                r4.x = __uint_as_float(e.idx);
                const float need = fmaxf(P.min_response, P.min_alpha / e.a.w);
                r4.y = (P.max_alpha > P.min_alpha && e.a.w > 0.f) ? gray_limit_rt(P.degree, need) : 0.f;
            }
            float4* rec = &s_rec[lane * 5];
            rec[0] = r0; rec[1] = r1; rec[2] = r2; rec[3] = r3; rec[4] = r4;
        }
        __syncthreads();
        const int n = (int)min(64u, range.y - b);
        for (int j = 0; j < n; ++j) {
            if (!__any(alive)) break;
            const float4* rec = &s_rec[j * 5];
            const uint32_t idx = __float_as_uint(rec[4].x);
            if (idx == 0xFFFFFFFFu) break;   // padding closes the list (gutKBufferRenderer.cuh:312-315)
            bool hit = false;
            float w = 0.f;
            f3 Pc = mk3(0.f, 0.f, 0.f);
            if (alive) {
                const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
                const f3 dl = ray.o - mk3(q0.w, q1.w, q2.w);
                const f3 gro = mk3(dot(mk3(q0.x, q0.y, q0.z), dl), dot(mk3(q1.x, q1.y, q1.z), dl), dot(mk3(q2.x, q2.y, q2.z), dl));
                const f3 grdu = mk3(dot(mk3(q0.x, q0.y, q0.z), ray.d), dot(mk3(q1.x, q1.y, q1.z), ray.d), dot(mk3(q2.x, q2.y, q2.z), ray.d));
                const float l2 = dot(grdu, grdu);
                const f3 gc = cross(grdu, gro);
                const float cc = dot(gc, gc);
                if (cc < rec[4].y * l2) {   // response > min_response && alpha > min_alpha
                    const float il2 = 1.f / l2;
                    const float resp = response_rt(P.degree, cc * il2);
                    const float alpha = fminf(P.max_alpha, resp * q3.w);
                    // canonical intersection gro + grd (grd . -gro) = gro - grdu (grdu . gro) / |grdu|^2; hit distance |S (that offset)|
                    const float along = -dot(grdu, gro) * il2;
                    const f3 cg = grdu * along;
                    const f3 sv = mk3(q3.x, q3.y, q3.z) * cg;
                    const float hitT = sqrtf(dot(sv, sv));
                    if ((hitT > ray.tmin) && (hitT < ray.tmax)) {
                        w = alpha * T;
                        D = fmaf(hitT, w, D);
                        T *= (1.f - alpha);
                        hit = w > 0.f;
                        Pc = gro + cg;
                        if (hit) cnt += 1.f;
                        if (T < P.min_transmittance) alive = false;
                    }
                }
            }
            if (!__any(hit)) continue;
            // the entry's feature vectors (wave-uniform address) and this lane's barycentric weights
            const uint32_t uidx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
            float wq[4] = {1.f, 0.f, 0.f, 0.f};
            if (P.nht_support == 1) {
                const f3 d = Pc - v0;
                wq[1] = dot(d, c23) * inv_det;
                wq[2] = dot(e1, cross(d, e3)) * inv_det;
                wq[3] = dot(e1, cross(e2, d)) * inv_det;
                wq[0] = 1.f - wq[1] - wq[2] - wq[3];
            }
            const int points = P.nht_support == 1 ? 4 : 1;
            float base[kNhtMaxIpd];
#pragma unroll
            for (int m = 0; m < kNhtMaxIpd; ++m) {
                base[m] = 0.f;
                if (m < ipd) {
                    for (int k = 0; k < points; ++k) {
                        const size_t at = (size_t)uidx * P.nht_k + (size_t)k * ipd + m;
                        const float fv = P.sph_half ? __half2float(reinterpret_cast<const __half*>(features)[at]) : features[at];
                        base[m] = k == 0 ? fv * wq[0] : fmaf(wq[k], fv, base[m]);   // (:166-176: base = f0 w0, then += wk fk)
                    }
                }
            }
            if (hit) {
#pragma unroll
                for (int i = 0; i < kNhtMaxRay; ++i) {
                    if (i < nr) {
                        float f;
                        if (P.nht_act == 0) f = base[i < kNhtMaxIpd ? i : 0];
                        else if (P.nht_act == 3) f = fmaxf(0.f, base[i < kNhtMaxIpd ? i : 0]);
                        else if (P.nht_act == 2) {
                            const int k = i / (2 * nf), rem = i - k * 2 * nf, fq = rem >> 1;
                            const float angle = base[k < kNhtMaxIpd ? k : 0] * (float)(fq + 1);
                            f = (rem & 1) ? nht_cos(angle) : nht_sin(angle);
                        } else {
                            const int k = i / nf, fq = i - k * nf;
                            f = nht_sin(base[k < kNhtMaxIpd ? k : 0] * ldexpf(1.f, fq));
                        }
                        acc[i] = fmaf(f, w, acc[i]);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (ray.inside) {
        const size_t opix = (size_t)py * P.W + px;
        const size_t stride = (size_t)nr + 1;
#pragma unroll
        for (int i = 0; i < kNhtMaxRay; ++i) {
            if (i < nr) {
                const float v = ray.valid ? acc[i] : 0.f;
                if (P.out_half) reinterpret_cast<__half*>(out_fd)[opix * stride + i] = __float2half(v);
                else out_fd[opix * stride + i] = v;
            }
        }
        const float op = ray.valid ? 1.f - T : 0.f;
        if (P.out_half) reinterpret_cast<__half*>(out_fd)[opix * stride + nr] = __float2half(op);
        else out_fd[opix * stride + nr] = op;
        out_dist[opix] = ray.valid ? D : 1e6f;
        if (P.hitcounts) out_cnt[opix] = ray.valid ? cnt : 0.f;
    }
}

// Neural harmonic features, backward (evalBackwardNoKBuffer's per-ray-features branch, gutKBufferRenderer.cuh:546-641): the forward's
// sweep again, front to back, un-blending the ray state hit by hit (the reverse mode of the lerp form, like the sorted mode's backward);
// per hit and pixel the gradient of the ray features flows through the activation and the barycentric blend into (i) the particle's
// feature rows, (ii) the canonical intersection and from there, with dL/d alpha and dL/d depth, into the particle's 11 geometric terms
// (restated and checked against float64 autograd in the oracle: orc_gut_render_nht_bwd).  All 64 pixels of the strip meet a list entry
// at the same time, so the wave sums each of the entry's words over its lanes (DPP reduce-scatter, 16 words at a time) before ONE set
// of atomics per (wave, entry) — the reference does the same with warp shuffles (shRadiativeGaussianParticles.cuh:421-441).
// First version: no checkpoints (every wave sweeps its tile's list from the start), correctness first.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void gut_render_nht_bwd_kernel(GutParams P, const uint2* __restrict__ ranges, EntryLists lists,
                                                                const float4* __restrict__ density12, const float* __restrict__ features,
                                                                const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                                const float* __restrict__ fd, const float* __restrict__ g_fd,
                                                                const float* __restrict__ dist, const float* __restrict__ g_dist,
                                                                float* __restrict__ g_density12, float* __restrict__ g_features) {
    __shared__ float4 s_rec[64 * 5];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const uint32_t tile = ((slot >> 2) << 3) + xcd, strip = slot & 3u;
    if (tile >= (uint32_t)(P.gx * P.gy)) return;
    const int lane = threadIdx.x;
    const int px = (int)(tile % P.gx) * 16 + (lane & 15);
    const int py = (int)(tile / P.gx) * 16 + (int)strip * 4 + (lane >> 4);
    const Ray ray = init_ray(P, ray_o, ray_d, px, py);
    bool alive = ray.valid;
    const int ipd = P.nht_ipd, nf = P.nht_nf, nr = P.nht_ray_dim;
    const int points = P.nht_support == 1 ? 4 : 1;
    const size_t pix = ray.valid ? (size_t)py * P.W + px : 0;
    float Cb[kNhtMaxRay], gC[kNhtMaxRay];
#pragma unroll
    for (int i = 0; i < kNhtMaxRay; ++i) {
        const bool use = alive && i < nr;
        Cb[i] = use ? (P.out_half ? __half2float(reinterpret_cast<const __half*>(fd)[pix * (nr + 1) + i]) : fd[pix * (nr + 1) + i]) : 0.f;
        gC[i] = use ? g_fd[pix * (nr + 1) + i] : 0.f;
    }
    float Tb = 1.f, gT = 0.f, Db = 0.f, gD = 0.f, T = 1.f;
    if (alive) {
        const float op = P.out_half ? __half2float(reinterpret_cast<const __half*>(fd)[pix * (nr + 1) + nr]) : fd[pix * (nr + 1) + nr];
        Tb = 1.f - op; gT = -g_fd[pix * (nr + 1) + nr];
        Db = dist[pix]; gD = g_dist ? g_dist[pix] : 0.f;
    }
    const float edge = 4.898979485566356f, face_h = 4.242640687119285f, face_in = 1.4142135623730951f;
    const f3 v0 = mk3(0.5f * edge, -face_in, -1.f), v1 = mk3(-0.5f * edge, -face_in, -1.f), v2 = mk3(0.f, face_h - face_in, -1.f), v3 = mk3(0.f, 0.f, 3.f);
    const f3 e1 = v1 - v0, e2 = v2 - v0, e3 = v3 - v0;
    const f3 c23 = cross(e2, e3);
    const float inv_det = 1.f / dot(e1, c23);
    const f3 gw1 = c23 * inv_det, gw2 = cross(e3, e1) * inv_det, gw3 = cross(e1, e2) * inv_det;
    const f3 gw0 = (gw1 + gw2 + gw3) * -1.f;
    const uint2 range = ranges[tile];
    for (uint32_t b = range.x; b < range.y; b += 64) {
        if (!__any(alive)) break;
        {
            const RawEntry e = load_entry<false>(b + lane, range.y, lists, density12, nullptr);
            float4 r0 = make_float4(1.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 1.f, 0.f, 0.f), r2 = make_float4(0.f, 0.f, 1.f, 0.f);
            float4 r3 = make_float4(1.f, 1.f, 1.f, 0.f), r4 = make_float4(__uint_as_float(0xFFFFFFFFu), 0.f, 0.f, 0.f);
            if (e.idx != 0xFFFFFFFFu) {   // raw rows: the gradient chain needs the quaternion and the scale themselves
                r0 = e.a; r1 = e.q; r2 = make_float4(e.s.x, e.s.y, e.s.z, 0.f);
                r4.x = __uint_as_float(e.idx);
                const float need = fmaxf(P.min_response, P.min_alpha / e.a.w);
                r4.y = (P.max_alpha > P.min_alpha && e.a.w > 0.f) ? gray_limit_rt(P.degree, need) : 0.f;
            }
            float4* rec = &s_rec[lane * 5];
            rec[0] = r0; rec[1] = r1; rec[2] = r2; rec[3] = r3; rec[4] = r4;
        }
        __syncthreads();
        const int n = (int)min(64u, range.y - b);
        for (int j = 0; j < n; ++j) {
            if (!__any(alive)) break;
            const float4* rec = &s_rec[j * 5];
            const uint32_t idx = __float_as_uint(rec[4].x);
            if (idx == 0xFFFFFFFFu) break;
            const float4 a = rec[0], q = rec[1], sc = rec[2];
            bool hit = false;
            float gd[16], gbase[kNhtMaxIpd], wq[4] = {1.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 16; ++k) gd[k] = 0.f;
#pragma unroll
            for (int m = 0; m < kNhtMaxIpd; ++m) gbase[m] = 0.f;
            if (alive) {
                const m3 rotT = quat_wxyz_to_rotT(q.x, q.y, q.z, q.w);
                const f3 gscl = mk3(sc.x, sc.y, sc.z), giscl = mk3(1.f / sc.x, 1.f / sc.y, 1.f / sc.z);
                const f3 gposc = ray.o - mk3(a.x, a.y, a.z);
                const f3 gposcr = mul_rows(rotT, gposc);
                const f3 gro = giscl * gposcr;
                const f3 rdr = mul_rows(rotT, ray.d);
                const f3 grdu = giscl * rdr;
                const float l2 = dot(grdu, grdu);
                const float il = 1.f / sqrtf(l2);
                const f3 grd = grdu * il;
                const f3 gcrod = cross(grd, gro);
                const float gray = dot(gcrod, gcrod);
                if (gray < rec[4].y) {
                    const float gres = response_rt(P.degree, gray);
                    const float alpha = fminf(P.max_alpha, gres * a.w);
                    const float pdot = -dot(grd, gro);
                    const f3 grdd = grd * pdot;
                    const f3 Pc = gro + grdd;
                    const f3 grds = gscl * grdd;
                    const float gsq = dot(grds, grds);
                    const float hitT = sqrtf(gsq);
                    if ((hitT > ray.tmin) && (hitT < ray.tmax)) {
                        hit = alpha > 0.f;
                        if (P.nht_support == 1) {
                            const f3 d = Pc - v0;
                            wq[1] = dot(d, c23) * inv_det; wq[2] = dot(e1, cross(d, e3)) * inv_det; wq[3] = dot(e1, cross(e2, d)) * inv_det;
                            wq[0] = 1.f - wq[1] - wq[2] - wq[3];
                        }
                        float base[kNhtMaxIpd];
#pragma unroll
                        for (int m = 0; m < kNhtMaxIpd; ++m) {
                            base[m] = 0.f;
                            if (m < ipd)
                                for (int k = 0; k < points; ++k) {
                                    const size_t at = (size_t)idx * P.nht_k + (size_t)k * ipd + m;
                                    const float fv = P.sph_half ? __half2float(reinterpret_cast<const __half*>(features)[at]) : features[at];
                                    base[m] = k == 0 ? fv * wq[0] : fmaf(wq[k], fv, base[m]);
                                }
                        }
                        const float w = 1.f / (1.f - alpha);
                        float dalpha = 0.f;
#pragma unroll
                        for (int i = 0; i < kNhtMaxRay; ++i) {
                            if (i < nr) {
                                // feature i and d feature i / d base (sincos: index k*nf*2 + f*2 + {0,1}; siren: k*nf + f)
                                float f, df;
                                int kb;
                                if (P.nht_act == 0) { kb = i; f = base[kb < kNhtMaxIpd ? kb : 0]; df = 1.f; }
                                else if (P.nht_act == 3) { kb = i; const float bv = base[kb < kNhtMaxIpd ? kb : 0]; f = fmaxf(0.f, bv); df = bv > 0.f ? 1.f : 0.f; }
                                else if (P.nht_act == 2) {
                                    kb = i / (2 * nf);
                                    const int rem = i - kb * 2 * nf, fq = rem >> 1;
                                    const float fr = (float)(fq + 1), ang = base[kb < kNhtMaxIpd ? kb : 0] * fr;
                                    const float sn = nht_sin(ang), cs = nht_cos(ang);
                                    f = (rem & 1) ? cs : sn; df = (rem & 1) ? -fr * sn : fr * cs;
                                } else {
                                    kb = i / nf;
                                    const float fr = ldexpf(1.f, i - kb * nf), ang = base[kb < kNhtMaxIpd ? kb : 0] * fr;
                                    f = nht_sin(ang); df = fr * nht_cos(ang);
                                }
                                if (hit) {
                                    Cb[i] = (Cb[i] - f * alpha) * w;
                                    dalpha = fmaf(f - Cb[i], gC[i], dalpha);
                                    const float gf = alpha * gC[i];
                                    gC[i] *= (1.f - alpha);
#pragma unroll
                                    for (int m = 0; m < kNhtMaxIpd; ++m)
                                        if (m == kb) gbase[m] = fmaf(df, gf, gbase[m]);
                                }
                            }
                        }
                        // blend backward: the canonical position's gradient (the feature rows' gradient is wq[k] * gbase, summed over the wave below)
                        f3 dP = mk3(0.f, 0.f, 0.f);
                        if (P.nht_support == 1 && hit) {
                            float dw[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                            for (int m = 0; m < kNhtMaxIpd; ++m)
                                if (m < ipd)
                                    for (int k = 0; k < 4; ++k) {
                                        const size_t at = (size_t)idx * P.nht_k + (size_t)k * ipd + m;
                                        const float fv = P.sph_half ? __half2float(reinterpret_cast<const __half*>(features)[at]) : features[at];
                                        dw[k] = fmaf(fv, gbase[m], dw[k]);
                                    }
                            dP = gw0 * dw[0] + gw1 * dw[1] + gw2 * dw[2] + gw3 * dw[3];
                        }
                        // density: T_out = T_in (1 - alpha), D_front = lerp(D_behind, depth, alpha)
                        Tb *= w;
                        Db = (Db - hitT * alpha) * w;
                        dalpha += (hitT - Db) * gD - Tb * gT;
                        const float ddepth = alpha * gD;
                        gD *= (1.f - alpha);
                        gT *= (1.f - alpha);
                        if (hit) {
                            float dres = 0.f, ddens = 0.f;
                            if (gres * a.w < P.max_alpha) { dres = a.w * dalpha; ddens = gres * dalpha; }
                            const float grayGrd = response_grd_rt(P.degree, gray, gres, dres);
                            const f3 grdsGrd = gsq > 0.f ? grds * (ddepth / hitT) : mk3(0.f, 0.f, 0.f);
                            const f3 gsclHit = grdd * grdsGrd;
                            const float sdot = dot(grdsGrd * gscl, grd);
                            const float gdP = dot(grd, dP);
                            const f3 grdHit = gscl * grdsGrd * pdot - gro * sdot + dP * pdot - gro * gdP;
                            const f3 groHit = grd * (-sdot) + dP - grd * gdP;
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
                            gd[0] = -gposcGrd.x; gd[1] = -gposcGrd.y; gd[2] = -gposcGrd.z; gd[3] = ddens;
                            gd[4] = gq1.x + gq2.x; gd[5] = gq1.y + gq2.y; gd[6] = gq1.z + gq2.z; gd[7] = gq1.w + gq2.w;
                            gd[8] = sclGrd.x; gd[9] = sclGrd.y; gd[10] = sclGrd.z;
                        }
                        T *= (1.f - alpha);
                        if (T < P.min_transmittance) alive = false;
                    }
                }
            }
            if (!__any(hit)) continue;
            // one set of atomics per (wave, entry): 11 geometric words, then the feature rows point by point
            const float tot = wave_reduce_scatter16(gd, lane);
            if (lane < 11) atomicAdd(g_density12 + 12 * (size_t)idx + lane, tot);
            for (int k = 0; k < points; ++k) {
                float gfk[16];
#pragma unroll
                for (int m = 0; m < 16; ++m) gfk[m] = (hit && m < ipd) ? wq[k] * gbase[m < kNhtMaxIpd ? m : 0] : 0.f;
                const float t2 = wave_reduce_scatter16(gfk, lane);
                if (lane < ipd) atomicAdd(g_features + (size_t)idx * P.nht_k + (size_t)k * ipd + lane, t2);
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Neural harmonic features behind the SORTED hit buffer (render.splat.k_buffer_size > 0 with model.feature_type = nht; round 6):
// gutKBufferRenderer.cuh:273-352 (evalKBuffer) with Params::PerRayParticleFeatures - processHitParticle :158-225 integrates, per popped hit,
// the features interpolated at the hit's canonical intersection.  The tile loop, the hit test, the hit distance in the checker's operation
// order (it is the buffer's sort key) and the buffer itself are gut_render_k_body's; a popped hit is a (particle, alpha, distance) triple,
// everything else the feature integration needs - the canonical intersection, the response for the gradient chain - is a function of
// (ray, particle) and is evaluated again at the pop from the particle's own rows (the reference keeps the intersection in the buffer: the
// same value).  The gradients leave per lane and hit with atomics, like the reference's (featuresIntegrateBwdToBuffer /
// densityProcessHitBwdToBuffer); the per-hit arithmetic is the unsorted strip kernels' above, hit by hit.
// ---------------------------------------------------------------------------------------------
struct NhtTetra4 { f3 v0, e1, e2, e3, c23, gw0, gw1, gw2, gw3; float inv_det; };
__device__ __forceinline__ NhtTetra4 nht_tetra4() {
    NhtTetra4 t;
    const float edge = 4.898979485566356f, face_h = 4.242640687119285f, face_in = 1.4142135623730951f;
    const f3 v1 = mk3(-0.5f * edge, -face_in, -1.f), v2 = mk3(0.f, face_h - face_in, -1.f), v3 = mk3(0.f, 0.f, 3.f);
    t.v0 = mk3(0.5f * edge, -face_in, -1.f);
    t.e1 = v1 - t.v0; t.e2 = v2 - t.v0; t.e3 = v3 - t.v0;
    t.c23 = cross(t.e2, t.e3);
    t.inv_det = 1.f / dot(t.e1, t.c23);
    t.gw1 = t.c23 * t.inv_det; t.gw2 = cross(t.e3, t.e1) * t.inv_det; t.gw3 = cross(t.e1, t.e2) * t.inv_det;
    t.gw0 = (t.gw1 + t.gw2 + t.gw3) * -1.f;
    return t;
}
__device__ __forceinline__ float nht_feature_word(const GutParams& P, const float* __restrict__ features, uint32_t idx, int word) {
    const size_t at = (size_t)idx * P.nht_k + word;
    return P.sph_half ? __half2float(reinterpret_cast<const __half*>(features)[at]) : features[at];
}
// a popped hit's particle is the lane's own: its feature row is gathered per lane.  The default model's row (48 floats = 4 vertices x 12,
// fp32) comes as twelve 16-byte loads instead of 48 single words (the first version's forward spent most of its time issuing them)
__host__ __device__ __forceinline__ bool nht_row48(const GutParams& P) { return P.nht_k == 48 && P.nht_ipd == 12 && P.nht_support == 1 && !P.sph_half; }
__device__ __forceinline__ void nht_row_blend(const GutParams& P, const float* __restrict__ features, uint32_t idx, const float (&wq)[4], float (&base)[kNhtMaxIpd]) {
    const int points = P.nht_support == 1 ? 4 : 1, ipd = P.nht_ipd;
#pragma unroll
    for (int m = 0; m < kNhtMaxIpd; ++m) base[m] = 0.f;
    if (nht_row48(P)) {
        const float4* src = reinterpret_cast<const float4*>(features + (size_t)idx * 48);
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const float4 v = src[q];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                constexpr int kIpd = 12;
                const int w = 4 * q + c, k = w / kIpd, m = w - k * kIpd;
                base[m] = k == 0 ? e[c] * wq[0] : fmaf(wq[k], e[c], base[m]);   // (base = f0 w0, then += wk fk: the strip kernels' order)
            }
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < kNhtMaxIpd; ++m)
        if (m < ipd)
            for (int k = 0; k < points; ++k) {
                const float fv = nht_feature_word(P, features, idx, k * ipd + m);
                base[m] = k == 0 ? fv * wq[0] : fmaf(wq[k], fv, base[m]);
            }
}
// dw[k] = sum_m F[k][m] gbase[m]: the barycentric weights' gradients
__device__ __forceinline__ void nht_row_dots(const GutParams& P, const float* __restrict__ features, uint32_t idx, const float (&gbase)[kNhtMaxIpd], float (&dw)[4]) {
    const int points = P.nht_support == 1 ? 4 : 1, ipd = P.nht_ipd;
    dw[0] = dw[1] = dw[2] = dw[3] = 0.f;
    if (nht_row48(P)) {
        const float4* src = reinterpret_cast<const float4*>(features + (size_t)idx * 48);
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            const float4 v = src[q];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                constexpr int kIpd = 12;
                const int w = 4 * q + c, k = w / kIpd, m = w - k * kIpd;
                dw[k] = fmaf(e[c], gbase[m], dw[k]);
            }
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < kNhtMaxIpd; ++m)
        if (m < ipd)
            for (int k = 0; k < points; ++k) dw[k] = fmaf(nht_feature_word(P, features, idx, k * ipd + m), gbase[m], dw[k]);
}
// feature i of the activation and its derivative with respect to its base feature kb (the unsorted strip kernels' rules)
__device__ __forceinline__ void nht_activation_rt(const GutParams& P, const float (&base)[kNhtMaxIpd], int i, float& f, float& df, int& kb) {
    const int nf = P.nht_nf;
    if (P.nht_act == 0) { kb = i; f = base[kb < kNhtMaxIpd ? kb : 0]; df = 1.f; }
    else if (P.nht_act == 3) { kb = i; const float bv = base[kb < kNhtMaxIpd ? kb : 0]; f = fmaxf(0.f, bv); df = bv > 0.f ? 1.f : 0.f; }
    else if (P.nht_act == 2) {
        kb = i / (2 * nf);
        const int rem = i - kb * 2 * nf, fq = rem >> 1;
        const float fr = (float)(fq + 1), ang = base[kb < kNhtMaxIpd ? kb : 0] * fr;
        const float sn = nht_sin(ang), cs = nht_cos(ang);
        f = (rem & 1) ? cs : sn; df = (rem & 1) ? -fr * sn : fr * cs;
    } else {
        kb = i / nf;
        const float fr = ldexpf(1.f, i - kb * nf), ang = base[kb < kNhtMaxIpd ? kb : 0] * fr;
        f = nht_sin(ang); df = fr * nht_cos(ang);
    }
}
struct NhtKFwdState { float T, D, cnt; float acc[kNhtMaxRay]; };
// FAST: the default feature model (48 = 4 x 12 fp32 floats, sincos with one frequency -> 24 ray features) as compile-time constants - the
// arrays shrink to what it uses and a base feature's sine and cosine are evaluated once for its two ray features (446 VGPRs -> see obj_resources)
template <bool FAST>
__device__ __forceinline__ void nht_k_pop_fwd(const GutParams& P, const Ray& ray, const NhtTetra4& tet, const float4* __restrict__ density12,
                                              const float* __restrict__ features, float hitT, float alpha, uint32_t idx, NhtKFwdState& s, bool& alive) {
    const float w = alpha * s.T;
    s.D = fmaf(hitT, w, s.D);
    s.T *= (1.f - alpha);
    if (w > 0.f) {
        const float4 a = density12[3 * (size_t)idx], q = density12[3 * (size_t)idx + 1], sc = density12[3 * (size_t)idx + 2];
        const m3 rt = quat_wxyz_to_rotT(q.x, q.y, q.z, q.w);
        const f3 giscl = mk3(1.f / sc.x, 1.f / sc.y, 1.f / sc.z);
        const f3 gro = giscl * mul_rows(rt, ray.o - mk3(a.x, a.y, a.z));
        const f3 grdu = giscl * mul_rows(rt, ray.d);
        const float along = -dot(grdu, gro) / dot(grdu, grdu);
        const f3 Pc = gro + grdu * along;
        float wq[4] = {1.f, 0.f, 0.f, 0.f};
        if (P.nht_support == 1) {
            const f3 d = Pc - tet.v0;
            wq[1] = dot(d, tet.c23) * tet.inv_det; wq[2] = dot(tet.e1, cross(d, tet.e3)) * tet.inv_det; wq[3] = dot(tet.e1, cross(tet.e2, d)) * tet.inv_det;
            wq[0] = 1.f - wq[1] - wq[2] - wq[3];
        }
        const int nr = P.nht_ray_dim;
        float base[kNhtMaxIpd];
        nht_row_blend(P, features, idx, wq, base);
        if (FAST) {
#pragma unroll
            for (int m = 0; m < 12; ++m) {
                s.acc[2 * m] = fmaf(nht_sin(base[m]), w, s.acc[2 * m]);
                s.acc[2 * m + 1] = fmaf(nht_cos(base[m]), w, s.acc[2 * m + 1]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < kNhtMaxRay; ++i) {
                if (i < nr) {
                    float f, df; int kb;
                    nht_activation_rt(P, base, i, f, df, kb);
                    s.acc[i] = fmaf(f, w, s.acc[i]);
                }
            }
        }
        s.cnt += 1.f;
    }
    if (s.T < P.min_transmittance) alive = false;
}
struct NhtKBwdState { float Cb[kNhtMaxRay], gC[kNhtMaxRay], Tb, gT, Db, gD, T; };
// returns whether the hit carries gradients; gd = its 11 geometric words, wq / gbase = the factors of its feature-row words (wq[k] * gbase[m])
template <bool FAST>
__device__ __forceinline__ bool nht_k_pop_bwd(const GutParams& P, const Ray& ray, const NhtTetra4& tet, const float4* __restrict__ density12,
                                              const float* __restrict__ features, float hitT, float alpha, uint32_t idx, NhtKBwdState& s, bool& alive,
                                              float (&gd)[11], float (&wq)[4], float (&gbase)[kNhtMaxIpd]) {
    const int points = P.nht_support == 1 ? 4 : 1, ipd = P.nht_ipd, nr = P.nht_ray_dim;
    const float4 a = density12[3 * (size_t)idx], q = density12[3 * (size_t)idx + 1], sc = density12[3 * (size_t)idx + 2];
    const m3 rotT = quat_wxyz_to_rotT(q.x, q.y, q.z, q.w);
    const f3 gscl = mk3(sc.x, sc.y, sc.z), giscl = mk3(1.f / sc.x, 1.f / sc.y, 1.f / sc.z);
    const f3 gposc = ray.o - mk3(a.x, a.y, a.z);
    const f3 gposcr = mul_rows(rotT, gposc);
    const f3 gro = giscl * gposcr;
    const f3 rdr = mul_rows(rotT, ray.d);
    const f3 grdu = giscl * rdr;
    const float l2 = dot(grdu, grdu);
    const float il = 1.f / sqrtf(l2);
    const f3 grd = grdu * il;
    const f3 gcrod = cross(grd, gro);
    const float gray = dot(gcrod, gcrod);
    const float gres = response_rt(P.degree, gray);
    const float pdot = -dot(grd, gro);
    const f3 grdd = grd * pdot;
    const f3 Pc = gro + grdd;
    const f3 grds = gscl * grdd;
    const float gsq = dot(grds, grds);
    const bool hit = alpha > 0.f;
    wq[0] = 1.f; wq[1] = 0.f; wq[2] = 0.f; wq[3] = 0.f;
#pragma unroll
    for (int k = 0; k < 11; ++k) gd[k] = 0.f;
    if (P.nht_support == 1) {
        const f3 d = Pc - tet.v0;
        wq[1] = dot(d, tet.c23) * tet.inv_det; wq[2] = dot(tet.e1, cross(d, tet.e3)) * tet.inv_det; wq[3] = dot(tet.e1, cross(tet.e2, d)) * tet.inv_det;
        wq[0] = 1.f - wq[1] - wq[2] - wq[3];
    }
    float base[kNhtMaxIpd];
    nht_row_blend(P, features, idx, wq, base);
#pragma unroll
    for (int m = 0; m < kNhtMaxIpd; ++m) gbase[m] = 0.f;
    const float w = 1.f / (1.f - alpha);
    float dalpha = 0.f;
    if (hit && FAST) {
#pragma unroll
        for (int m = 0; m < 12; ++m) {
            const float sn = nht_sin(base[m]), cs = nht_cos(base[m]);
#pragma unroll
            for (int h = 0; h < 2; ++h) {   // ray features 2 m (sine) and 2 m + 1 (cosine), in this order like the generic loop
                const int i = 2 * m + h;
                const float f = h ? cs : sn, df = h ? -sn : cs;
                s.Cb[i] = (s.Cb[i] - f * alpha) * w;
                dalpha = fmaf(f - s.Cb[i], s.gC[i], dalpha);
                const float gf = alpha * s.gC[i];
                s.gC[i] *= (1.f - alpha);
                gbase[m] = fmaf(df, gf, gbase[m]);
            }
        }
    } else if (hit) {
#pragma unroll
        for (int i = 0; i < kNhtMaxRay; ++i) {
            if (i < nr) {
                float f, df; int kb;
                nht_activation_rt(P, base, i, f, df, kb);
                s.Cb[i] = (s.Cb[i] - f * alpha) * w;
                dalpha = fmaf(f - s.Cb[i], s.gC[i], dalpha);
                const float gf = alpha * s.gC[i];
                s.gC[i] *= (1.f - alpha);
#pragma unroll
                for (int m = 0; m < kNhtMaxIpd; ++m)
                    if (m == kb) gbase[m] = fmaf(df, gf, gbase[m]);
            }
        }
    }
    // blend backward: the canonical position (the feature rows' words wq[k] * gbase[m] leave through nht_k_bwd_flush)
    f3 dP = mk3(0.f, 0.f, 0.f);
    if (hit && P.nht_support == 1) {
        float dw[4];
        nht_row_dots(P, features, idx, gbase, dw);
        dP = tet.gw0 * dw[0] + tet.gw1 * dw[1] + tet.gw2 * dw[2] + tet.gw3 * dw[3];
    }
    // density: T_out = T_in (1 - alpha), D_front = lerp(D_behind, depth, alpha)
    s.Tb *= w;
    s.Db = (s.Db - hitT * alpha) * w;
    dalpha += (hitT - s.Db) * s.gD - s.Tb * s.gT;
    const float ddepth = alpha * s.gD;
    s.gD *= (1.f - alpha);
    s.gT *= (1.f - alpha);
    if (hit) {
        float dres = 0.f, ddens = 0.f;
        if (gres * a.w < P.max_alpha) { dres = a.w * dalpha; ddens = gres * dalpha; }
        const float grayGrd = response_grd_rt(P.degree, gray, gres, dres);
        const f3 grdsGrd = gsq > 0.f ? grds * (ddepth / hitT) : mk3(0.f, 0.f, 0.f);
        const f3 gsclHit = grdd * grdsGrd;
        const float sdot = dot(grdsGrd * gscl, grd);
        const float gdP = dot(grd, dP);
        const f3 grdHit = gscl * grdsGrd * pdot - gro * sdot + dP * pdot - gro * gdP;
        const f3 groHit = grd * (-sdot) + dP - grd * gdP;
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
        gd[0] = -gposcGrd.x; gd[1] = -gposcGrd.y; gd[2] = -gposcGrd.z; gd[3] = ddens;
        gd[4] = gq1.x + gq2.x; gd[5] = gq1.y + gq2.y; gd[6] = gq1.z + gq2.z; gd[7] = gq1.w + gq2.w;
        gd[8] = sclGrd.x; gd[9] = sclGrd.y; gd[10] = sclGrd.z;
    }
    s.T *= (1.f - alpha);
    if (s.T < P.min_transmittance) alive = false;
    return hit;
}
// The gradients of a step's popped hits, hit-major through LDS (k_bwd_flush_lds / the 3DGRT feature replay): every popping lane parks its 11
// geometric words, 4 barycentric weights and <= 16 base-feature gradients; per DISTINCT particle of the step the lanes ARE the words of its
// rows - feature word (k, m) = sum over the member lanes of wq[k] * gbase[m], then the 11 geometric words - and leave as one atomic
// instruction per 64 consecutive words.  (Per-lane atomics of all 59 words, the reference's own scheme and this kernel's first version: 644 ms
// for the 1 M / 1080p backward.)
constexpr int kNhtKTermStride = 33;
template <bool FAST>
__device__ __forceinline__ void nht_k_bwd_flush(const GutParams& P, bool have, uint32_t idx, const float (&gd)[11], const float (&wq)[4],
                                                const float (&gbase)[kNhtMaxIpd], int lane, float* __restrict__ s_terms, float* __restrict__ g_density12,
                                                float* __restrict__ g_features) {
    if (have) {
        float* tw = s_terms + lane * kNhtKTermStride;
#pragma unroll
        for (int k = 0; k < 11; ++k) tw[k] = gd[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) tw[11 + k] = wq[k];
#pragma unroll
        for (int m = 0; m < (FAST ? 12 : kNhtMaxIpd); ++m) tw[15 + m] = gbase[m];
    }
    __syncthreads();   // single-wave workgroup: orders the LDS hand-off
    const int points = FAST ? 4 : (P.nht_support == 1 ? 4 : 1), ipd = FAST ? 12 : P.nht_ipd, words = points * ipd;
    unsigned long long m = __ballot(have);
    while (m) {
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t pid = (uint32_t)__builtin_amdgcn_readlane((int)idx, leader);
        const unsigned long long same = __ballot(have && idx == pid);
        m &= ~same;
        for (int chunk = 0; chunk < words; chunk += 64) {
            const int word = chunk + lane;
            const int kq = word < words ? word / ipd : 0, nq = word < words ? word - kq * ipd : 0;
            float v = 0.f;
            for (unsigned long long r = same; r; r &= r - 1) {
                const float* tw = s_terms + (__ffsll((long long)r) - 1) * kNhtKTermStride;
                v = fmaf(tw[11 + kq], tw[15 + nq], v);
            }
            if (word < words && v != 0.f) atomicAdd(g_features + (size_t)pid * P.nht_k + word, v);
        }
        float v = 0.f;
        for (unsigned long long r = same; r; r &= r - 1) v += s_terms[(__ffsll((long long)r) - 1) * kNhtKTermStride + (lane < 11 ? lane : 0)];
        if (lane < 11 && v != 0.f) atomicAdd(g_density12 + 12 * (size_t)pid + lane, v);
    }
    __syncthreads();   // the next step overwrites s_terms
}
#ifndef GRUT_NHT_K_WAVES
#define GRUT_NHT_K_WAVES 2   // the default model's instantiations are held to two waves per SIMD (256 VGPRs): forward K = 16 259 -> 256
#endif
template <int K, bool BWD, bool FAST>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FAST ? GRUT_NHT_K_WAVES : 1, 8))) void gut_render_nht_k_kernel(GutParams P, const uint2* __restrict__ ranges, EntryLists lists,
                                                              const float4* __restrict__ density12, const float* __restrict__ features,
                                                              const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                              float* __restrict__ fd /* BWD: the forward's image (read) */, float* __restrict__ dist,
                                                              float* __restrict__ out_cnt, const float* __restrict__ g_fd, const float* __restrict__ g_dist,
                                                              float* __restrict__ g_density12, float* __restrict__ g_features) {
    constexpr int kQ = 8;   // as gut_render_k_body: 0-2 M rows | pos, 3 scale | density, 4 particle | accept limit, 5-7 rows of R^T | 1 / scale
    __shared__ float4 s_rec[64 * kQ];
    __shared__ float s_kterms[BWD ? 64 * kNhtKTermStride : 1];
    const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
    const uint32_t tile = ((slot >> 2) << 3) + xcd, strip = slot & 3u;
    if (tile >= (uint32_t)(P.gx * P.gy)) return;
    const int lane = threadIdx.x;
    const int px = (int)(tile % P.gx) * 16 + (lane & 15);
    const int py = (int)(tile / P.gx) * 16 + (int)strip * 4 + (lane >> 4);
    const Ray ray = init_ray(P, ray_o, ray_d, px, py);
    bool alive = ray.valid;
    const size_t pix = ray.valid ? (size_t)py * P.W + px : 0;
    const int nr = FAST ? 24 : P.nht_ray_dim;
    const NhtTetra4 tet = nht_tetra4();
    NhtKFwdState fs;
    NhtKBwdState bs;
    if (!BWD) {
        fs.T = 1.f; fs.D = 0.f; fs.cnt = 0.f;
#pragma unroll
        for (int i = 0; i < (FAST ? 24 : kNhtMaxRay); ++i) fs.acc[i] = 0.f;
    } else {
#pragma unroll
        for (int i = 0; i < (FAST ? 24 : kNhtMaxRay); ++i) {
            const bool use = alive && i < nr;
            bs.Cb[i] = use ? (P.out_half ? __half2float(reinterpret_cast<const __half*>(fd)[pix * (nr + 1) + i]) : fd[pix * (nr + 1) + i]) : 0.f;
            bs.gC[i] = use ? g_fd[pix * (nr + 1) + i] : 0.f;
        }
        bs.Tb = 1.f; bs.gT = 0.f; bs.Db = 0.f; bs.gD = 0.f; bs.T = 1.f;
        if (alive) {
            const float op = P.out_half ? __half2float(reinterpret_cast<const __half*>(fd)[pix * (nr + 1) + nr]) : fd[pix * (nr + 1) + nr];
            bs.Tb = 1.f - op; bs.gT = -g_fd[pix * (nr + 1) + nr];
            bs.Db = dist[pix]; bs.gD = g_dist ? g_dist[pix] : 0.f;
        }
    }
    KBuffer<K> kb;
    kb.clear();
    const uint2 range = ranges[tile];
    for (uint32_t b = range.x; b < range.y; b += 64) {
        if (!__any(alive)) break;
        {   // stage up to 64 entries (gut_render_k_body)
            const RawEntry e = load_entry<false>(b + lane, range.y, lists, density12, nullptr);
            float4 r0 = make_float4(1.f, 0.f, 0.f, 0.f), r1 = make_float4(0.f, 1.f, 0.f, 0.f), r2 = make_float4(0.f, 0.f, 1.f, 0.f);
            float4 r3 = make_float4(1.f, 1.f, 1.f, 0.f), r4 = make_float4(__uint_as_float(0xFFFFFFFFu), 0.f, 0.f, 0.f);
            float4 r5 = r0, r6 = r1, r7 = r2;
            if (e.idx != 0xFFFFFFFFu) {
                {
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
            if (idx == 0xFFFFFFFFu) break;
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
                if (cc < rec[4].y * l2) {
                    const float il2 = __builtin_amdgcn_rcpf(l2);
                    const float resp = response_rt(P.degree, cc * il2);
                    const float alpha = fminf(P.max_alpha, resp * q3.w);
                    const float4 q5 = rec[5], q6 = rec[6], q7 = rec[7];
                    const float hitT = oracle_order_hit_t(ray, mk3(q0.w, q1.w, q2.w), mk3(q3.x, q3.y, q3.z), mk3(q5.x, q5.y, q5.z), mk3(q6.x, q6.y, q6.z),
                                                          mk3(q7.x, q7.y, q7.z), mk3(q5.w, q6.w, q7.w));
                    if ((hitT > ray.tmin) && (hitT < ray.tmax)) {
                        if (kb.num == K) {
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
                if (__any(pop)) {   // wave-level: the popped hits' gradients leave hit-major, lanes that popped the same particle together
                    float gd[11], wq[4], gbase[kNhtMaxIpd];
                    const bool have = pop && nht_k_pop_bwd<FAST>(P, ray, tet, density12, features, pop_t, pop_a, pop_i, bs, alive, gd, wq, gbase);
                    nht_k_bwd_flush<FAST>(P, have, pop_i, gd, wq, gbase, lane, s_kterms, g_density12, g_features);
                }
            } else if (pop) {
                nht_k_pop_fwd<FAST>(P, ray, tet, density12, features, pop_t, pop_a, pop_i, fs, alive);
            }
        }
        __syncthreads();
    }
    // drain what is left, nearest first (:343-351), as gut_render_k_body
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
                float gd[11], wq[4], gbase[kNhtMaxIpd];
                const bool have = act && nht_k_pop_bwd<FAST>(P, ray, tet, density12, features, t0, a0, i0, bs, alive, gd, wq, gbase);
                nht_k_bwd_flush<FAST>(P, have, i0, gd, wq, gbase, lane, s_kterms, g_density12, g_features);
            }
        } else if (act) {
            nht_k_pop_fwd<FAST>(P, ray, tet, density12, features, t0, a0, i0, fs, alive);
        }
    }
    if (!BWD && ray.inside) {
        const size_t opix = (size_t)py * P.W + px;
        const size_t stride = (size_t)nr + 1;
#pragma unroll
        for (int i = 0; i < (FAST ? 24 : kNhtMaxRay); ++i) {
            if (i < nr) {
                const float v = ray.valid ? fs.acc[i] : 0.f;
                if (P.out_half) reinterpret_cast<__half*>(fd)[opix * stride + i] = __float2half(v);
                else fd[opix * stride + i] = v;
            }
        }
        const float op = ray.valid ? 1.f - fs.T : 0.f;
        if (P.out_half) reinterpret_cast<__half*>(fd)[opix * stride + nr] = __float2half(op);
        else fd[opix * stride + nr] = op;
        dist[opix] = ray.valid ? fs.D : 1e6f;
        if (P.hitcounts) out_cnt[opix] = ray.valid ? fs.cnt : 0.f;
    }
}

#include "gut_render_nht.inl"

bool nht_fast_path(const GutParams& P) {
    const bool generic = getenv("GRUT_NHT_GENERIC") != nullptr;   // (development / test switch, read per call: the strip kernels for every shape)
    return P.nht && !generic && P.nht_k == kNhtK && P.nht_ipd == kNhtIpd && P.nht_support == 1 && P.nht_act == 2 && P.nht_nf == 1 && P.k_buffer == 0;
}
uint64_t nht_checkpoint_bytes(uint32_t num_boundaries) {   // (num_boundaries counts kGutSegment boundaries; the feature sweeps use every kNhtSegment-th entry)
    return ((uint64_t)nht_boundaries(num_boundaries) + 1u) * 2u * kNhtCkQuads * 64u * sizeof(float4);
}
void launch_render_nhtp_fwd(hipStream_t s, const GutParams& P, const uint32_t* ranges, const uint32_t* sorted_pos, const uint32_t* pos_particle,
                            const float* density12, const float* features, const float* ray_o, const float* ray_d, float* out_fd, float* out_dist,
                            float* out_cnt, void* ck_nht, const GutCheckpoints& ck, bool write_checkpoints) {
    const EntryLists lists = entry_lists(P, sorted_pos, pos_particle);
    if (write_checkpoints && ck_nht) {
        GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_nhtp_fwd_kernel<D_, true>), dim3(half_grid(P)), dim3(64), 0, s, P,
                                                          reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12),
                                                          features, ray_o, ray_d, out_fd, out_dist, out_cnt, reinterpret_cast<float4*>(ck_nht), ck));
    } else {
        GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_nhtp_fwd_kernel<D_, false>), dim3(half_grid(P)), dim3(64), 0, s, P,
                                                          reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12),
                                                          features, ray_o, ray_d, out_fd, out_dist, out_cnt, reinterpret_cast<float4*>(ck_nht), ck));
    }
}
void launch_render_nhtp_bwd(hipStream_t s, const GutParams& P, const uint32_t* ranges, const uint32_t* sorted_pos, const float* density12,
                            const float* features, const float* ray_o, const float* ray_d, const float* fd, const float* g_fd, const float* g_feat,
                            const float* g_opa, const float* dist, const float* g_dist, const GutGradSlots& slots, float* g_features,
                            const void* ck_nht, const GutCheckpoints& ck) {
    const dim3 grid(segment_grid(P, nht_boundaries(ck.num_boundaries)));
    const EntryLists lists = entry_lists(P, sorted_pos, slots.pos_particle);
    const NhtGradIn g_in{g_fd, g_feat, g_opa};
    if (g_dist) {
        GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_nhtp_bwd_kernel<D_, true>), grid, dim3(64), 0, s, P,
                                                          reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12),
                                                          features, ray_o, ray_d, fd, g_in, dist, g_dist, slots, g_features,
                                                          reinterpret_cast<const float4*>(ck_nht), ck));
    } else {
        GRUT_DISPATCH_DEGREE(P.degree, hipLaunchKernelGGL((gut_render_nhtp_bwd_kernel<D_, false>), grid, dim3(64), 0, s, P,
                                                          reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12),
                                                          features, ray_o, ray_d, fd, g_in, dist, g_dist, slots, g_features,
                                                          reinterpret_cast<const float4*>(ck_nht), ck));
    }
}
void launch_render_nht_fwd(hipStream_t s, const GutParams& P, const uint32_t* ranges, const uint32_t* sorted_pos, const uint32_t* pos_particle,
                           const float* density12, const float* features, const float* ray_o, const float* ray_d, float* out_fd, float* out_dist,
                           float* out_cnt) {
    const EntryLists lists = entry_lists(P, sorted_pos, pos_particle);
    if (P.k_buffer > 0) {   // the sorted hit buffer in front of the feature integration (round 6)
        const bool fast = nht_row48(P) && P.nht_act == 2 && P.nht_nf == 1;   // the default feature model
        if (fast) {
            GRUT_DISPATCH_K(P.k_buffer, hipLaunchKernelGGL((gut_render_nht_k_kernel<K_, false, true>), dim3(strip_grid(P)), dim3(64), 0, s, P,
                                                           reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12), features,
                                                           ray_o, ray_d, out_fd, out_dist, out_cnt, nullptr, nullptr, nullptr, nullptr));
        } else {
            GRUT_DISPATCH_K(P.k_buffer, hipLaunchKernelGGL((gut_render_nht_k_kernel<K_, false, false>), dim3(strip_grid(P)), dim3(64), 0, s, P,
                                                           reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12), features,
                                                           ray_o, ray_d, out_fd, out_dist, out_cnt, nullptr, nullptr, nullptr, nullptr));
        }
        return;
    }
    hipLaunchKernelGGL(gut_render_nht_fwd_kernel, dim3(strip_grid(P)), dim3(64), 0, s, P, reinterpret_cast<const uint2*>(ranges), lists,
                       reinterpret_cast<const float4*>(density12), features, ray_o, ray_d, out_fd, out_dist, out_cnt);
}
void launch_render_nht_bwd(hipStream_t s, const GutParams& P, const uint32_t* ranges, const uint32_t* sorted_pos, const uint32_t* pos_particle,
                           const float* density12, const float* features, const float* ray_o, const float* ray_d, const float* fd, const float* g_fd,
                           const float* dist, const float* g_dist, float* g_density12, float* g_features) {
    const EntryLists lists = entry_lists(P, sorted_pos, pos_particle);
    if (P.k_buffer > 0) {
        const bool fast = nht_row48(P) && P.nht_act == 2 && P.nht_nf == 1;
        if (fast) {
            GRUT_DISPATCH_K(P.k_buffer, hipLaunchKernelGGL((gut_render_nht_k_kernel<K_, true, true>), dim3(strip_grid(P)), dim3(64), 0, s, P,
                                                           reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12), features,
                                                           ray_o, ray_d, const_cast<float*>(fd), const_cast<float*>(dist), nullptr, g_fd, g_dist, g_density12,
                                                           g_features));
        } else {
            GRUT_DISPATCH_K(P.k_buffer, hipLaunchKernelGGL((gut_render_nht_k_kernel<K_, true, false>), dim3(strip_grid(P)), dim3(64), 0, s, P,
                                                           reinterpret_cast<const uint2*>(ranges), lists, reinterpret_cast<const float4*>(density12), features,
                                                           ray_o, ray_d, const_cast<float*>(fd), const_cast<float*>(dist), nullptr, g_fd, g_dist, g_density12,
                                                           g_features));
        }
        return;
    }
    hipLaunchKernelGGL(gut_render_nht_bwd_kernel, dim3(strip_grid(P)), dim3(64), 0, s, P, reinterpret_cast<const uint2*>(ranges), lists,
                       reinterpret_cast<const float4*>(density12), features, ray_o, ray_d, fd, g_fd, dist, g_dist, g_density12, g_features);
}

}  // namespace grut
