// loss.hip — the image losses of a training step: the fused, differentiable SSIM that the reference's loss imports as `fused_ssim`
// (threedgrut/model/losses.py:17, called at :31-33 with padding="valid"; trainer.py:715-720), and the fused photometric loss that adds
// the mask, L1 and L2 of trainer.py:687-720 to the same pass.  One kernel template per direction serves both.
//
//   map = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),   mu = G*x, s1 = G*(xx) - mu1^2, s12 = G*(xy) - mu1 mu2
//   G: separable 11-tap Gaussian (sigma 1.5), zero padding, per channel and per image of the batch.
//   photometric: a = m pred, b = m gt (m = 1 without a mask: no multiply is issued)
//   out = { mean|a - b|,  mean (pred - b)^2,  mean SSIM(a, b) }     (the L2 term's unmasked prediction is the reference's: trainer.py:709)
//
// Modes (compile time).  kLossSsim: the SSIM term alone, what grut_ssim_* launch; the runtime `terms` word is not read, there is one
// sum per workgroup at partials[workgroup] and one mean at out[0].  kLossPhoto / kLossPhotoMasked: what grut_photo_loss_* launch; up to
// three sums per workgroup leave in a fixed order (partials[k * workgroups + workgroup], k = 0 L1, 1 L2, 2 SSIM).  Because the SSIM-only
// mode is the same body with the additions compiled out, photometric_loss with only the SSIM term and no mask is fused_ssim bit for bit.
//
//   * forward: one workgroup per 32x32 output tile.  Tile + 5-pixel halo of both images -> LDS (bounds-checked loads: no padded copy),
//     horizontal pass of the five window sums (x, y, xx, yy, xy) -> LDS, vertical pass -> registers, then the map and, when training,
//     the three partial-derivative planes dmap/dmu1 (with the dependence of s1 and s12 on mu1 folded in), dmap/ds1, dmap/ds12.  The mask
//     ([B, H, W], broadcast over the channels) is staged into LDS first, so it is read once per pixel, and the images are multiplied by
//     it on their way into LDS; the planes are functions of a = m pred, the mask's factor is the backward's.  |a - b| and (pred - b)^2
//     are added up by the lane that stages the element, for the 32x32 centre of the staged tile only, so every pixel is counted by
//     exactly one workgroup and no image word is read twice for them.  Each sum of the tile is reduced in a fixed order (lane-sequential,
//     DPP wave sum, four waves in order) into ONE partial per workgroup; a second launch of one workgroup adds the partials in fp64 in a
//     fixed order and writes the means.  No floating-point atomics: bitwise reproducible.
//   * backward: dL/dimg1 = G*(dL dm_dmu1) + 2 img1 G*(dL dm_ds1) + img2 G*(dL dm_ds12), dL = grad_out / count inside the counted region
//     (the 5-pixel crop of "valid") and 0 outside; same tiling, three window sums instead of five.  The photometric modes add
//     g_l1 m sign(a - b) / P and 2 g_l2 (pred - b) / P at the centre pixel already held in LDS.  grad_out is read from device memory.
//     Terms that are not selected cost nothing but the staging; with the SSIM term off the backward skips the window sums altogether.
//
// Layout.  Both kernels take element strides for (B, C, H, W).  NC channels are handled by one workgroup: NC = 1 for planar (NCHW)
// memory, NC = C (2..4) for an NCHW view of channels-last memory (stride_c == 1, stride_w == C: what trainer.py:717-718 passes).  The
// staging loop walks a tile row as (pixel, channel) pairs, which for channels-last memory is ONE contiguous run of 42 NC (forward) or
// 32 NC (backward, and its gradient store) words, so consecutive lanes touch consecutive addresses in either layout; the channels are
// de-interleaved on the way into LDS so that both passes read unit-stride rows.  Any other stride pattern runs with NC = 1: correct,
// with strided loads.  The derivative planes are private: planar [B, C, H, W].
//
// Sizes.  Tile 32x32, 256 threads (4 waves).  A 32-wide tile makes a row of the horizontal result exactly one 32-lane LDS access group
// (ds_read_b32 / ds_write_b32 are served in two 32-lane halves, bank = word mod 32: unit-stride rows never conflict, and the staged rows'
// pitch of 42 words only matters across halves, which do not interact).  The halo costs (42/32)^2 = 1.72x loads, absorbed by L2; a 64x64
// tile (1.34x) would need 2.4x the LDS.  LDS per workgroup, forward: 2 NC 42x42 staged + 5 x 42x32 horizontal sums = 40.0 KiB (NC = 1),
// 67.6 KiB (NC = 3), 81.4 KiB (NC = 4); backward: 3 x 42x42 + 3 x 42x32 + 2 NC 32x32 = 44.4 KiB (NC = 1), 60.4 KiB (NC = 3).  Of the CU's
// 160 KiB that is 3 / 2 / 1 resident workgroups forward and 3 / 2 backward; the horizontal sums are kept per channel (not 5 NC planes)
// precisely so that RGB keeps two.  A mask adds 42x42 words forward (NC = 3: 74.5 KiB, still two workgroups per CU) and 32x32 backward
// (64.4 KiB).  The vertical pass gives each lane a 4-row strip of one column (14 LDS reads per 4 outputs and sum); the forward uses 84
// (NC = 1) to 112 (NC = 4, photometric) VGPRs, under the 128 that 4 waves per SIMD would allow, and LDS caps residency at 3 workgroups
// = 3 waves per SIMD anyway, hence amdgpu_waves_per_eu(1, 4): no register squeeze for an occupancy LDS forbids.
// Byte model (P = B C H W): forward training reads 8P and writes 12P, backward reads 20P and writes 4P, inference reads 8P;
// a mask adds P / C to each.
#include <algorithm>
#include <type_traits>

#include "common.hpp"

namespace grut {

constexpr int kSsimThreads = 256, kSsimTile = 32, kSsimHalo = 5, kSsimSpan = kSsimTile + 2 * kSsimHalo, kSsimTaps = 11, kSsimStrip = 4;
static_assert(kSsimThreads == kSsimTile * (kSsimTile / kSsimStrip), "one lane per column and 4-row strip");
// exp(-(i-5)^2 / (2 1.5^2)) normalised to sum 1 in double, rounded to fp32 (9 significant digits reproduce the fp32 value exactly)
static __device__ const float kSsimTap[kSsimTaps] = {0.00102838012f, 0.00759875821f, 0.0360007733f, 0.109360687f, 0.213005543f, 0.266011715f,
                                                      0.213005543f,   0.109360687f,   0.0360007733f, 0.00759875821f, 0.00102838012f};
constexpr float kSsimC1 = 0.01f * 0.01f, kSsimC2 = 0.03f * 0.03f;

constexpr int kLossSsim = 0, kLossPhoto = 1, kLossPhotoMasked = 2;   // MODE
constexpr int kPhotoL1 = 1, kPhotoL2 = 2, kPhotoSsim = 4, kPhotoTerms = 3;
// sums per workgroup, means and upstream gradients of a mode; the SSIM term's is always the last
constexpr int loss_sums(int mode) { return mode == kLossSsim ? 1 : kPhotoTerms; }
// whether a term is computed: known at compile time in the SSIM-only mode, which never reads the runtime word
template <int MODE>
__device__ __forceinline__ bool loss_has(int terms, int term) {
    if constexpr (MODE == kLossSsim)
        return term == kPhotoSsim;
    else
        return (terms & term) != 0;
}

// this lane's share of each sum of a tile; the SSIM-only mode has no L1 and L2
template <int MODE>
struct LossSums {
    float l1 = 0.0f, l2 = 0.0f, map = 0.0f;
};
template <>
struct LossSums<kLossSsim> {
    float map = 0.0f;
};

struct SsimView {   // an NCHW view: element strides
    const float* p;
    long long sb, sc, sh, sw;
    __device__ __forceinline__ float at(int b, int c, int y, int x) const { return p[b * sb + c * sc + y * sh + x * sw]; }
};
struct SsimShape {
    int C, H, W, valid;
};
struct PhotoMask {   // [B, H, W] through element strides
    const float* p;
    long long sb, sh, sw;
    __device__ __forceinline__ float at(int b, int y, int x) const { return p[b * sb + y * sh + x * sw]; }
};

// the 4-row strip of column x: out[j] = sum_k tap[k] * rows[ys + j + k][x]
template <typename Rows>
__device__ __forceinline__ void ssim_vertical(const Rows& rows, int ys, int x, float (&out)[kSsimStrip]) {
    float v[kSsimStrip + kSsimTaps - 1];
#pragma unroll
    for (int i = 0; i < kSsimStrip + kSsimTaps - 1; ++i) v[i] = rows[ys + i][x];
#pragma unroll
    for (int j = 0; j < kSsimStrip; ++j) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < kSsimTaps; ++k) s = fmaf(kSsimTap[k], v[j + k], s);
        out[j] = s;
    }
}

// Staging loop: element i of TOTAL is produced by load(i) (global memory, N words) and consumed by store(i, words) (LDS).  Written as
// "request kSsimBatch elements, then store them" because a plain load-store loop has ONE request per lane in flight: with at most 12
// waves per CU that made both kernels wait on HBM latency ~21 times in a row per tile (forward 127 us at 1080p RGB, 1.0 TB/s by the
// byte model, before).
constexpr int kSsimBatch = 8;
template <int N>
struct SsimWords {
    float v[N];
};
template <int TOTAL, int N, typename Load, typename Store>
__device__ __forceinline__ void ssim_stage(int t, Load load, Store store) {
    for (int base = t; base < TOTAL; base += kSsimBatch * kSsimThreads) {
        SsimWords<N> w[kSsimBatch];
#pragma unroll
        for (int k = 0; k < kSsimBatch; ++k) {
            const int i = base + k * kSsimThreads;
            if (i < TOTAL) w[k] = load(i);
        }
#pragma unroll
        for (int k = 0; k < kSsimBatch; ++k) {
            const int i = base + k * kSsimThreads;
            if (i < TOTAL) store(i, w[k]);
        }
    }
}

__device__ __forceinline__ bool ssim_counted(const SsimShape& s, int y, int x) {   // the pixels the mean runs over
    const int m = s.valid ? kSsimHalo : 0;
    return y >= m && y < s.H - m && x >= m && x < s.W - m;
}

template <int NC, bool TRAIN, int MODE>
__global__ __launch_bounds__(kSsimThreads) __attribute__((amdgpu_waves_per_eu(1, 4))) void loss_forward_kernel(
    SsimShape shp, SsimView img1, SsimView img2, PhotoMask mask, int terms, float* __restrict__ partials, float* __restrict__ dm_dmu1,
    float* __restrict__ dm_ds1, float* __restrict__ dm_ds12) {
    constexpr bool kPhoto = MODE != kLossSsim, kMasked = MODE == kLossPhotoMasked;
    constexpr int kSums = loss_sums(MODE), kMap = kSums - 1;
    __shared__ float s_raw[2][NC][kSsimSpan][kSsimSpan];
    __shared__ float s_h[5][kSsimSpan][kSsimTile];
    __shared__ float s_m[kMasked ? kSsimSpan : 1][kSsimSpan];   // only referenced, hence only allocated, with a mask
    __shared__ float s_red[kSums][kSsimThreads / GRUT_WAVE];
    const int t = threadIdx.x, H = shp.H, W = shp.W;
    const int x0 = blockIdx.x * kSsimTile, y0 = blockIdx.y * kSsimTile;
    const int groups = shp.C / NC, b = blockIdx.z / groups, c0 = (blockIdx.z % groups) * NC;

    if constexpr (kMasked) {
        ssim_stage<kSsimSpan * kSsimSpan, 1>(
            t,
            [&](int i) {
                const int r = i / kSsimSpan, px = i - r * kSsimSpan;
                const int y = y0 - kSsimHalo + r, x = x0 - kSsimHalo + px;
                const bool in = y >= 0 && y < H && x >= 0 && x < W;
                return SsimWords<1>{{in ? mask.at(b, y, x) : 0.0f}};
            },
            [&](int i, const SsimWords<1>& w) {
                const int r = i / kSsimSpan, px = i - r * kSsimSpan;
                s_m[r][px] = w.v[0];
            });
        __syncthreads();
    }

    LossSums<MODE> sum;
    constexpr int kRun = kSsimSpan * NC;   // one staged row as (pixel, channel) pairs: contiguous in channels-last memory
    ssim_stage<kSsimSpan * kRun, 2>(
        t,
        [&](int i) {
            const int r = i / kRun, j = i - r * kRun, px = j / NC, ch = j - px * NC;
            const int y = y0 - kSsimHalo + r, x = x0 - kSsimHalo + px;
            const bool in = y >= 0 && y < H && x >= 0 && x < W;
            return SsimWords<2>{{in ? img1.at(b, c0 + ch, y, x) : 0.0f, in ? img2.at(b, c0 + ch, y, x) : 0.0f}};
        },
        [&](int i, const SsimWords<2>& w) {
            const int r = i / kRun, j = i - r * kRun, px = j / NC, ch = j - px * NC;
            float av = w.v[0], bv = w.v[1];
            if constexpr (kMasked) {
                const float m = s_m[r][px];
                av *= m;
                bv *= m;
            }
            s_raw[0][ch][r][px] = av;
            s_raw[1][ch][r][px] = bv;
            if constexpr (kPhoto) {
                // the tile's own pixels (outside the image both words are 0): each belongs to exactly one workgroup
                if (r >= kSsimHalo && r < kSsimHalo + kSsimTile && px >= kSsimHalo && px < kSsimHalo + kSsimTile) {
                    if (loss_has<MODE>(terms, kPhotoL1)) sum.l1 += fabsf(av - bv);
                    if (loss_has<MODE>(terms, kPhotoL2)) {
                        const float d = w.v[0] - bv;
                        sum.l2 = fmaf(d, d, sum.l2);
                    }
                }
            }
        });

    const int x = t & (kSsimTile - 1), ys = (t / kSsimTile) * kSsimStrip;
    if (loss_has<MODE>(terms, kPhotoSsim)) {
        for (int ch = 0; ch < NC; ++ch) {
            __syncthreads();   // the staged tile is complete / the previous channel's vertical pass has read s_h
            for (int i = t; i < kSsimSpan * kSsimTile; i += kSsimThreads) {
                const int r = i / kSsimTile, c = i & (kSsimTile - 1);
                float m1 = 0.0f, m2 = 0.0f, xx = 0.0f, yy = 0.0f, xy = 0.0f;
#pragma unroll
                for (int k = 0; k < kSsimTaps; ++k) {
                    const float p = s_raw[0][ch][r][c + k], q = s_raw[1][ch][r][c + k];
                    const float wp = kSsimTap[k] * p, wq = kSsimTap[k] * q;
                    m1 += wp;
                    m2 += wq;
                    xx = fmaf(wp, p, xx);
                    yy = fmaf(wq, q, yy);
                    xy = fmaf(wp, q, xy);
                }
                s_h[0][r][c] = m1;
                s_h[1][r][c] = m2;
                s_h[2][r][c] = xx;
                s_h[3][r][c] = yy;
                s_h[4][r][c] = xy;
            }
            __syncthreads();
            float o[5][kSsimStrip];
#pragma unroll
            for (int q = 0; q < 5; ++q) ssim_vertical(s_h[q], ys, x, o[q]);
#pragma unroll
            for (int j = 0; j < kSsimStrip; ++j) {
                const int gy = y0 + ys + j, gx = x0 + x;
                if (gy >= H || gx >= W) continue;
                const float mu1 = o[0][j], mu2 = o[1][j];
                const float mu1s = mu1 * mu1, mu2s = mu2 * mu2, mu12 = mu1 * mu2;
                const float s1 = o[2][j] - mu1s, s2 = o[3][j] - mu2s, s12 = o[4][j] - mu12;
                const float a1 = 2.0f * mu12 + kSsimC1, a2 = 2.0f * s12 + kSsimC2;
                const float b1 = mu1s + mu2s + kSsimC1, b2 = s1 + s2 + kSsimC2;
                const float den = b1 * b2;
                const float map = (a1 * a2) / den;
                if (ssim_counted(shp, gy, gx)) sum.map += map;
                if constexpr (TRAIN) {
                    // map as a function of (mu1, E[xx], E[xy]): dmap/dE[xx] = dmap/ds1, dmap/dE[xy] = dmap/ds12, and the total derivative in
                    // mu1 carries ds1/dmu1 = -2 mu1 and ds12/dmu1 = -mu2
                    const float d_s1 = -map / b2;
                    const float d_s12 = (2.0f * a1) / den;
                    const float d_mu1 = (2.0f * a2) / den * (mu2 - mu1 * (a1 / b1)) - 2.0f * mu1 * d_s1 - mu2 * d_s12;
                    const size_t at = (((size_t)b * shp.C + (c0 + ch)) * H + gy) * W + gx;
                    dm_dmu1[at] = d_mu1;
                    dm_ds1[at] = d_s1;
                    dm_ds12[at] = d_s12;
                }
            }
        }
    }
    if constexpr (kPhoto) {
        sum.l1 = wave_sum(sum.l1);
        sum.l2 = wave_sum(sum.l2);
    }
    sum.map = wave_sum(sum.map);
    if ((t & (GRUT_WAVE - 1)) == 0) {
        if constexpr (kPhoto) {
            s_red[0][t / GRUT_WAVE] = sum.l1;
            s_red[1][t / GRUT_WAVE] = sum.l2;
        }
        s_red[kMap][t / GRUT_WAVE] = sum.map;
    }
    __syncthreads();
    if (t < kSums && (!kPhoto || ((terms >> t) & 1))) {   // lane k adds up sum k
        float s = s_red[t][0];
        for (int w = 1; w < kSsimThreads / GRUT_WAVE; ++w) s += s_red[t][w];
        const uint32_t workgroup = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        if constexpr (kPhoto)
            partials[t * (gridDim.x * gridDim.y * gridDim.z) + workgroup] = s;
        else
            partials[workgroup] = s;
    }
}

// One workgroup, the `sums` means one after the other: lane t adds partials t, t + 256, ... of a sum in fp64, then a fixed tree over the
// 256 lanes.  Sum k belongs to term bit kPhotoTerms - sums + k (the SSIM term's is the last); a term that was not selected is written as 0.
__global__ __launch_bounds__(kSsimThreads) void loss_mean_kernel(const float* __restrict__ partials, uint32_t n, int sums, int terms,
                                                                 double inv_pixels, double inv_ssim_count, float* __restrict__ out) {
    __shared__ double s_sum[kSsimThreads];
    for (int k = 0; k < sums; ++k) {
        if (!((terms >> (kPhotoTerms - sums + k)) & 1)) {
            if (threadIdx.x == 0) out[k] = 0.0f;
            continue;
        }
        double s = 0.0;
        for (uint32_t i = threadIdx.x; i < n; i += kSsimThreads) s += (double)partials[k * n + i];
        __syncthreads();   // the previous term's tree has been read
        s_sum[threadIdx.x] = s;
        __syncthreads();
        for (int half = kSsimThreads / 2; half > 0; half >>= 1) {
            if ((int)threadIdx.x < half) s_sum[threadIdx.x] += s_sum[threadIdx.x + half];
            __syncthreads();
        }
        if (threadIdx.x == 0) out[k] = (float)(s_sum[0] * (k == sums - 1 ? inv_ssim_count : inv_pixels));
    }
}

template <int NC, int MODE>
__global__ __launch_bounds__(kSsimThreads) __attribute__((amdgpu_waves_per_eu(1, 4))) void loss_backward_kernel(
    SsimShape shp, SsimView img1, SsimView img2, PhotoMask mask, int terms, const float* __restrict__ grad_out, float inv_count,
    double inv_pixels, const float* __restrict__ dm_dmu1, const float* __restrict__ dm_ds1, const float* __restrict__ dm_ds12,
    float* __restrict__ grad, long long gsb, long long gsc, long long gsh, long long gsw) {
    constexpr bool kPhoto = MODE != kLossSsim, kMasked = MODE == kLossPhotoMasked;
    __shared__ float s_x[kSsimTile][kSsimTile * NC], s_y[kSsimTile][kSsimTile * NC];   // img1 (unmasked) and b = m img2, (pixel, channel) pairs as in memory
    __shared__ float s_m[kMasked ? kSsimTile : 1][kSsimTile];                            // only referenced, hence only allocated, with a mask
    __shared__ float s_p[3][kSsimSpan][kSsimSpan];
    __shared__ float s_h[3][kSsimSpan][kSsimTile];
    const int t = threadIdx.x, H = shp.H, W = shp.W;
    const int x0 = blockIdx.x * kSsimTile, y0 = blockIdx.y * kSsimTile;
    const int groups = shp.C / NC, b = blockIdx.z / groups, c0 = (blockIdx.z % groups) * NC;
    const bool with_ssim = loss_has<MODE>(terms, kPhotoSsim);
    const float scale = with_ssim ? grad_out[loss_sums(MODE) - 1] * inv_count : 0.0f;
    double c_l1 = 0.0;   // rounded to fp32 once, after the mask
    float c_l2 = 0.0f;
    if constexpr (kPhoto) {
        c_l1 = loss_has<MODE>(terms, kPhotoL1) ? (double)grad_out[0] * inv_pixels : 0.0;
        c_l2 = loss_has<MODE>(terms, kPhotoL2) ? (float)(2.0 * (double)grad_out[1] * inv_pixels) : 0.0f;
    }

    if constexpr (kMasked) {
        ssim_stage<kSsimTile * kSsimTile, 1>(
            t,
            [&](int i) {
                const int r = i / kSsimTile, px = i - r * kSsimTile;
                const int y = y0 + r, x = x0 + px;
                return SsimWords<1>{{(y < H && x < W) ? mask.at(b, y, x) : 0.0f}};
            },
            [&](int i, const SsimWords<1>& w) { s_m[i / kSsimTile][i & (kSsimTile - 1)] = w.v[0]; });
        __syncthreads();
    }
    constexpr int kRun = kSsimTile * NC;
    ssim_stage<kSsimTile * kRun, 2>(
        t,
        [&](int i) {
            const int r = i / kRun, j = i - r * kRun, px = j / NC, ch = j - px * NC;
            const int y = y0 + r, x = x0 + px;
            const bool in = y < H && x < W;
            return SsimWords<2>{{in ? img1.at(b, c0 + ch, y, x) : 0.0f, in ? img2.at(b, c0 + ch, y, x) : 0.0f}};
        },
        [&](int i, const SsimWords<2>& w) {
            const int r = i / kRun, j = i - r * kRun;
            s_x[r][j] = w.v[0];
            if constexpr (kMasked)
                s_y[r][j] = s_m[r][j / NC] * w.v[1];
            else
                s_y[r][j] = w.v[1];
        });

    const int x = t & (kSsimTile - 1), ys = (t / kSsimTile) * kSsimStrip;
    for (int ch = 0; ch < NC; ++ch) {
        float o[3][kSsimStrip] = {};
        if (with_ssim) {
            __syncthreads();   // s_x and s_y are complete / the previous channel's passes are done with s_p and s_h
            const size_t plane = ((size_t)b * shp.C + (c0 + ch)) * H;
            ssim_stage<kSsimSpan * kSsimSpan, 3>(
                t,
                [&](int i) {
                    const int r = i / kSsimSpan, px = i - r * kSsimSpan;
                    const int y = y0 - kSsimHalo + r, xg = x0 - kSsimHalo + px;
                    const bool in = y >= 0 && xg >= 0 && ssim_counted(shp, y, xg);   // dL/dmap is 0 outside the counted region
                    const size_t at = in ? (plane + y) * W + xg : 0;
                    return SsimWords<3>{{in ? dm_dmu1[at] : 0.0f, in ? dm_ds1[at] : 0.0f, in ? dm_ds12[at] : 0.0f}};
                },
                [&](int i, const SsimWords<3>& w) {
                    const int r = i / kSsimSpan, px = i - r * kSsimSpan;
                    s_p[0][r][px] = w.v[0];
                    s_p[1][r][px] = w.v[1];
                    s_p[2][r][px] = w.v[2];
                });
            __syncthreads();
            for (int i = t; i < kSsimSpan * kSsimTile; i += kSsimThreads) {
                const int r = i / kSsimTile, c = i & (kSsimTile - 1);
                float h0 = 0.0f, h1 = 0.0f, h2 = 0.0f;
#pragma unroll
                for (int k = 0; k < kSsimTaps; ++k) {
                    h0 = fmaf(kSsimTap[k], s_p[0][r][c + k], h0);
                    h1 = fmaf(kSsimTap[k], s_p[1][r][c + k], h1);
                    h2 = fmaf(kSsimTap[k], s_p[2][r][c + k], h2);
                }
                s_h[0][r][c] = h0;
                s_h[1][r][c] = h1;
                s_h[2][r][c] = h2;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 3; ++q) ssim_vertical(s_h[q], ys, x, o[q]);
        } else if (ch == 0) {
            __syncthreads();   // s_x and s_y are complete
        }
#pragma unroll
        for (int j = 0; j < kSsimStrip; ++j) {   // each (row, pixel, channel) slot of s_x is read and overwritten by this lane alone
            const float pv = s_x[ys + j][x * NC + ch], yv = s_y[ys + j][x * NC + ch];
            float m = 1.0f, xv = pv;
            if constexpr (kMasked) {
                m = s_m[ys + j][x];
                xv = m * pv;
            }
            float g = 0.0f;
            if (with_ssim) {
                g = scale * (o[0][j] + 2.0f * xv * o[1][j] + yv * o[2][j]);
                if constexpr (kMasked) g *= m;
            }
            if constexpr (kPhoto) {
                if (loss_has<MODE>(terms, kPhotoL1)) {   // sign(0) = 0, as torch.abs's gradient
                    const float d = xv - yv;
                    const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
                    if constexpr (kMasked)
                        g += (float)((double)(m * sgn) * c_l1);
                    else
                        g += sgn * (float)c_l1;
                }
                if (loss_has<MODE>(terms, kPhotoL2)) g = fmaf(c_l2, pv - yv, g);
            }
            s_x[ys + j][x * NC + ch] = g;
        }
    }
    __syncthreads();
    for (int i = t; i < kSsimTile * kRun; i += kSsimThreads) {
        const int r = i / kRun, j = i - r * kRun, px = j / NC, ch = j - px * NC;
        const int y = y0 + r, xg = x0 + px;
        if (y < H && xg < W) grad[b * gsb + (c0 + ch) * gsc + y * gsh + xg * gsw] = s_x[r][j];
    }
}

static int ssim_check_shape(const char* who, int B, int C, int H, int W, int valid) {
    GRUT_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: B, C, H, W must be >= 1 (got %d, %d, %d, %d)", who, B, C, H, W);
    GRUT_REQUIRE(valid == 0 || valid == 1, "%s: valid must be 0 (\"same\") or 1 (got %d)", who, valid);
    GRUT_REQUIRE(!valid || (H >= kSsimTaps && W >= kSsimTaps), "%s: \"valid\" needs H, W >= 11 (got %d x %d)", who, H, W);
    GRUT_REQUIRE((int64_t)B * C <= 65535, "%s: B * C must be <= 65535 (got %lld)", who, (long long)B * C);
    return GRUT_OK;
}
static int photo_check(const char* who, int B, int C, int H, int W, int terms, int valid) {
    GRUT_REQUIRE(terms >= 1 && terms <= (kPhotoL1 | kPhotoL2 | kPhotoSsim), "%s: terms must be a non-empty combination of 1 (L1), 2 (L2), 4 (SSIM) (got %d)",
                 who, terms);
    GRUT_REQUIRE(valid == 0 || valid == 1, "%s: valid must be 0 (\"same\") or 1 (got %d)", who, valid);
    return ssim_check_shape(who, B, C, H, W, (terms & kPhotoSsim) ? valid : 0);   // the window's size limit only binds the SSIM term
}

// NC > 1 only for an NCHW view of channels-last memory with 2..4 channels (see the head of the file)
static int ssim_channels_per_group(int C, int W, const int64_t* s) {
    return (C >= 2 && C <= 4 && s[1] == 1 && s[3] == C && s[2] >= (int64_t)W * C) ? C : 1;
}

// What the four launching entry points make of their (checked) C arguments.  The grut_ssim_* pair passes no mask and terms = kPhotoSsim.
struct LossCall {
    hipStream_t stream;
    int nc, mode, terms;
    dim3 grid;
    SsimShape shp;
    SsimView v1, v2;
    PhotoMask mask;
    double inv_pixels, inv_ssim_count;   // 1 / (B C H W) and 1 / (the pixels the SSIM mean runs over), 0 with the SSIM term off
};
// grad_stride: the third strided tensor of a backward, null in a forward
static LossCall loss_call(void* stream, bool photo, int B, int C, int H, int W, const float* img1, const int64_t* stride1, const float* img2,
                          const int64_t* stride2, const float* mask, const int64_t* mask_stride, int terms, int valid,
                          const int64_t* grad_stride) {
    LossCall c;
    c.stream = reinterpret_cast<hipStream_t>(stream);
    c.nc = std::min(ssim_channels_per_group(C, W, stride1), ssim_channels_per_group(C, W, stride2));
    if (grad_stride) c.nc = std::min(c.nc, ssim_channels_per_group(C, W, grad_stride));
    c.mode = !photo ? kLossSsim : (mask ? kLossPhotoMasked : kLossPhoto);
    c.terms = terms;
    c.grid = dim3(div_up((uint32_t)W, kSsimTile), div_up((uint32_t)H, kSsimTile), (uint32_t)(B * (C / c.nc)));
    c.shp = SsimShape{C, H, W, valid};
    c.v1 = SsimView{img1, stride1[0], stride1[1], stride1[2], stride1[3]};
    c.v2 = SsimView{img2, stride2[0], stride2[1], stride2[2], stride2[3]};
    c.mask = mask ? PhotoMask{mask, mask_stride[0], mask_stride[1], mask_stride[2]} : PhotoMask{nullptr, 0, 0, 0};
    c.inv_pixels = 1.0 / ((double)B * C * (double)H * (double)W);
    const int m = valid ? 2 * kSsimHalo : 0;
    c.inv_ssim_count = (terms & kPhotoSsim) ? 1.0 / ((double)B * C * (double)(H - m) * (double)(W - m)) : 0.0;
    return c;
}

// launch(NC, MODE), both as std::integral_constant: the one place where the runtime choice meets the instantiations
template <int V>
using LossConst = std::integral_constant<int, V>;
template <typename Launch>
static void loss_dispatch(const LossCall& c, Launch launch) {
    auto with_nc = [&](auto nc) {
        switch (c.mode) {
            case kLossPhoto: launch(nc, LossConst<kLossPhoto>{}); break;
            case kLossPhotoMasked: launch(nc, LossConst<kLossPhotoMasked>{}); break;
            default: launch(nc, LossConst<kLossSsim>{}); break;
        }
    };
    switch (c.nc) {
        case 2: with_nc(LossConst<2>{}); break;
        case 3: with_nc(LossConst<3>{}); break;
        case 4: with_nc(LossConst<4>{}); break;
        default: with_nc(LossConst<1>{}); break;
    }
}

// the derivative planes are all given (training) or all null (inference): the entry points have checked
static int loss_forward(const LossCall& c, float* out, float* partials, float* dm_dmu1, float* dm_ds1, float* dm_ds12) {
    loss_dispatch(c, [&](auto nc, auto mode) {
        constexpr int NC = decltype(nc)::value, MODE = decltype(mode)::value;
        if (dm_dmu1)
            hipLaunchKernelGGL((loss_forward_kernel<NC, true, MODE>), c.grid, dim3(kSsimThreads), 0, c.stream, c.shp, c.v1, c.v2, c.mask, c.terms,
                               partials, dm_dmu1, dm_ds1, dm_ds12);
        else
            hipLaunchKernelGGL((loss_forward_kernel<NC, false, MODE>), c.grid, dim3(kSsimThreads), 0, c.stream, c.shp, c.v1, c.v2, c.mask, c.terms,
                               partials, (float*)nullptr, (float*)nullptr, (float*)nullptr);
    });
    GRUT_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_mean_kernel, dim3(1), dim3(kSsimThreads), 0, c.stream, partials, c.grid.x * c.grid.y * c.grid.z, loss_sums(c.mode),
                       c.terms, c.inv_pixels, c.inv_ssim_count, out);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

static int loss_backward(const LossCall& c, const float* grad_out, const float* dm_dmu1, const float* dm_ds1, const float* dm_ds12, float* grad,
                         const int64_t* grad_stride) {
    loss_dispatch(c, [&](auto nc, auto mode) {
        hipLaunchKernelGGL((loss_backward_kernel<decltype(nc)::value, decltype(mode)::value>), c.grid, dim3(kSsimThreads), 0, c.stream, c.shp, c.v1,
                           c.v2, c.mask, c.terms, grad_out, (float)c.inv_ssim_count, c.inv_pixels, dm_dmu1, dm_ds1, dm_ds12, grad,
                           (long long)grad_stride[0], (long long)grad_stride[1], (long long)grad_stride[2], (long long)grad_stride[3]);
    });
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

}  // namespace grut

extern "C" uint32_t grut_ssim_partials(int B, int C, int H, int W) {
    using namespace grut;
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    return (uint32_t)B * (uint32_t)C * div_up((uint32_t)W, kSsimTile) * div_up((uint32_t)H, kSsimTile);
}

extern "C" uint32_t grut_photo_loss_partials(int B, int C, int H, int W) { return grut::kPhotoTerms * grut_ssim_partials(B, C, H, W); }

extern "C" int grut_ssim_forward(void* stream, int B, int C, int H, int W, const float* img1, const int64_t* stride1, const float* img2,
                                 const int64_t* stride2, int valid, float* out_mean, float* partials, float* dm_dmu1, float* dm_ds1,
                                 float* dm_ds12) {
    using namespace grut;
    GRUT_CHECK(ssim_check_shape("grut_ssim_forward", B, C, H, W, valid));
    GRUT_REQUIRE(img1 && img2 && stride1 && stride2 && out_mean && partials, "grut_ssim_forward: null tensor");
    const bool train = dm_dmu1 || dm_ds1 || dm_ds12;
    GRUT_REQUIRE(!train || (dm_dmu1 && dm_ds1 && dm_ds12), "grut_ssim_forward: the three derivative planes are given together or not at all");
    return loss_forward(loss_call(stream, false, B, C, H, W, img1, stride1, img2, stride2, nullptr, nullptr, kPhotoSsim, valid, nullptr), out_mean,
                        partials, dm_dmu1, dm_ds1, dm_ds12);
}

extern "C" int grut_ssim_backward(void* stream, int B, int C, int H, int W, const float* img1, const int64_t* stride1, const float* img2,
                                  const int64_t* stride2, int valid, const float* grad_out, const float* dm_dmu1, const float* dm_ds1,
                                  const float* dm_ds12, float* grad_img1, const int64_t* grad_stride) {
    using namespace grut;
    GRUT_CHECK(ssim_check_shape("grut_ssim_backward", B, C, H, W, valid));
    GRUT_REQUIRE(img1 && img2 && stride1 && stride2 && grad_out && dm_dmu1 && dm_ds1 && dm_ds12 && grad_img1 && grad_stride,
                 "grut_ssim_backward: null tensor");
    return loss_backward(loss_call(stream, false, B, C, H, W, img1, stride1, img2, stride2, nullptr, nullptr, kPhotoSsim, valid, grad_stride),
                         grad_out, dm_dmu1, dm_ds1, dm_ds12, grad_img1, grad_stride);
}

extern "C" int grut_photo_loss_forward(void* stream, int B, int C, int H, int W, const float* pred, const int64_t* pred_stride, const float* gt,
                                       const int64_t* gt_stride, const float* mask, const int64_t* mask_stride, int terms, int valid,
                                       float* out, float* partials, float* dm_dmu1, float* dm_ds1, float* dm_ds12) {
    using namespace grut;
    GRUT_CHECK(photo_check("grut_photo_loss_forward", B, C, H, W, terms, valid));
    GRUT_REQUIRE(pred && gt && pred_stride && gt_stride && out && partials, "grut_photo_loss_forward: null tensor");
    GRUT_REQUIRE(!mask || mask_stride, "grut_photo_loss_forward: a mask needs its strides");
    const bool train = dm_dmu1 || dm_ds1 || dm_ds12;
    GRUT_REQUIRE(!train || (dm_dmu1 && dm_ds1 && dm_ds12), "grut_photo_loss_forward: the three derivative planes are given together or not at all");
    GRUT_REQUIRE(!train || (terms & kPhotoSsim), "grut_photo_loss_forward: derivative planes are only written with the SSIM term (4) selected");
    return loss_forward(loss_call(stream, true, B, C, H, W, pred, pred_stride, gt, gt_stride, mask, mask_stride, terms, valid, nullptr), out, partials,
                        dm_dmu1, dm_ds1, dm_ds12);
}

extern "C" int grut_photo_loss_backward(void* stream, int B, int C, int H, int W, const float* pred, const int64_t* pred_stride, const float* gt,
                                        const int64_t* gt_stride, const float* mask, const int64_t* mask_stride, int terms, int valid,
                                        const float* grad_out, const float* dm_dmu1, const float* dm_ds1, const float* dm_ds12, float* grad_pred,
                                        const int64_t* grad_stride) {
    using namespace grut;
    GRUT_CHECK(photo_check("grut_photo_loss_backward", B, C, H, W, terms, valid));
    GRUT_REQUIRE(pred && gt && pred_stride && gt_stride && grad_out && grad_pred && grad_stride, "grut_photo_loss_backward: null tensor");
    GRUT_REQUIRE(!mask || mask_stride, "grut_photo_loss_backward: a mask needs its strides");
    GRUT_REQUIRE(!(terms & kPhotoSsim) || (dm_dmu1 && dm_ds1 && dm_ds12), "grut_photo_loss_backward: the SSIM term (4) needs the three derivative planes");
    return loss_backward(loss_call(stream, true, B, C, H, W, pred, pred_stride, gt, gt_stride, mask, mask_stride, terms, valid, grad_stride), grad_out,
                         dm_dmu1, dm_ds1, dm_ds12, grad_pred, grad_stride);
}
