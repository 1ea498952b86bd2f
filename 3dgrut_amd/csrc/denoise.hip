// denoise.hip — non-local means (Buades, Coll, Morel 2005) on an RGB frame: what stands behind Tracer.denoise, the call the reference's
// playground engine makes at the end of every render pass (threedgrut_playground/tracer.py:269-271 -> hybridTracer.h:143, the OptiX
// learned LDR denoiser on RGB alone).  The model is this project's choice and is stated in include/grut_amd.h (grut_denoise) and
// DESIGN.md §7n; in short, for a pixel p and every other pixel q of the same image within the search radius r:
//   d2(p,q) = sum over o in [-f,f]^2 and the three channels of (I[clamp(p+o)] - I[clamp(q+o)])^2
//   w(p,q)  = exp(-min(d2 / (3 (2f+1)^2 h^2), 80)),   w(p,p) = max_q w(p,q)   (1 when there is no q)
//   out[p]  = (sum_q w(p,q) I[q] + w(p,p) I[p]) / (sum_q w(p,q) + w(p,p))
//
// One launch.  A workgroup of 512 lanes owns a 32 x 16 tile of output pixels, one lane per pixel, and stages the tile with its halo of
// r + f pixels, coordinates clamped to the image, once in LDS as float4.  Every candidate offset d is then evaluated from LDS in two steps
// that share the per-offset squared-difference image D_d(x) = |I(x) - I(x + d)|^2 between the patches of neighbouring pixels:
//   A  column sums V(x, y) = sum_{oy} D_d(x, y + oy) for the tile's 16 rows and its 32 + 2f columns: (32 + 2f) 16 <= 640 items over 512
//      lanes (the first 32 f lanes take a second one), each 2f + 1 pairs of ds_read_b128, written to a double-buffered [16][32 + 2f] plane
//   B  after one barrier, lane (tx, ty) adds V(tx .. tx + 2f, ty), takes the weight and accumulates I(p + d) with it
// so a pixel costs (32 + 2f) / 32 (2f + 1) patch elements per candidate instead of (2f + 1)^2, and the loop has one barrier per offset:
// step A of offset k + 1 writes the plane that step B of offset k - 1 read, and every lane passed the barrier of offset k in between.
// Every term of every sum is non-negative and the order is fixed by (H, W, f, r): channels, then oy ascending, then ox ascending, then
// the candidates row by row.  No atomics.  No address depends on a pixel's value: a NaN poisons the sums it enters and nothing else.
#include "common.hpp"

#include <cfloat>
#include <cmath>

namespace grut {

constexpr int kDenoiseTileW = 32, kDenoiseTileH = 16;   // TILE_W, TILE_H of 3dgrut_amd/denoise.py
constexpr int kDenoiseThreads = kDenoiseTileW * kDenoiseTileH;
constexpr int kDenoiseMaxPatch = 4, kDenoiseMaxSearch = 16;
constexpr float kDenoiseXMax = 80.f;

// bytes of LDS of one workgroup: the clamped halo image as float4 and the two column-sum planes
static uint32_t denoise_lds_bytes(int f, int r) {
    const uint32_t iw = kDenoiseTileW + 2 * (r + f), ih = kDenoiseTileH + 2 * (r + f);
    return iw * ih * 16u + 2u * kDenoiseTileH * (kDenoiseTileW + 2 * f) * 4u;
}

__device__ __forceinline__ float denoise_dist(const float4 a, const float4 b, float acc) {
    const float dr = a.x - b.x, dg = a.y - b.y, db = a.z - b.z;
    return fmaf(db, db, fmaf(dg, dg, fmaf(dr, dr, acc)));
}

template <int F>
__global__ __launch_bounds__(kDenoiseThreads) void denoise_kernel(int r, float inv_nh2, uint32_t height, uint32_t width, uint32_t tiles_x,
                                                                  uint32_t tiles_y, const float* __restrict__ rgb_in,
                                                                  float* __restrict__ rgb_out) {
    constexpr int CW = kDenoiseTileW + 2 * F;                  // columns of a column-sum plane
    constexpr int kItems = CW * kDenoiseTileH;                 // column sums per offset, <= 640
    const int R = r + F;                                       // halo
    const int IW = kDenoiseTileW + 2 * R, IH = kDenoiseTileH + 2 * R;
    extern __shared__ __attribute__((aligned(16))) unsigned char denoise_lds[];
    float4* const img = reinterpret_cast<float4*>(denoise_lds);                  // [IH][IW], pixel (x0 - R + lx, y0 - R + ly) clamped
    float* const planes = reinterpret_cast<float*>(img + IW * IH);               // [2][kDenoiseTileH][CW]

    const uint32_t tile = blockIdx.x, per_image = tiles_x * tiles_y;
    const uint32_t b = tile / per_image, in_image = tile % per_image;
    const int x0 = (int)(in_image % tiles_x) * kDenoiseTileW, y0 = (int)(in_image / tiles_x) * kDenoiseTileH;
    const int t = (int)threadIdx.x, tx = t % kDenoiseTileW, ty = t / kDenoiseTileW;
    const int H = (int)height, W = (int)width;
    const size_t image_base = (size_t)b * height * width;      // pixels; (b H + y) W + x < 2^31 is the entry point's precondition

    for (int i = t; i < IW * IH; i += kDenoiseThreads) {
        const int lx = i % IW, ly = i / IW;
        const int gx = min(max(x0 - R + lx, 0), W - 1), gy = min(max(y0 - R + ly, 0), H - 1);
        const float* src = rgb_in + 3 * (image_base + (size_t)gy * width + (size_t)gx);
        img[i] = make_float4(src[0], src[1], src[2], 0.f);
    }
    __syncthreads();

    // step A's items: column cx of row ry of the plane is the image's column (x0 + cx - F), LDS column cx + r; its rows are LDS rows
    // ry + r .. ry + r + 2F.  With the offset added the column is cx + r + dx in [0, IW) and the row ry + r + oy + dy in [0, IH).
    const int item1 = t + kDenoiseThreads;
    const bool second = item1 < kItems;
    const int a0 = (t / CW + r) * IW + (t % CW) + r;
    const int a1 = second ? (item1 / CW + r) * IW + (item1 % CW) + r : a0;
    const int centre = (ty + R) * IW + tx + R;
    const int px = x0 + tx, py = y0 + ty;

    float sum_w = 0.f, w_max = 0.f, acc_r = 0.f, acc_g = 0.f, acc_b = 0.f;
    int parity = 0;
    for (int dy = -r; dy <= r; ++dy) {
        for (int dx = -r; dx <= r; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int shift = dy * IW + dx;
            float* const plane = planes + parity * kItems;
            {
                float v = 0.f;
#pragma unroll
                for (int oy = 0; oy <= 2 * F; ++oy) v = denoise_dist(img[a0 + oy * IW], img[a0 + oy * IW + shift], v);
                plane[t] = v;
            }
            if (second) {
                float v = 0.f;
#pragma unroll
                for (int oy = 0; oy <= 2 * F; ++oy) v = denoise_dist(img[a1 + oy * IW], img[a1 + oy * IW + shift], v);
                plane[item1] = v;
            }
            __syncthreads();
            float d2 = 0.f;
#pragma unroll
            for (int ox = 0; ox <= 2 * F; ++ox) d2 += plane[ty * CW + tx + ox];
            const int qx = px + dx, qy = py + dy;
            if (qx >= 0 && qx < W && qy >= 0 && qy < H) {      // coordinates only: q is a pixel of this image
                const float w = expf(-fminf(d2 * inv_nh2, kDenoiseXMax));
                const float4 q = img[centre + shift];
                sum_w += w;
                w_max = fmaxf(w_max, w);
                acc_r = fmaf(w, q.x, acc_r);
                acc_g = fmaf(w, q.y, acc_g);
                acc_b = fmaf(w, q.z, acc_b);
            }
            parity ^= 1;
        }
    }
    if (px < W && py < H) {
        if (H == 1 && W == 1) w_max = 1.f;                     // no other pixel: the image comes back as it is
        const float4 p = img[centre];
        const float inv = 1.f / (sum_w + w_max);
        float* dst = rgb_out + 3 * (image_base + (size_t)py * width + (size_t)px);
        dst[0] = fmaf(w_max, p.x, acc_r) * inv;
        dst[1] = fmaf(w_max, p.y, acc_g) * inv;
        dst[2] = fmaf(w_max, p.z, acc_b) * inv;
    }
}

template <int F>
static int denoise_launch(hipStream_t stream, int r, float inv_nh2, uint32_t batch, uint32_t height, uint32_t width, const float* rgb_in,
                          float* rgb_out) {
    const uint32_t tiles_x = (width + kDenoiseTileW - 1) / kDenoiseTileW, tiles_y = (height + kDenoiseTileH - 1) / kDenoiseTileH;
    const uint32_t bytes = denoise_lds_bytes(F, r);
    if (bytes > 64u * 1024u)
        GRUT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&denoise_kernel<F>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    // tiles <= pixels < 2^31: a one-dimensional grid holds them
    denoise_kernel<F><<<dim3(batch * tiles_x * tiles_y), dim3(kDenoiseThreads), bytes, stream>>>(r, inv_nh2, height, width, tiles_x, tiles_y, rgb_in,
                                                                                              rgb_out);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

}  // namespace grut

extern "C" int grut_denoise(void* stream, const GrutDenoiseConfig* cfg, uint32_t batch, uint32_t height, uint32_t width, const float* rgb_in,
                            float* rgb_out) {
    using namespace grut;
    GRUT_REQUIRE(cfg, "grut_denoise: cfg is NULL");
    GRUT_REQUIRE(rgb_in, "grut_denoise: rgb_in is NULL");
    GRUT_REQUIRE(rgb_out, "grut_denoise: rgb_out is NULL");
    const int f = cfg->patch_radius, r = cfg->search_radius;
    GRUT_REQUIRE(f >= 0 && f <= kDenoiseMaxPatch, "grut_denoise: patch_radius = %d, must be 0..%d", f, kDenoiseMaxPatch);
    GRUT_REQUIRE(r >= 1 && r <= kDenoiseMaxSearch, "grut_denoise: search_radius = %d, must be 1..%d", r, kDenoiseMaxSearch);
    GRUT_REQUIRE(std::isfinite(cfg->h) && cfg->h > 0.f, "grut_denoise: h = %g, must be finite and above 0", (double)cfg->h);
    GRUT_REQUIRE(height != 0u, "grut_denoise: height is 0");
    GRUT_REQUIRE(width != 0u, "grut_denoise: width is 0");
    const uint64_t pixels = (uint64_t)batch * height * width;   // three factors below 2^32: reduce before the third
    GRUT_REQUIRE((uint64_t)batch * height < (1ull << 31) && pixels < (1ull << 31),
                 "grut_denoise: batch * height * width = %u * %u * %u, must be below 2^31", batch, height, width);
    const uintptr_t in0 = (uintptr_t)rgb_in, out0 = (uintptr_t)rgb_out, span = (uintptr_t)pixels * 3u * sizeof(float);
    GRUT_REQUIRE(in0 + span <= out0 || out0 + span <= in0, "grut_denoise: rgb_in and rgb_out overlap (the filter is out of place)");
    if (batch == 0u) return GRUT_OK;
    const int n = 3 * (2 * f + 1) * (2 * f + 1);
    // 1 / (n h^2) rounded to fp32 once, and held finite: with an h so small that it would be inf, equal patches (d2 = 0) still get
    // x = 0 and every other pair the clamp
    const float inv_nh2 = (float)std::fmin(1.0 / ((double)n * (double)cfg->h * (double)cfg->h), (double)FLT_MAX);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (f) {
        case 0: return denoise_launch<0>(s, r, inv_nh2, batch, height, width, rgb_in, rgb_out);
        case 1: return denoise_launch<1>(s, r, inv_nh2, batch, height, width, rgb_in, rgb_out);
        case 2: return denoise_launch<2>(s, r, inv_nh2, batch, height, width, rgb_in, rgb_out);
        case 3: return denoise_launch<3>(s, r, inv_nh2, batch, height, width, rgb_in, rgb_out);
        default: return denoise_launch<4>(s, r, inv_nh2, batch, height, width, rgb_in, rgb_out);
    }
}
