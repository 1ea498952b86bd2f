// ppisp.hip — PPISP post-processing (the learned camera model the reference's trainer applies between render() and get_losses,
// threedgrut/utils/render.py:110-151) as one HIP pass each way.  The model and its gradient conventions: ppisp_math.hpp.
//
// Layout.  A lane takes kPix = 4 consecutive pixels per trip (three 16-byte loads of rgb, two of pixel_coords), a block of 256 lanes 1024,
// and the grid (at most kMaxBlocks blocks) strides over the image.  The activated parameters are computed ONCE per block by its first lane
// into LDS and then live in scalar registers (readfirstlane), not in 53 VGPRs of every lane.  The backward pass recomputes the forward
// from rgb (nothing is saved: the pass is memory-bound), keeps the 40 parameter gradients of its pixels in registers against the activated
// quantities, and reduces them wave (DPP reduce-scatter, common.hpp) -> block (LDS, fixed order) -> one 48-float row of `partials`.
// A one-block kernel sums the rows in a fixed order and applies the chain rules of softplus / sigmoid / the homography construction.
// No atomics anywhere: two runs on the same input are bitwise equal.
#include "common.hpp"
#include "ppisp_math.hpp"

namespace grut {
namespace {

using namespace ppisp;

constexpr int kBlock = 256, kPix = 4, kBlockPixels = kBlock * kPix, kWaves = kBlock / GRUT_WAVE;
constexpr uint32_t kMaxBlocks = 1024;   // 4 blocks of 4 waves per CU: enough loads in flight, and few enough rows for the finish kernel
constexpr int kFinishThreads = 1008, kFinishGroups = kFinishThreads / kRow;   // 21 row groups x 48 columns

uint32_t num_blocks(uint32_t P) {
    const uint32_t need = (uint32_t)(((uint64_t)P + kBlockPixels - 1) / kBlockPixels);
    return need < kMaxBlocks ? need : kMaxBlocks;
}

struct Params {
    const float *exposure, *color, *vignetting, *crf;
    float res_w, res_h;
};

__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// the block's prologue: lane 0 activates the parameters, everyone picks them up as wave-uniform values
__device__ __forceinline__ Prep block_prep(const Params& a) {
    __shared__ Prep sp;
    if (threadIdx.x == 0) prepare(sp, a.res_w, a.res_h, a.exposure, a.color, a.vignetting, a.crf);
    __syncthreads();
    Prep p;
    p.scale = uni(sp.scale);
    p.half_w = uni(sp.half_w);
    p.half_h = uni(sp.half_h);
    p.inv_extent = uni(sp.inv_extent);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int k = 0; k < 5; ++k) p.vig[c][k] = uni(sp.vig[c][k]);
        p.crf[c].toe = uni(sp.crf[c].toe);
        p.crf[c].shoulder = uni(sp.crf[c].shoulder);
        p.crf[c].gamma = uni(sp.crf[c].gamma);
        p.crf[c].centre = uni(sp.crf[c].centre);
        p.crf[c].a = uni(sp.crf[c].a);
        p.crf[c].b = uni(sp.crf[c].b);
        p.crf[c].inv_centre = uni(sp.crf[c].inv_centre);
        p.crf[c].inv_rest = uni(sp.crf[c].inv_rest);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) p.H[k] = uni(sp.H[k]);
    p.stages = __builtin_amdgcn_readfirstlane(sp.stages);
    return p;
}

// kPix pixels' worth of an N-floats-per-pixel array starting at pixel `first`; pixels at or beyond P read as 0 / are not written.
// VEC: the array's base is 16-byte aligned, so a full group moves as float4.
template <int N, bool VEC>
__device__ __forceinline__ void load_group(const float* __restrict__ src, uint64_t first, uint32_t P, float (&v)[kPix * N]) {
    const float* p = src + first * N;
    if (first + kPix <= P) {
        if (VEC) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const float4 q = reinterpret_cast<const float4*>(p)[i];
                v[4 * i] = q.x, v[4 * i + 1] = q.y, v[4 * i + 2] = q.z, v[4 * i + 3] = q.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kPix * N; ++i) v[i] = p[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < kPix * N; ++i) v[i] = first + i / N < P ? p[i] : 0.f;
    }
}
template <int N, bool VEC>
__device__ __forceinline__ void store_group(float* __restrict__ dst, uint64_t first, uint32_t P, const float (&v)[kPix * N]) {
    float* p = dst + first * N;
    if (first + kPix <= P) {
        if (VEC) {
#pragma unroll
            for (int i = 0; i < N; ++i) reinterpret_cast<float4*>(p)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < kPix * N; ++i) p[i] = v[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < kPix * N; ++i)
            if (first + i / N < P) p[i] = v[i];
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void ppisp_forward_kernel(uint32_t P, const float* __restrict__ rgb, const float* __restrict__ pc, Params a,
                                                               float* __restrict__ out) {
    const Prep prep = block_prep(a);
    const uint64_t groups = ((uint64_t)P + kPix - 1) / kPix;
    float acc[3][16];   // never touched by the forward instantiation
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * kBlock) {
        const uint64_t first = g * kPix;
        float in[kPix * 3], xy[kPix * 2] = {}, o[kPix * 3];
        load_group<3, VEC>(rgb, first, P, in);
        if (prep.stages & HAS_VIGNETTING) load_group<2, VEC>(pc, first, P, xy);
#pragma unroll
        for (int j = 0; j < kPix; ++j) pixel<false>(prep, in + 3 * j, xy[2 * j], xy[2 * j + 1], o + 3 * j, nullptr, nullptr, acc);
        store_group<3, VEC>(out, first, P, o);
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void ppisp_backward_kernel(uint32_t P, const float* __restrict__ rgb, const float* __restrict__ pc, Params a,
                                                                const float* __restrict__ grad_out, float* __restrict__ grad_rgb,
                                                                float* __restrict__ partials) {
    const Prep prep = block_prep(a);
    const uint64_t groups = ((uint64_t)P + kPix - 1) / kPix;
    float acc[3][16];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[i][k] = 0.f;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * kBlock) {
        const uint64_t first = g * kPix;
        float in[kPix * 3], xy[kPix * 2] = {}, go[kPix * 3], gin[kPix * 3], o[3];
        load_group<3, VEC>(rgb, first, P, in);
        load_group<3, VEC>(grad_out, first, P, go);   // 0 beyond P: such a pixel adds nothing to any sum
        if (prep.stages & HAS_VIGNETTING) load_group<2, VEC>(pc, first, P, xy);
#pragma unroll
        for (int j = 0; j < kPix; ++j) pixel<true>(prep, in + 3 * j, xy[2 * j], xy[2 * j + 1], o, go + 3 * j, gin + 3 * j, acc);
        if (grad_rgb) store_group<3, VEC>(grad_rgb, first, P, gin);
    }
    // wave: lane l ends up with the wave's total of slot 16 i + (l & 15); block: the waves' totals added in wave order
    __shared__ float red[kWaves][kRow];
    const int lane = lane_id(), wave = threadIdx.x / GRUT_WAVE;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t = wave_reduce_scatter16(acc[i], lane);
        if (lane < 16) red[wave][16 * i + lane] = t;
    }
    __syncthreads();
    if (threadIdx.x < kRow) {
        float t = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += red[w][threadIdx.x];
        partials[(size_t)blockIdx.x * kRow + threadIdx.x] = t;
    }
}

// one block: column c of the rows is summed by kFinishGroups lanes (rows g, g + 21, ...), their sums are added in group order, and lane 0
// turns the row of gradients against the activated quantities into gradients of the raw parameter rows
__global__ __launch_bounds__(1024) void ppisp_finish_kernel(uint32_t rows, const float* __restrict__ partials, Params a, float* g_exposure,
                                                            float* g_color, float* g_vignetting, float* g_crf) {
    __shared__ float part[kFinishGroups][kRow];
    __shared__ float row[kRow];
    const int t = threadIdx.x;
    if (t < kFinishThreads) {
        const int col = t % kRow, grp = t / kRow;
        float s = 0.f;
        for (uint32_t r = grp; r < rows; r += kFinishGroups) s += partials[(size_t)r * kRow + col];
        part[grp][col] = s;
    }
    __syncthreads();
    if (t < kRow) {
        float s = part[0][t];
        for (int g = 1; g < kFinishGroups; ++g) s += part[g][t];
        row[t] = s;
    }
    __syncthreads();
    if (t == 0) finish(row, a.exposure, a.color, a.crf, g_exposure, g_color, g_vignetting, g_crf);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace
}  // namespace grut

using namespace grut;

extern "C" uint32_t grut_ppisp_partials(uint32_t num_pixels) { return num_pixels ? num_blocks(num_pixels) * ppisp::kRow : 0u; }

extern "C" int grut_ppisp_forward(void* stream, uint32_t P, const float* rgb, const float* pixel_coords, float res_w, float res_h,
                                  const float* exposure, const float* color, const float* vignetting, const float* crf, float* out) {
    GRUT_REQUIRE(P > 0 && rgb && out, "grut_ppisp_forward: num_pixels > 0, rgb and out are required");
    GRUT_REQUIRE(!vignetting || pixel_coords, "grut_ppisp_forward: the vignetting stage needs pixel_coords");
    GRUT_REQUIRE(!vignetting || (res_w > 0.f && res_h > 0.f), "grut_ppisp_forward: the vignetting stage needs a positive resolution");
    const Params a{exposure, color, vignetting, crf, res_w, res_h};
    const hipStream_t s = (hipStream_t)stream;
    if (aligned16(rgb) && aligned16(out) && aligned16(pixel_coords))
        ppisp_forward_kernel<true><<<num_blocks(P), kBlock, 0, s>>>(P, rgb, pixel_coords, a, out);
    else
        ppisp_forward_kernel<false><<<num_blocks(P), kBlock, 0, s>>>(P, rgb, pixel_coords, a, out);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_ppisp_backward(void* stream, uint32_t P, const float* rgb, const float* pixel_coords, float res_w, float res_h,
                                   const float* exposure, const float* color, const float* vignetting, const float* crf, const float* grad_out,
                                   float* grad_rgb, float* grad_exposure, float* grad_color, float* grad_vignetting, float* grad_crf,
                                   float* partials) {
    GRUT_REQUIRE(P > 0 && rgb && grad_out && partials, "grut_ppisp_backward: num_pixels > 0, rgb, grad_out and partials are required");
    GRUT_REQUIRE(!vignetting || pixel_coords, "grut_ppisp_backward: the vignetting stage needs pixel_coords");
    GRUT_REQUIRE(!vignetting || (res_w > 0.f && res_h > 0.f), "grut_ppisp_backward: the vignetting stage needs a positive resolution");
    GRUT_REQUIRE((exposure || !grad_exposure) && (color || !grad_color) && (vignetting || !grad_vignetting) && (crf || !grad_crf),
                 "grut_ppisp_backward: a stage without parameters (NULL) has no gradient to write: its gradient pointer must be NULL too");
    const Params a{exposure, color, vignetting, crf, res_w, res_h};
    const hipStream_t s = (hipStream_t)stream;
    const uint32_t blocks = num_blocks(P);
    if (aligned16(rgb) && aligned16(grad_out) && aligned16(grad_rgb) && aligned16(pixel_coords))
        ppisp_backward_kernel<true><<<blocks, kBlock, 0, s>>>(P, rgb, pixel_coords, a, grad_out, grad_rgb, partials);
    else
        ppisp_backward_kernel<false><<<blocks, kBlock, 0, s>>>(P, rgb, pixel_coords, a, grad_out, grad_rgb, partials);
    GRUT_HIP(hipGetLastError());
    if (grad_exposure || grad_color || grad_vignetting || grad_crf) {
        ppisp_finish_kernel<<<1, 1024, 0, s>>>(blocks, partials, a, grad_exposure, grad_color, grad_vignetting, grad_crf);
        GRUT_HIP(hipGetLastError());
    }
    return GRUT_OK;
}
