// regularizers.hip — the opacity and scale regularisers of the MCMC configurations (threedgrut/trainer.py:722-736 with
// configs/base_mcmc.yaml: loss.use_opacity, loss.use_scale), from the RAW parameter tensors:
//   mean_i sigmoid(raw_density[i])   and   mean_ij exp(raw_scale[i][j])        (abs of a non-negative value is the identity)
// and their gradients back to the raw tensors.  Replaces torch's sigmoid, abs, mean, exp, abs, mean (seven launches) with two and
// the autograd chain behind them (about ten) with one.  Pure streaming over the flat [N] and [3N] arrays in float4 (16 B per particle
// forward, 32 B backward) with one double-precision exponential per element: at the sizes this project runs the launches are the cost,
// DESIGN.md §7m.
//
// Order of summation (fp32, fixed: no atomics, bitwise reproducible):
//   lane    one float4 as (x + y) + (z + w); the trips of its grid-stride loop in a compensated (Kahan) sum, worth two roundings
//           however many trips there are (the grid is capped, so at large N a lane makes up to 4096 of them)
//   wave    DPP tree, ((r3 + r2) + (r1 + r0)) over rows summed as aligned halves: balanced, depth 6
//   block   (w0 + w1) + (w2 + w3) through LDS, one partial pair per block
//   finish  one block: thread t takes partial t, the same wave tree, then the 16 wave sums in one more tree: depth 10
// Quad q goes to lane q % 256 of block (q / 256) % grid, so the non-zero leaves of every tree are a prefix of it and adding the
// zeros behind them is exact: a term passes at most min(ceil(log2(count)), 22) roundings.
#include "common.hpp"

namespace grut {

constexpr int kRegThreads = 256;               // 4 waves
constexpr uint32_t kRegMaxBlocks = 1024;       // forward grid cap: partials are two floats per block, 8 KiB at most
constexpr int kRegFinishThreads = 1024;        // one thread per partial pair
constexpr uint32_t kRegBwdMaxBlocks = 2048;    // 8 blocks per CU, grid-stride beyond
static_assert(kRegFinishThreads == (int)kRegMaxBlocks, "the finishing block reads one partial pair per thread");

// The activations are evaluated in double and rounded to fp32 once.  The packing pass (optim.hip) takes 1 / (1 + expf(-x)) and expf(x),
// and the device's expf was measured up to 11 ulp from the exact value (12 288 inputs in [-15, 3], mean 1.8 ulp; torch's exp: 0.8) -
// more than the four ulp a gradient element is allowed here and than the whole bound of a sum of few terms.  The mean regularised is
// therefore that of the exact activation of the stored parameter; the value rendered is within those 11 ulp of it.
struct RegSigmoid { __device__ __forceinline__ float operator()(float x) const { return (float)(1.0 / (1.0 + exp(-(double)x))); } };
struct RegExp { __device__ __forceinline__ float operator()(float x) const { return (float)exp((double)x); } };

// sum of act(p[4q .. 4q+3]) over the elements below `count`; q < ceil(count / 4) <= 2^30, so 4q does not wrap and `left` >= 1
template <class Act>
__device__ __forceinline__ float reg_quad_sum(const float* __restrict__ p, uint32_t q, uint32_t count) {
    const Act act;
    const uint32_t base = 4u * q, left = count - base;
    if (left >= 4u) {
        const float4 v = *reinterpret_cast<const float4*>(p + base);
        return (act(v.x) + act(v.y)) + (act(v.z) + act(v.w));
    }
    const float a = act(p[base]);
    const float b = left > 1u ? act(p[base + 1]) : 0.f;
    const float c = left > 2u ? act(p[base + 2]) : 0.f;
    return (a + b) + c;
}

__device__ __forceinline__ void kahan_add(float& sum, float& comp, float v) {
    const float y = v - comp;
    const float t = sum + y;
    comp = (t - sum) - y;
    sum = t;
}

__device__ __forceinline__ uint32_t reg_quads(uint32_t count) { return count / 4u + (count % 4u != 0u ? 1u : 0u); }

__global__ __launch_bounds__(kRegThreads) void reg_partial_kernel(uint32_t n, const float* __restrict__ raw_dns, const float* __restrict__ raw_scl,
                                                                  float* __restrict__ partials) {
    const uint32_t count_s = 3u * n;
    const uint32_t quads_d = reg_quads(n), quads = raw_scl ? reg_quads(count_s) : quads_d;
    const uint32_t stride = gridDim.x * kRegThreads;   // <= 2^18, q < 2^30: q + stride does not wrap
    float sum_d = 0.f, comp_d = 0.f, sum_s = 0.f, comp_s = 0.f;
    for (uint32_t q = blockIdx.x * kRegThreads + threadIdx.x; q < quads; q += stride) {
        if (raw_scl) kahan_add(sum_s, comp_s, reg_quad_sum<RegExp>(raw_scl, q, count_s));
        if (raw_dns && q < quads_d) kahan_add(sum_d, comp_d, reg_quad_sum<RegSigmoid>(raw_dns, q, n));
    }
    sum_d = wave_sum_to_lane63(sum_d);
    sum_s = wave_sum_to_lane63(sum_s);
    __shared__ float wave_sums[2][kRegThreads / 64];
    if ((threadIdx.x & 63u) == 63u) {
        wave_sums[0][threadIdx.x >> 6] = sum_d;
        wave_sums[1][threadIdx.x >> 6] = sum_s;
    }
    __syncthreads();
    if (threadIdx.x < 2u) {
        const float* w = wave_sums[threadIdx.x];
        partials[2u * blockIdx.x + threadIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
    }
}

__global__ __launch_bounds__(kRegFinishThreads) void reg_finish_kernel(uint32_t n, uint32_t blocks, int has_dns, int has_scl,
                                                                       const float* __restrict__ partials, float* __restrict__ out) {
    const uint32_t t = threadIdx.x;
    float d = t < blocks ? partials[2u * t] : 0.f;
    float s = t < blocks ? partials[2u * t + 1u] : 0.f;
    d = wave_sum_to_lane63(d);
    s = wave_sum_to_lane63(s);
    __shared__ float wave_sums[2][kRegFinishThreads / 64];
    if ((t & 63u) == 63u) {
        wave_sums[0][t >> 6] = d;
        wave_sums[1][t >> 6] = s;
    }
    __syncthreads();
    if (t < 64u) {   // the 16 wave sums in row 0 of wave 0; rows 1-3 add zeros
        d = wave_sum_to_lane63(t < kRegFinishThreads / 64 ? wave_sums[0][t] : 0.f);
        s = wave_sum_to_lane63(t < kRegFinishThreads / 64 ? wave_sums[1][t] : 0.f);
        if (t == 63u) {
            out[0] = has_dns ? d / (float)n : 0.f;
            out[1] = has_scl ? s / (float)(3u * n) : 0.f;
        }
    }
}

// upstream * s (1 - s) as upstream * e / (1 + e)^2 with e = exp(-|x|): keeps its leading digits where s rounds to 1, cannot overflow,
// and is rounded to fp32 once
__device__ __forceinline__ float reg_dsigmoid(double upstream, float x) {
    const double e = exp(-fabs((double)x));
    const double p = 1.0 + e;
    return (float)(upstream * e / (p * p));
}
__device__ __forceinline__ float reg_dexp(double upstream, float x) { return (float)(upstream * exp((double)x)); }

__global__ __launch_bounds__(kRegThreads) void reg_backward_kernel(uint32_t n, const float* __restrict__ raw_dns, const float* __restrict__ raw_scl,
                                                                   const float* __restrict__ grad_out, float* __restrict__ g_dns,
                                                                   float* __restrict__ g_scl) {
    const uint32_t count_s = 3u * n;
    const uint32_t quads_d = reg_quads(n), quads = g_scl ? reg_quads(count_s) : quads_d;
    const double up_d = g_dns ? (double)grad_out[0] / (double)n : 0.0;
    const double up_s = g_scl ? (double)grad_out[1] / (double)count_s : 0.0;
    const uint32_t stride = gridDim.x * kRegThreads;
    for (uint32_t q = blockIdx.x * kRegThreads + threadIdx.x; q < quads; q += stride) {
        const uint32_t base = 4u * q;
        if (g_scl) {
            const uint32_t left = count_s - base;
            if (left >= 4u) {
                const float4 v = *reinterpret_cast<const float4*>(raw_scl + base);
                *reinterpret_cast<float4*>(g_scl + base) = make_float4(reg_dexp(up_s, v.x), reg_dexp(up_s, v.y), reg_dexp(up_s, v.z), reg_dexp(up_s, v.w));
            } else {
                for (uint32_t k = 0; k < left; ++k) g_scl[base + k] = reg_dexp(up_s, raw_scl[base + k]);
            }
        }
        if (g_dns && q < quads_d) {
            const uint32_t left = n - base;
            if (left >= 4u) {
                const float4 v = *reinterpret_cast<const float4*>(raw_dns + base);
                *reinterpret_cast<float4*>(g_dns + base) =
                    make_float4(reg_dsigmoid(up_d, v.x), reg_dsigmoid(up_d, v.y), reg_dsigmoid(up_d, v.z), reg_dsigmoid(up_d, v.w));
            } else {
                for (uint32_t k = 0; k < left; ++k) g_dns[base + k] = reg_dsigmoid(up_d, raw_dns[base + k]);
            }
        }
    }
}

static bool reg_count_ok(uint32_t n) { return n != 0u && n <= 0x55555555u; }   // 3 N < 2^32
static uint32_t reg_blocks(uint32_t count, uint32_t cap) {
    const uint32_t quads = count / 4u + (count % 4u != 0u ? 1u : 0u);
    const uint32_t blocks = (quads + (uint32_t)kRegThreads - 1u) / (uint32_t)kRegThreads;
    return blocks < cap ? blocks : cap;
}
static bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

}  // namespace grut

extern "C" uint32_t grut_reg_partials(uint32_t num_particles) {
    using namespace grut;
    return reg_count_ok(num_particles) ? 2u * reg_blocks(3u * num_particles, kRegMaxBlocks) : 0u;
}

extern "C" int grut_reg_forward(void* stream, uint32_t num_particles, const float* raw_density, const float* raw_scale, float* partials,
                                float* out) {
    using namespace grut;
    GRUT_REQUIRE(num_particles != 0u, "grut_reg_forward: num_particles is 0");
    GRUT_REQUIRE(reg_count_ok(num_particles), "grut_reg_forward: num_particles = %u, 3 N must be below 2^32", num_particles);
    GRUT_REQUIRE(raw_density || raw_scale, "grut_reg_forward: raw_density and raw_scale are both NULL");
    GRUT_REQUIRE(partials, "grut_reg_forward: partials is NULL");
    GRUT_REQUIRE(out, "grut_reg_forward: out is NULL");
    GRUT_REQUIRE(aligned16(raw_density), "grut_reg_forward: raw_density must be 16-byte aligned");
    GRUT_REQUIRE(aligned16(raw_scale), "grut_reg_forward: raw_scale must be 16-byte aligned");
    const uint32_t blocks = reg_blocks(3u * num_particles, kRegMaxBlocks);   // from N only, whichever terms are asked for
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(reg_partial_kernel, dim3(blocks), dim3(kRegThreads), 0, s, num_particles, raw_density, raw_scale, partials);
    GRUT_HIP(hipGetLastError());
    hipLaunchKernelGGL(reg_finish_kernel, dim3(1), dim3(kRegFinishThreads), 0, s, num_particles, blocks, raw_density ? 1 : 0, raw_scale ? 1 : 0,
                       (const float*)partials, out);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_reg_backward(void* stream, uint32_t num_particles, const float* raw_density, const float* raw_scale, const float* grad_out,
                                 float* grad_raw_density, float* grad_raw_scale) {
    using namespace grut;
    GRUT_REQUIRE(num_particles != 0u, "grut_reg_backward: num_particles is 0");
    GRUT_REQUIRE(reg_count_ok(num_particles), "grut_reg_backward: num_particles = %u, 3 N must be below 2^32", num_particles);
    GRUT_REQUIRE(raw_density || raw_scale, "grut_reg_backward: raw_density and raw_scale are both NULL");
    GRUT_REQUIRE(grad_out, "grut_reg_backward: grad_out is NULL");
    GRUT_REQUIRE(grad_raw_density || grad_raw_scale, "grut_reg_backward: grad_raw_density and grad_raw_scale are both NULL");
    GRUT_REQUIRE(!grad_raw_density || raw_density, "grut_reg_backward: grad_raw_density given but raw_density is NULL");
    GRUT_REQUIRE(!grad_raw_scale || raw_scale, "grut_reg_backward: grad_raw_scale given but raw_scale is NULL");
    GRUT_REQUIRE(aligned16(raw_density), "grut_reg_backward: raw_density must be 16-byte aligned");
    GRUT_REQUIRE(aligned16(raw_scale), "grut_reg_backward: raw_scale must be 16-byte aligned");
    GRUT_REQUIRE(aligned16(grad_raw_density), "grut_reg_backward: grad_raw_density must be 16-byte aligned");
    GRUT_REQUIRE(aligned16(grad_raw_scale), "grut_reg_backward: grad_raw_scale must be 16-byte aligned");
    const uint32_t blocks = reg_blocks(grad_raw_scale ? 3u * num_particles : num_particles, kRegBwdMaxBlocks);
    hipLaunchKernelGGL(reg_backward_kernel, dim3(blocks), dim3(kRegThreads), 0, reinterpret_cast<hipStream_t>(stream), num_particles,
                       raw_density, raw_scale, grad_out, grad_raw_density, grad_raw_scale);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}
