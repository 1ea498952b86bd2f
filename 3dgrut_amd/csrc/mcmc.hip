// mcmc.hip — the two device passes of the MCMC densification strategy (threedgrut/strategy/mcmc.py).
//
//   * relocation: the opacity / scale of a Gaussian that is split into n copies (Eq. 9 of "3D Gaussian Splatting as Markov Chain
//     Monte Carlo"); replaces compute_relocation_kernel (threedgrut/strategy/src/gaussian_mcmc.cu:36-66), one lane per sampled
//     Gaussian, same arithmetic and summation order.
//   * perturbation: positions += R S S^T R^T (noise * sigmoid_100(1 - density) * noise_lr * lr), the whole of
//     MCMCStrategy.perturb_gaussians (mcmc.py:167-187) after the noise draw in ONE pass instead of a few dozen torch launches
//     over [N,3,3] / [N,3] temporaries.  HBM-bound: 56 B read (rotation 16, scale 12, density 4, noise 12, positions 12) and 12 B
//     written per Gaussian.
#include "common.hpp"
#include "mcmc_device.inl"

namespace grut {

constexpr int kMcmcThreads = 256;

// ---- relocation ------------------------------------------------------------------------------------------------------------------
// The formula itself is mcmc_relocation_values (mcmc_device.inl), shared with the event plan of mcmc_events.hip.
__global__ __launch_bounds__(kMcmcThreads) void mcmc_relocation_kernel(uint32_t n, const float* __restrict__ opacities,
                                                                       const float* __restrict__ scales, const int32_t* __restrict__ ratios,
                                                                       const float* __restrict__ binoms, int n_max,
                                                                       float* __restrict__ new_opacities, float* __restrict__ new_scales) {
    const uint32_t idx = blockIdx.x * kMcmcThreads + threadIdx.x;
    if (idx >= n) return;
    const float o = opacities[idx];
    float new_o, coeff;
    mcmc_relocation_values(o, ratios[idx], binoms, n_max, new_o, coeff);
    new_opacities[idx] = new_o;
    const size_t s = 3 * (size_t)idx;
    new_scales[s] = coeff * scales[s];
    new_scales[s + 1] = coeff * scales[s + 1];
    new_scales[s + 2] = coeff * scales[s + 2];
}

// ---- fused perturbation ----------------------------------------------------------------------------------------------------------
// One lane per Gaussian, 256 Gaussians per block.  The three [N,3] streams (scale, noise, positions) are staged through LDS with
// dword loads at lane stride (a block's 768 contiguous words in three fully coalesced instructions per stream) and read back at a
// 3-word lane stride (odd: no bank conflict); rotation is one float4 per lane, density one word.  positions is written back through
// LDS the same way.  Nothing is allocated; the caller's noise buffer holds torch.randn_like(positions) (the generator stays the
// reference's, mcmc.py:182).
__global__ __launch_bounds__(kMcmcThreads) void mcmc_perturb_kernel(uint32_t n, float* __restrict__ positions, const float4* __restrict__ rotation,
                                                                    const float* __restrict__ scale, const float* __restrict__ density,
                                                                    const float* __restrict__ noise, float noise_lr, float lr, int activated) {
    __shared__ float s_scl[3 * kMcmcThreads], s_nse[3 * kMcmcThreads], s_pos[3 * kMcmcThreads];
    const uint32_t first = blockIdx.x * kMcmcThreads;
    const uint32_t rows = min((uint32_t)kMcmcThreads, n - first);
    const size_t base = 3 * (size_t)first;
    const uint32_t words = 3u * rows;
    for (uint32_t w = threadIdx.x; w < words; w += kMcmcThreads) {
        s_scl[w] = scale[base + w];
        s_nse[w] = noise[base + w];
        s_pos[w] = positions[base + w];
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < rows) {
        const uint32_t i = first + t;
        float4 q = rotation[i];
        float sx = s_scl[3 * t], sy = s_scl[3 * t + 1], sz = s_scl[3 * t + 2];
        float d = density[i];
        if (!activated) {   // the model's default activations (model.py:102-118, utils/misc.py:44-49): normalize (eps 1e-12), exp, sigmoid
            const float len = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
            q = make_float4(q.x / len, q.y / len, q.z / len, q.w / len);
            sx = expf(sx); sy = expf(sy); sz = expf(sz);
            d = 1.0f / (1.0f + expf(-d));
        }
        // quaternion_to_so3 (utils/misc.py:67-88) normalises again; q = (r, x, y, z)
        const float norm = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
        const float r = q.x / norm, x = q.y / norm, y = q.z / norm, z = q.w / norm;
        const float R[3][3] = {{1.0f - 2.0f * (y * y + z * z), 2.0f * (x * y - r * z), 2.0f * (x * z + r * y)},
                               {2.0f * (x * y + r * z), 1.0f - 2.0f * (x * x + z * z), 2.0f * (y * z - r * x)},
                               {2.0f * (x * z - r * y), 2.0f * (y * z + r * x), 1.0f - 2.0f * (x * x + y * y)}};
        const float s[3] = {sx, sy, sz};
        // op_sigmoid(1 - d) (mcmc.py:177-178).  For dense particles exp overflows to +inf and 1 / (1 + inf) = 0: the noise vanishes.
        const float sg = 1.0f / (1.0f + expf(-100.0f * ((1.0f - d) - 0.995f)));
        // noise * sigmoid * noise_lr * lr, left to right as mcmc.py:181-183
        const float v[3] = {s_nse[3 * t] * sg * noise_lr * lr, s_nse[3 * t + 1] * sg * noise_lr * lr, s_nse[3 * t + 2] * sg * noise_lr * lr};
        // covariance (model.py:120-130): ((R S) S^T) R^T, then the batched matvec (mcmc.py:184)
        float A[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 3; ++k) A[a][k] = R[a][k] * s[k] * s[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float delta = 0.0f;
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const float cov = A[a][0] * R[b][0] + A[a][1] * R[b][1] + A[a][2] * R[b][2];
                delta += cov * v[b];
            }
            s_pos[3 * t + a] += delta;
        }
    }
    __syncthreads();
    for (uint32_t w = threadIdx.x; w < words; w += kMcmcThreads) positions[base + w] = s_pos[w];
}

}  // namespace grut

extern "C" int grut_mcmc_relocation(void* stream, uint32_t n, const float* opacities, const float* scales, const int32_t* ratios,
                                    const float* binoms, int n_max, float* new_opacities, float* new_scales) {
    using namespace grut;
    GRUT_REQUIRE(n_max >= 1, "grut_mcmc_relocation: n_max must be >= 1 (got %d)", n_max);
    if (n == 0) return GRUT_OK;
    GRUT_REQUIRE(opacities && scales && ratios && binoms && new_opacities && new_scales, "grut_mcmc_relocation: null tensor");
    hipLaunchKernelGGL(mcmc_relocation_kernel, dim3((uint32_t)(((uint64_t)n + kMcmcThreads - 1) / kMcmcThreads)), dim3(kMcmcThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), n, opacities, scales, ratios, binoms, n_max, new_opacities, new_scales);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_mcmc_perturb(void* stream, uint32_t n, float* positions, const float* rotation, const float* scale, const float* density,
                                 const float* noise, float noise_lr, float lr, int activated) {
    using namespace grut;
    GRUT_REQUIRE(activated == 0 || activated == 1, "grut_mcmc_perturb: activated must be 0 (raw parameters) or 1 (got %d)", activated);
    if (n == 0) return GRUT_OK;
    GRUT_REQUIRE(positions && rotation && scale && density && noise, "grut_mcmc_perturb: null tensor");
    GRUT_REQUIRE((uintptr_t)rotation % 16 == 0, "grut_mcmc_perturb: rotation must be 16-byte aligned");
    hipLaunchKernelGGL(mcmc_perturb_kernel, dim3((uint32_t)(((uint64_t)n + kMcmcThreads - 1) / kMcmcThreads)), dim3(kMcmcThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), n, positions, reinterpret_cast<const float4*>(rotation), scale, density, noise,
                       noise_lr, lr, activated);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}
