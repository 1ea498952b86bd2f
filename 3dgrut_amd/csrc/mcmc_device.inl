// mcmc_device.inl — the relocation formula shared by mcmc_relocation_kernel (mcmc.hip) and mcmc_sample_plan_kernel (mcmc_events.hip).
#pragma once

namespace grut {

// new_opacity = 1 - (1 - o)^(1/n)
// new_scale   = coeff * scale,  coeff = o / D,  D = sum_{i=1..n} sum_{k=0..i-1} binoms[(i-1) n_max + k] (-1)^k / sqrt(k+1) new_opacity^(k+1)
// D is an alternating sum that cancels by up to ~3 decades in fp32 at large n; the reference's result IS that fp32 sum in this order
// (i outer, k inner, one running sum), so it is evaluated term by term and not through a closed form.
// n is clamped to [1, n_max]: the reference's caller always clamps (mcmc.py:203-205) and the table holds n_max rows of n_max entries,
// so the clamp keeps every binoms read inside [0, n_max^2) whatever the caller passes.
__device__ __forceinline__ void mcmc_relocation_values(float o, int ratio, const float* __restrict__ binoms, int n_max, float& new_o,
                                                       float& coeff) {
    const int copies = min(max(ratio, 1), n_max);
    new_o = 1.0f - powf(1.0f - o, 1.0f / (float)copies);
    float denom = 0.0f;
    for (int i = 1; i <= copies; ++i) {
        const float* row = binoms + (size_t)(i - 1) * (size_t)n_max;
        for (int k = 0; k < i; ++k) {
            const float term = ((k & 1) ? -1.0f : 1.0f) / sqrtf((float)(k + 1)) * powf(new_o, (float)(k + 1));
            denom += row[k] * term;
        }
    }
    coeff = o / denom;
}

}  // namespace grut
