// densify.hip — the device passes of the default densification strategy (threedgrut/strategy/gs.py).
//
//   * accumulate: GSStrategy.update_gradient_buffer (gs.py:131-139) in ONE pass, one lane per particle.  The reference builds a boolean
//     mask and indexes with it four times (a nonzero + host wait each) around a dozen N-sized temporaries; the arithmetic is 3 loads,
//     3 loads and two read-modify-writes.  40 B of traffic per particle with a gradient, 12 B for the others.
//   * relayout: what clone / split / prune do to every parameter and optimizer-state tensor through _update_param_with_optimizer
//     (strategy/base.py:76-107): out = cat([v[keep], v[append].repeat(copies, 1)]) (or zeros for the appended block).  One scan of the
//     two masks gives every row its destinations; one flattened copy kernel per tensor moves it: each source row is read once and
//     written up to 1 + copies times, no temporaries.
//   * split tail: the appended block of a split (gs.py:168-186): positions += R(q) (noise * exp(scale)), scale = log(exp(scale) / (0.8 k)).
// Nothing here allocates or synchronises; scratch and outputs are the caller's.
#include "common.hpp"

namespace grut {

namespace {

constexpr int kDensifyThreads = 256;
constexpr int kWordsPerThread = 4;   // words per thread of the relayout copy (a block moves 1024 consecutive words)

inline uint32_t blocks_for(uint64_t items, uint32_t per_block) { return (uint32_t)((items + per_block - 1) / per_block); }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- gradient statistic ----------------------------------------------------------------------------------------------------------
// accum[i] += || g_i * ||p_i - c||_2 ||_2 / 2, denom[i] += 1 for the rows with any non-zero (or NaN) gradient component; every other
// row is not touched.  c = sensor[0], sensor[stride], sensor[2 stride]: the caller's T_to_world[0, :3, 3] view read in place.
__global__ __launch_bounds__(kDensifyThreads) void densify_accumulate_kernel(uint32_t n, const float* __restrict__ grad,
                                                                             const float* __restrict__ positions,
                                                                             const float* __restrict__ sensor, int64_t sensor_stride,
                                                                             float* __restrict__ accum, int32_t* __restrict__ denom) {
    const uint32_t i = blockIdx.x * kDensifyThreads + threadIdx.x;
    if (i >= n) return;
    const size_t r = 3 * (size_t)i;
    const float gx = grad[r], gy = grad[r + 1], gz = grad[r + 2];
    if (!(gx != 0.0f || gy != 0.0f || gz != 0.0f)) return;   // NaN != 0 holds, as in torch
    const float dx = positions[r] - sensor[0], dy = positions[r + 1] - sensor[sensor_stride], dz = positions[r + 2] - sensor[2 * sensor_stride];
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    const float vx = gx * dist, vy = gy * dist, vz = gz * dist;
    accum[i] += sqrtf(vx * vx + vy * vy + vz * vz) / 2.0f;
    denom[i] += 1;
}

// ---- relayout: masks -> destinations ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDensifyThreads) void relayout_flags_kernel(uint32_t n, const uint8_t* __restrict__ keep,
                                                                         const uint8_t* __restrict__ append,
                                                                         uint32_t* __restrict__ keep_flag, uint32_t* __restrict__ append_flag) {
    const uint32_t i = blockIdx.x * kDensifyThreads + threadIdx.x;
    if (i >= n) return;
    if (keep) keep_flag[i] = keep[i] != 0;
    if (append) append_flag[i] = append[i] != 0;
}

// inclusive -> exclusive (in place), the defaults of a NULL mask (keep: identity, append: none) and the two totals
__global__ __launch_bounds__(kDensifyThreads) void relayout_offsets_kernel(uint32_t n, const uint32_t* __restrict__ keep_flag,
                                                                           const uint32_t* __restrict__ append_flag,
                                                                           uint32_t* __restrict__ keep_offset, uint32_t* __restrict__ append_offset,
                                                                           uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * kDensifyThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t k_incl = keep_flag ? keep_offset[i] : i + 1, a_incl = append_flag ? append_offset[i] : 0u;
    keep_offset[i] = keep_flag ? k_incl - keep_flag[i] : i;
    append_offset[i] = append_flag ? a_incl - append_flag[i] : 0u;
    if (i == n - 1) {
        counts[0] = k_incl;
        counts[1] = a_incl;
    }
}

// ---- relayout: one tensor --------------------------------------------------------------------------------------------------------
// Flattened over (row, element): consecutive lanes read consecutive words of `in` and write consecutive words of a destination row,
// so a 45-float SH row moves coalesced.  ROW > 0: row_elems is that constant (the division becomes a multiply); ROW = 0: run-time.
template <int ROW>
__global__ __launch_bounds__(kDensifyThreads) void relayout_rows_kernel(uint64_t total, uint32_t row_elems_rt, const uint32_t* __restrict__ in,
                                                                        const uint8_t* __restrict__ keep, const uint8_t* __restrict__ append,
                                                                        const uint32_t* __restrict__ keep_offset,
                                                                        const uint32_t* __restrict__ append_offset, uint32_t n_keep,
                                                                        uint32_t n_append, uint32_t copies, int zero, uint32_t* __restrict__ out) {
    const uint64_t row_elems = ROW ? (uint64_t)ROW : (uint64_t)row_elems_rt;
    const uint64_t base = (uint64_t)blockIdx.x * (kDensifyThreads * kWordsPerThread) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kWordsPerThread; ++k) {
        const uint64_t idx = base + (uint64_t)k * kDensifyThreads;
        if (idx >= total) return;
        const uint64_t row = idx / row_elems, e = idx - row * row_elems;
        const bool kept = keep ? keep[row] != 0 : true;
        const bool appended = append ? append[row] != 0 : false;
        if (!kept && !appended) continue;
        const uint32_t v = (kept || !zero) ? in[idx] : 0u;   // a dropped row that is zero-appended is not read
        if (kept) out[(uint64_t)keep_offset[row] * row_elems + e] = v;
        if (appended) {
            const uint32_t w = zero ? 0u : v;
            uint64_t dst = ((uint64_t)n_keep + append_offset[row]) * row_elems + e;
            for (uint32_t c = 0; c < copies; ++c, dst += (uint64_t)n_append * row_elems) out[dst] = w;
        }
    }
}

// ---- split tail ------------------------------------------------------------------------------------------------------------------
// One lane per appended row: positions += R(q / |q|) (noise * exp(scale)), then scale = log(exp(scale) / (0.8 copies)) (exp, divide,
// log in that order, as scale_activation_inv(scale_activation(.) / (0.8 k)) evaluates it; not scale - log(0.8 k)).  The lane reads its scale row before it writes it.
__global__ __launch_bounds__(kDensifyThreads) void split_tail_kernel(uint32_t m, float* __restrict__ positions, float* __restrict__ scale,
                                                                     const float* __restrict__ rotation, const float* __restrict__ noise,
                                                                     float divisor) {
    const uint32_t i = blockIdx.x * kDensifyThreads + threadIdx.x;
    if (i >= m) return;
    const size_t r3 = 3 * (size_t)i, r4 = 4 * (size_t)i;
    const float qw = rotation[r4], qx = rotation[r4 + 1], qy = rotation[r4 + 2], qz = rotation[r4 + 3];
    const float sx = expf(scale[r3]), sy = expf(scale[r3 + 1]), sz = expf(scale[r3 + 2]);
    // quaternion_to_so3 (utils/misc.py:67-88); q = (r, x, y, z)
    const float norm = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
    const float r = qw / norm, x = qx / norm, y = qy / norm, z = qz / norm;
    const float vx = noise[r3] * sx, vy = noise[r3 + 1] * sy, vz = noise[r3 + 2] * sz;   // torch.normal(0, stds): z * std
    const float ox = (1.0f - 2.0f * (y * y + z * z)) * vx + 2.0f * (x * y - r * z) * vy + 2.0f * (x * z + r * y) * vz;
    const float oy = 2.0f * (x * y + r * z) * vx + (1.0f - 2.0f * (x * x + z * z)) * vy + 2.0f * (y * z - r * x) * vz;
    const float oz = 2.0f * (x * z - r * y) * vx + 2.0f * (y * z + r * x) * vy + (1.0f - 2.0f * (x * x + y * y)) * vz;
    // ONE rounding at the magnitude of the position: a contracted p + R0 vx + R1 vy + R2 vz would round there three times
    positions[r3]     = add_rn(positions[r3], ox);
    positions[r3 + 1] = add_rn(positions[r3 + 1], oy);
    positions[r3 + 2] = add_rn(positions[r3 + 2], oz);
    // exp in fp32 as the reference's activation rounds it; the quotient and its logarithm in fp64, rounded once: at |scale| ~ 8 an fp32
    // logf alone may be an ulp (9.5e-7) off, on top of the quotient's rounding
    const double d = (double)divisor;
    scale[r3] = (float)log((double)sx / d);
    scale[r3 + 1] = (float)log((double)sy / d);
    scale[r3 + 2] = (float)log((double)sz / d);
}

}  // namespace

}  // namespace grut

extern "C" int grut_densify_accumulate(void* stream, uint32_t n, const float* positions_grad, const float* positions,
                                       const float* sensor_position, int64_t sensor_stride, float* accum, int32_t* denom) {
    using namespace grut;
    if (n == 0) return GRUT_OK;
    GRUT_REQUIRE(positions_grad && positions && sensor_position && accum && denom, "grut_densify_accumulate: null tensor");
    hipLaunchKernelGGL(densify_accumulate_kernel, dim3(blocks_for(n, kDensifyThreads)), dim3(kDensifyThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), n, positions_grad, positions, sensor_position, sensor_stride, accum, denom);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

// scratch: [n] keep flags | [n] append flags (256-byte aligned each) | the scan's own scratch
extern "C" uint64_t grut_relayout_scratch_bytes(uint32_t n) {
    return 2 * (uint64_t)grut::align256((size_t)n * sizeof(uint32_t)) + grut::scan_scratch_bytes(n);
}

extern "C" int grut_relayout_scan(void* stream, uint32_t n, const uint8_t* keep, const uint8_t* append, uint32_t* keep_offset,
                                  uint32_t* append_offset, uint32_t* counts, void* scratch, uint64_t scratch_bytes) {
    using namespace grut;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    GRUT_REQUIRE(counts, "grut_relayout_scan: counts is null");
    if (n == 0) {
        GRUT_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s));
        return GRUT_OK;
    }
    GRUT_REQUIRE(keep_offset && append_offset, "grut_relayout_scan: null offsets");
    GRUT_REQUIRE(scratch && scratch_bytes >= grut_relayout_scratch_bytes(n), "grut_relayout_scan: scratch too small (%llu bytes needed)",
                 (unsigned long long)grut_relayout_scratch_bytes(n));
    GRUT_REQUIRE((uintptr_t)scratch % 16 == 0 && (uintptr_t)keep_offset % 16 == 0 && (uintptr_t)append_offset % 16 == 0,
                 "grut_relayout_scan: scratch and offsets must be 16-byte aligned");
    const size_t flag_bytes = align256((size_t)n * sizeof(uint32_t));
    uint32_t* keep_flag = keep ? reinterpret_cast<uint32_t*>(scratch) : nullptr;
    uint32_t* append_flag = append ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(scratch) + flag_bytes) : nullptr;
    void* scan_scratch = reinterpret_cast<char*>(scratch) + 2 * flag_bytes;
    const size_t scan_bytes = scan_scratch_bytes(n);
    const dim3 grid(blocks_for(n, kDensifyThreads)), block(kDensifyThreads);
    if (keep || append) hipLaunchKernelGGL(relayout_flags_kernel, grid, block, 0, s, n, keep, append, keep_flag, append_flag);
    if (keep) GRUT_CHECK(inclusive_scan_u32(s, n, keep_flag, nullptr, keep_offset, scan_scratch, scan_bytes));
    if (append) GRUT_CHECK(inclusive_scan_u32(s, n, append_flag, nullptr, append_offset, scan_scratch, scan_bytes));
    hipLaunchKernelGGL(relayout_offsets_kernel, grid, block, 0, s, n, keep_flag, append_flag, keep_offset, append_offset, counts);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_relayout_rows(void* stream, uint32_t n, uint32_t row_elems, const void* in, const uint8_t* keep, const uint8_t* append,
                                  const uint32_t* keep_offset, const uint32_t* append_offset, uint32_t n_keep, uint32_t n_append,
                                  uint32_t copies, int append_mode, void* out) {
    using namespace grut;
    GRUT_REQUIRE(append_mode == GRUT_APPEND_COPY || append_mode == GRUT_APPEND_ZERO, "grut_relayout_rows: unknown append mode %d", append_mode);
    GRUT_REQUIRE(row_elems >= 1, "grut_relayout_rows: row_elems must be >= 1");
    GRUT_REQUIRE(n_keep <= n && n_append <= n, "grut_relayout_rows: n_keep (%u) / n_append (%u) exceed n (%u)", n_keep, n_append, n);
    GRUT_REQUIRE(keep || n_keep == n, "grut_relayout_rows: keep is null (all rows kept) but n_keep (%u) != n (%u)", n_keep, n);
    GRUT_REQUIRE(append || n_append == 0, "grut_relayout_rows: append is null (no rows appended) but n_append = %u", n_append);
    if (n == 0 || (uint64_t)n_keep + (uint64_t)copies * n_append == 0) return GRUT_OK;
    GRUT_REQUIRE(in && out && keep_offset && append_offset, "grut_relayout_rows: null tensor");
    const uint64_t total = (uint64_t)n * row_elems;
    const uint64_t nblocks = (total + kDensifyThreads * kWordsPerThread - 1) / (kDensifyThreads * kWordsPerThread);
    GRUT_REQUIRE(nblocks <= 0x7fffffffull, "grut_relayout_rows: tensor too large (%llu words)", (unsigned long long)total);
    const dim3 grid((uint32_t)nblocks), block(kDensifyThreads);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(in);
    uint32_t* dst = reinterpret_cast<uint32_t*>(out);
    const int zero = append_mode == GRUT_APPEND_ZERO;
#define GRUT_RELAYOUT_LAUNCH(ROW_)                                                                                                        \
    hipLaunchKernelGGL((relayout_rows_kernel<ROW_>), grid, block, 0, s, total, row_elems, src, keep, append, keep_offset, append_offset, \
                       n_keep, n_append, copies, zero, dst)
    switch (row_elems) {   // the row widths of the model's tensors (density, positions / scale / albedo, rotation, SH degree 3)
        case 1: GRUT_RELAYOUT_LAUNCH(1); break;
        case 3: GRUT_RELAYOUT_LAUNCH(3); break;
        case 4: GRUT_RELAYOUT_LAUNCH(4); break;
        case 45: GRUT_RELAYOUT_LAUNCH(45); break;
        default: GRUT_RELAYOUT_LAUNCH(0); break;
    }
#undef GRUT_RELAYOUT_LAUNCH
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_split_tail(void* stream, uint32_t n, float* positions_tail, float* scale_tail, const float* rotation_tail,
                               const float* noise, uint32_t copies) {
    using namespace grut;
    GRUT_REQUIRE(copies >= 1, "grut_split_tail: copies must be >= 1");
    if (n == 0) return GRUT_OK;
    GRUT_REQUIRE(positions_tail && scale_tail && rotation_tail && noise, "grut_split_tail: null tensor");
    hipLaunchKernelGGL(split_tail_kernel, dim3(blocks_for(n, kDensifyThreads)), dim3(kDensifyThreads), 0, reinterpret_cast<hipStream_t>(stream),
                       n, positions_tail, scale_tail, rotation_tail, noise, (float)(0.8 * (double)copies));   // the reference's Python double 0.8 * k, rounded once
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}
