// mcmc_events.hip — the two periodic events of the MCMC densification strategy (threedgrut/strategy/mcmc.py) as fused passes.
//
//   * classify:  the two torch.where of relocate_gaussians (mcmc.py:112-116) and the gather densities[alive_idxs] of
//                sample_new_gaussians (:198) as one compaction on the scan of scan_sort.hip.
//   * plan:      valid_indices[sampled], bincount, its gather and clamp, the three gathers around compute_relocation_tensor, the
//                relocation itself and the two inverse activations (mcmc.py:202-222) in two kernels.
//   * relocate:  every indexed write of update_param_fn / update_optimizer_fn (mcmc.py:121-131) over ALL parameters and moments,
//                one launch.
//   * append:    the indexed writes, torch.cat and zeros + cat of add_new_gaussians (mcmc.py:148-158) over ALL parameters and
//                moments, one launch: each old row is read once and each new row written once.  HBM-bound.
// Nothing here allocates, synchronises or uses float atomics; scratch and outputs are the caller's.
#include <cfloat>

#include "common.hpp"
#include "mcmc_device.inl"

namespace grut {

namespace {

constexpr int kEvThreads = 256;
constexpr uint32_t kBodyWords = kEvThreads * 4 * 4;   // words a block copies of an appended tensor's old rows: 4 x 16 bytes per lane
constexpr uint32_t kRowWords = kEvThreads * 4;        // words a block moves of gathered rows: 4 per lane

inline uint32_t blocks_for(uint64_t items, uint32_t per_block) { return (uint32_t)((items + per_block - 1) / per_block); }
inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- classify --------------------------------------------------------------------------------------------------------------------
// NaN compares false both ways: such a row is in neither list, as with torch.where.
__global__ __launch_bounds__(kEvThreads) void mcmc_classify_flags_kernel(uint32_t n, const float* __restrict__ density, float threshold,
                                                                         uint32_t* __restrict__ dead_flag, uint32_t* __restrict__ alive_flag) {
    const uint32_t i = blockIdx.x * kEvThreads + threadIdx.x;
    if (i >= n) return;
    const float d = density[i];
    dead_flag[i] = d <= threshold;
    alive_flag[i] = d > threshold;
}

// rank (inclusive scan) -> position; ascending because the scan is.  The probabilities are the density's BITS.
__global__ __launch_bounds__(kEvThreads) void mcmc_classify_scatter_kernel(uint32_t n, const uint32_t* __restrict__ density_bits,
                                                                           const uint32_t* __restrict__ dead_flag,
                                                                           const uint32_t* __restrict__ alive_flag,
                                                                           const uint32_t* __restrict__ dead_rank,
                                                                           const uint32_t* __restrict__ alive_rank, int64_t* __restrict__ dead_idx,
                                                                           int64_t* __restrict__ alive_idx, uint32_t* __restrict__ alive_prob,
                                                                           uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * kEvThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t dr = dead_rank[i], ar = alive_rank[i];
    if (dead_flag[i]) dead_idx[dr - 1] = (int64_t)i;
    if (alive_flag[i]) {
        alive_idx[ar - 1] = (int64_t)i;
        alive_prob[ar - 1] = density_bits[i];
    }
    if (i == n - 1) {
        counts[0] = dr;
        counts[1] = ar;
    }
}

// ---- plan ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kEvThreads) void mcmc_plan_clear_kernel(uint32_t n, int32_t* __restrict__ count, int32_t* __restrict__ first) {
    const uint32_t i = blockIdx.x * kEvThreads + threadIdx.x;
    if (i >= n) return;
    count[i] = 0;
    first[i] = INT32_MAX;
}

// source = index_map[sampled] (or sampled), its histogram and the first draw of every source.  A draw outside [0, n_map) or a mapped
// index outside [0, n) cannot come out of torch.multinomial over n_map probabilities; it is clamped so that no access leaves the
// buffers.
__global__ __launch_bounds__(kEvThreads) void mcmc_plan_count_kernel(uint32_t m, uint32_t n, uint32_t n_map, const int64_t* __restrict__ sampled,
                                                                     const int64_t* __restrict__ index_map, int64_t* __restrict__ source,
                                                                     int32_t* __restrict__ count, int32_t* __restrict__ first) {
    const uint32_t j = blockIdx.x * kEvThreads + threadIdx.x;
    if (j >= m) return;
    int64_t s = sampled[j];
    if (index_map) {
        s = min(max(s, (int64_t)0), (int64_t)n_map - 1);
        s = index_map[s];
    }
    s = min(max(s, (int64_t)0), (int64_t)n - 1);
    source[j] = s;
    atomicAdd(&count[s], 1);
    atomicMin(&first[s], (int32_t)j);
}

// One lane per draw.  Draws of one source read the same density, scale row and count: their outputs are bit-identical.
__global__ __launch_bounds__(kEvThreads) void mcmc_plan_values_kernel(uint32_t m, const int64_t* __restrict__ source, const int32_t* __restrict__ count,
                                                                      const float* __restrict__ density, const float* __restrict__ scale,
                                                                      int scale_activated, const float* __restrict__ binoms, int n_max,
                                                                      float threshold, float* __restrict__ new_density_raw,
                                                                      float* __restrict__ new_scale_raw, float* __restrict__ new_density_act,
                                                                      float* __restrict__ new_scale_act) {
    const uint32_t j = blockIdx.x * kEvThreads + threadIdx.x;
    if (j >= m) return;
    const size_t src = (size_t)source[j];
    // (bincount[sampled] + 1).clamp_(1, n_max) (mcmc.py:204-206); the count is at most m < 2^31, the sum is formed in 64 bits
    const int ratio = (int)min((int64_t)count[src] + 1, (int64_t)n_max);
    const float o = density[src];
    float sx = scale[3 * src], sy = scale[3 * src + 1], sz = scale[3 * src + 2];
    if (!scale_activated) {   // the model's default scale activation (model.py:102-118), as in mcmc_perturb_kernel
        sx = expf(sx); sy = expf(sy); sz = expf(sz);
    }
    float new_o, coeff;
    mcmc_relocation_values(o, ratio, binoms, n_max, new_o, coeff);
    const float ax = coeff * sx, ay = coeff * sy, az = coeff * sz;
    const size_t r = 3 * (size_t)j;
    if (new_density_act) new_density_act[j] = new_o;
    if (new_scale_act) {
        new_scale_act[r] = ax;
        new_scale_act[r + 1] = ay;
        new_scale_act[r + 2] = az;
    }
    // density_activation_inv(clamp(new_o, threshold, 1 - eps)) = log(x / (1 - x)) (mcmc.py:216-220), scale_activation_inv = log (:222)
    const float x = fminf(fmaxf(new_o, threshold), 1.0f - FLT_EPSILON);
    new_density_raw[j] = logf(__fdiv_rn(x, 1.0f - x));
    new_scale_raw[r] = logf(ax);
    new_scale_raw[r + 1] = logf(ay);
    new_scale_raw[r + 2] = logf(az);
}

// ---- rows ------------------------------------------------------------------------------------------------------------------------
struct RowArgs {
    GrutMcmcTensor t[GRUT_MCMC_MAX_TENSORS];
    void* out[GRUT_MCMC_MAX_TENSORS];             // append only
    uint32_t block_start[GRUT_MCMC_MAX_TENSORS + 1];   // first block of tensor k in the 1-D grid
    uint32_t body_blocks[GRUT_MCMC_MAX_TENSORS];  // append only: blocks of tensor k that copy old rows; the rest gather the new ones
    uint32_t num;
};

// the tensor this block works on: a wave-uniform walk over at most 32 kernel-argument words
__device__ __forceinline__ uint32_t tensor_of_block(const RowArgs& a, uint32_t b) {
    uint32_t k = 0;
    while (k + 1 < a.num && b >= a.block_start[k + 1]) ++k;
    return k;
}

// (row, element) of word idx of a [rows, W] tensor.  W > 0: a constant (the division becomes a multiply); W = 0: run-time width.
template <int W>
__device__ __forceinline__ void split_index(uint64_t idx, uint32_t w_rt, uint32_t& row, uint32_t& e) {
    if (W == 1) {
        row = (uint32_t)idx;
        e = 0;
    } else {
        const uint64_t w = W ? (uint64_t)W : (uint64_t)w_rt;
        const uint64_t r = idx / w;
        row = (uint32_t)r;
        e = (uint32_t)(idx - r * w);
    }
}

// Relocation of m draws, in place.  Word (j, e) of the tensor's m x W work items:
//   COPY         data[dead[j]]   = data[source[j]]
//   NEW_*        data[dead[j]]   = new[j];  data[source[j]] = new[j] from the one j with first[source[j]] == j
//   STATE        data[source[j]] = 0        (dead rows keep their moments, mcmc.py:129-131)
// Race-free: every source is alive and every destination dead, so the rows read (sources) and the rows written by COPY / NEW_* at
// dead[j] are disjoint sets, dead[] holds no duplicates, and a source row is written only by the single lane set that owns `first`
// (NEW_*) or with the same zeros by every duplicate (STATE).  No row is both read and written within the launch.
template <int W>
__device__ __forceinline__ void relocate_rows_body(const GrutMcmcTensor& t, uint32_t block, uint32_t m, const int64_t* __restrict__ source,
                                                   const int64_t* __restrict__ dead, const int32_t* __restrict__ first,
                                                   const uint32_t* __restrict__ new_density, const uint32_t* __restrict__ new_scale) {
    const uint32_t w = W ? (uint32_t)W : t.row_elems;
    const uint64_t total = (uint64_t)m * w;
    uint32_t* __restrict__ data = reinterpret_cast<uint32_t*>(t.data);
    const uint64_t base = (uint64_t)block * kRowWords + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t idx = base + (uint64_t)k * kEvThreads;
        if (idx >= total) return;
        uint32_t j, e;
        split_index<W>(idx, w, j, e);
        const uint64_t src = (uint64_t)source[j];
        if (t.role == GRUT_MCMC_ROLE_STATE) {
            data[src * w + e] = 0u;
            continue;
        }
        const uint64_t dst = (uint64_t)dead[j];
        if (t.role == GRUT_MCMC_ROLE_COPY) {
            data[dst * w + e] = data[src * w + e];
        } else {
            const uint32_t v = (t.role == GRUT_MCMC_ROLE_NEW_DENSITY ? new_density : new_scale)[idx];
            data[dst * w + e] = v;
            if (first[src] == (int32_t)j) data[src * w + e] = v;
        }
    }
}

__global__ __launch_bounds__(kEvThreads) void mcmc_relocate_rows_kernel(RowArgs a, uint32_t m, const int64_t* __restrict__ source,
                                                                        const int64_t* __restrict__ dead, const int32_t* __restrict__ first,
                                                                        const uint32_t* __restrict__ new_density,
                                                                        const uint32_t* __restrict__ new_scale) {
    const uint32_t k = tensor_of_block(a, blockIdx.x);
    const GrutMcmcTensor t = a.t[k];
    const uint32_t block = blockIdx.x - a.block_start[k];
    switch (t.row_elems) {   // the row widths of the model's tensors (density, positions / scale / albedo, rotation, SH degree 3)
        case 1: relocate_rows_body<1>(t, block, m, source, dead, first, new_density, new_scale); break;
        case 3: relocate_rows_body<3>(t, block, m, source, dead, first, new_density, new_scale); break;
        case 4: relocate_rows_body<4>(t, block, m, source, dead, first, new_density, new_scale); break;
        case 45: relocate_rows_body<45>(t, block, m, source, dead, first, new_density, new_scale); break;
        default: relocate_rows_body<0>(t, block, m, source, dead, first, new_density, new_scale); break;
    }
}

// Append of m draws: out [n + m, W].  The first body_blocks of a tensor move the n old rows, the others write the m new ones.
//   old rows   out[i] = in[i]; NEW_* (W = 1 resp. 3, checked on the host): new[first[i]] where count[i] > 0.  Without a substitution
//              this is a flat copy that needs no row index: 16 bytes per access when both bases are 16-byte aligned, 4 x 16 bytes per
//              lane, the last n W mod 4 words one by one.
//   new rows   out[n + j] = in[source[j]] (COPY), new[j] (NEW_*: what out[source[j]] holds), 0 (STATE)
// `in` is only read and `out` only written, each word of out by exactly one lane.
template <int W>
__device__ __forceinline__ void append_rows_body(const GrutMcmcTensor& t, uint32_t* __restrict__ out, uint32_t block, uint32_t body_blocks,
                                                 uint32_t n, uint32_t m, const int64_t* __restrict__ source, const int32_t* __restrict__ count,
                                                 const int32_t* __restrict__ first, const uint32_t* __restrict__ new_density,
                                                 const uint32_t* __restrict__ new_scale) {
    const uint32_t w = W ? (uint32_t)W : t.row_elems;
    const uint32_t* __restrict__ in = reinterpret_cast<const uint32_t*>(t.data);
    const bool is_new = t.role == GRUT_MCMC_ROLE_NEW_DENSITY || t.role == GRUT_MCMC_ROLE_NEW_SCALE;
    const uint32_t* __restrict__ fresh = t.role == GRUT_MCMC_ROLE_NEW_DENSITY ? new_density : new_scale;
    if (block < body_blocks) {
        const uint64_t total = (uint64_t)n * w;
        const uint64_t first_word = (uint64_t)block * kBodyWords;
        if (is_new) {
#pragma unroll 4
            for (int k = 0; k < 16; ++k) {
                const uint64_t idx = first_word + (uint64_t)k * kEvThreads + threadIdx.x;
                if (idx >= total) return;
                uint32_t i, e;
                split_index<W>(idx, w, i, e);
                out[idx] = count[i] > 0 ? fresh[(uint64_t)first[i] * w + e] : in[idx];
            }
            return;
        }
        const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
        if (vec) {
            const uint64_t total4 = total >> 2;
            const uint4* __restrict__ in4 = reinterpret_cast<const uint4*>(in);
            uint4* __restrict__ out4 = reinterpret_cast<uint4*>(out);
            const uint64_t v0 = (first_word >> 2) + threadIdx.x;
            if ((first_word >> 2) + 4 * kEvThreads <= total4) {   // a whole block: four loads in flight per lane, then four stores
                const uint4 a = in4[v0], b = in4[v0 + kEvThreads], c = in4[v0 + 2 * kEvThreads], d = in4[v0 + 3 * kEvThreads];
                out4[v0] = a;
                out4[v0 + kEvThreads] = b;
                out4[v0 + 2 * kEvThreads] = c;
                out4[v0 + 3 * kEvThreads] = d;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint64_t i4 = v0 + (uint64_t)k * kEvThreads;
                    if (i4 < total4) out4[i4] = in4[i4];
                }
            }
            // the words after the last whole 16 bytes, by the block that holds the end
            const uint64_t rest = (total4 << 2) + threadIdx.x;
            if (block == body_blocks - 1 && rest < total) out[rest] = in[rest];
        } else {
#pragma unroll 4
            for (int k = 0; k < 16; ++k) {
                const uint64_t idx = first_word + (uint64_t)k * kEvThreads + threadIdx.x;
                if (idx >= total) return;
                out[idx] = in[idx];
            }
        }
        return;
    }
    const uint64_t total = (uint64_t)m * w;
    const uint64_t base = (uint64_t)(block - body_blocks) * kRowWords + threadIdx.x;
    uint32_t* __restrict__ tail = out + (uint64_t)n * w;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t idx = base + (uint64_t)k * kEvThreads;
        if (idx >= total) return;
        if (t.role == GRUT_MCMC_ROLE_STATE) {
            tail[idx] = 0u;
        } else if (is_new) {
            tail[idx] = fresh[idx];
        } else {
            uint32_t j, e;
            split_index<W>(idx, w, j, e);
            tail[idx] = in[(uint64_t)source[j] * w + e];
        }
    }
}

__global__ __launch_bounds__(kEvThreads) void mcmc_append_rows_kernel(RowArgs a, uint32_t n, uint32_t m, const int64_t* __restrict__ source,
                                                                      const int32_t* __restrict__ count, const int32_t* __restrict__ first,
                                                                      const uint32_t* __restrict__ new_density,
                                                                      const uint32_t* __restrict__ new_scale) {
    const uint32_t k = tensor_of_block(a, blockIdx.x);
    const GrutMcmcTensor t = a.t[k];
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out[k]);
    const uint32_t block = blockIdx.x - a.block_start[k], body = a.body_blocks[k];
    switch (t.row_elems) {
        case 1: append_rows_body<1>(t, out, block, body, n, m, source, count, first, new_density, new_scale); break;
        case 3: append_rows_body<3>(t, out, block, body, n, m, source, count, first, new_density, new_scale); break;
        case 4: append_rows_body<4>(t, out, block, body, n, m, source, count, first, new_density, new_scale); break;
        case 45: append_rows_body<45>(t, out, block, body, n, m, source, count, first, new_density, new_scale); break;
        default: append_rows_body<0>(t, out, block, body, n, m, source, count, first, new_density, new_scale); break;
    }
}

// what the two row entry points require of their descriptors; 0 on success
int check_tensors(const char* who, const GrutMcmcTensor* tensors, uint32_t num_tensors, void* const* outs, uint32_t m,
                  const void* new_density, const void* new_scale) {
    GRUT_REQUIRE(num_tensors <= GRUT_MCMC_MAX_TENSORS, "%s: num_tensors (%u) exceeds %d", who, num_tensors, GRUT_MCMC_MAX_TENSORS);
    GRUT_REQUIRE(tensors || num_tensors == 0, "%s: tensors is null", who);
    for (uint32_t k = 0; k < num_tensors; ++k) {
        const GrutMcmcTensor& t = tensors[k];
        GRUT_REQUIRE(t.data, "%s: tensors[%u].data is null", who, k);
        GRUT_REQUIRE(!outs || outs[k], "%s: outs[%u] is null", who, k);
        GRUT_REQUIRE(t.row_elems >= 1, "%s: tensors[%u].row_elems must be >= 1", who, k);
        GRUT_REQUIRE(t.role <= GRUT_MCMC_ROLE_STATE, "%s: tensors[%u].role %u is unknown", who, k, t.role);
        GRUT_REQUIRE(t.role != GRUT_MCMC_ROLE_NEW_DENSITY || (t.row_elems == 1 && (new_density || m == 0)),
                     "%s: tensors[%u] has the NEW_DENSITY role: row_elems must be 1 and new_density given (unless m is 0)", who, k);
        GRUT_REQUIRE(t.role != GRUT_MCMC_ROLE_NEW_SCALE || (t.row_elems == 3 && (new_scale || m == 0)),
                     "%s: tensors[%u] has the NEW_SCALE role: row_elems must be 3 and new_scale given (unless m is 0)", who, k);
    }
    return GRUT_OK;
}

}  // namespace

}  // namespace grut

// scratch: [n] dead flags | [n] alive flags | [n] dead ranks | [n] alive ranks (256-byte aligned each) | the scan's own scratch
extern "C" uint64_t grut_mcmc_classify_scratch_bytes(uint32_t n) {
    return 4 * (uint64_t)grut::align256((size_t)n * sizeof(uint32_t)) + grut::scan_scratch_bytes(n);
}

extern "C" int grut_mcmc_classify(void* stream, uint32_t n, const float* density, float threshold, int64_t* dead_idx, int64_t* alive_idx,
                                  float* alive_prob, uint32_t* counts, void* scratch, uint64_t scratch_bytes) {
    using namespace grut;
    GRUT_REQUIRE(n < 0x80000000u, "grut_mcmc_classify: n (%u) must be below 2^31", n);
    GRUT_REQUIRE(counts, "grut_mcmc_classify: counts is null");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n == 0) {
        GRUT_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(uint32_t), s));
        return GRUT_OK;
    }
    GRUT_REQUIRE(density, "grut_mcmc_classify: density is null");
    GRUT_REQUIRE(dead_idx, "grut_mcmc_classify: dead_idx is null");
    GRUT_REQUIRE(alive_idx, "grut_mcmc_classify: alive_idx is null");
    GRUT_REQUIRE(alive_prob, "grut_mcmc_classify: alive_prob is null");
    GRUT_REQUIRE(scratch && scratch_bytes >= grut_mcmc_classify_scratch_bytes(n), "grut_mcmc_classify: scratch too small (%llu bytes needed)",
                 (unsigned long long)grut_mcmc_classify_scratch_bytes(n));
    GRUT_REQUIRE((uintptr_t)scratch % 16 == 0, "grut_mcmc_classify: scratch must be 16-byte aligned");
    const size_t part = align256((size_t)n * sizeof(uint32_t));
    char* p = reinterpret_cast<char*>(scratch);
    uint32_t* dead_flag = reinterpret_cast<uint32_t*>(p);
    uint32_t* alive_flag = reinterpret_cast<uint32_t*>(p + part);
    uint32_t* dead_rank = reinterpret_cast<uint32_t*>(p + 2 * part);
    uint32_t* alive_rank = reinterpret_cast<uint32_t*>(p + 3 * part);
    void* scan_scratch = p + 4 * part;
    const size_t scan_bytes = scan_scratch_bytes(n);
    const dim3 grid(blocks_for(n, kEvThreads)), block(kEvThreads);
    hipLaunchKernelGGL(mcmc_classify_flags_kernel, grid, block, 0, s, n, density, threshold, dead_flag, alive_flag);
    GRUT_CHECK(inclusive_scan_u32(s, n, dead_flag, nullptr, dead_rank, scan_scratch, scan_bytes));
    GRUT_CHECK(inclusive_scan_u32(s, n, alive_flag, nullptr, alive_rank, scan_scratch, scan_bytes));
    hipLaunchKernelGGL(mcmc_classify_scatter_kernel, grid, block, 0, s, n, reinterpret_cast<const uint32_t*>(density), dead_flag, alive_flag,
                       dead_rank, alive_rank, dead_idx, alive_idx, reinterpret_cast<uint32_t*>(alive_prob), counts);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_mcmc_sample_plan(void* stream, uint32_t n, uint32_t m, const int64_t* sampled, const int64_t* index_map, uint32_t n_map,
                                     const float* density, const float* scale, int scale_activated, const float* binoms, int n_max,
                                     float threshold, int64_t* source, int32_t* count, int32_t* first, float* new_density_raw,
                                     float* new_scale_raw, float* new_density_act, float* new_scale_act) {
    using namespace grut;
    GRUT_REQUIRE(n < 0x80000000u && m < 0x80000000u, "grut_mcmc_sample_plan: n (%u) and m (%u) must be below 2^31", n, m);
    GRUT_REQUIRE(n_max >= 1, "grut_mcmc_sample_plan: n_max must be >= 1 (got %d)", n_max);
    GRUT_REQUIRE(scale_activated == 0 || scale_activated == 1, "grut_mcmc_sample_plan: scale_activated must be 0 (raw) or 1 (got %d)",
                 scale_activated);
    GRUT_REQUIRE(m == 0 || n > 0, "grut_mcmc_sample_plan: %u draws over no rows", m);
    GRUT_REQUIRE(!index_map || m == 0 || n_map > 0, "grut_mcmc_sample_plan: index_map given but n_map is 0");
    GRUT_REQUIRE(n_map <= n, "grut_mcmc_sample_plan: n_map (%u) exceeds n (%u)", n_map, n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n == 0) return GRUT_OK;   // (and m == 0 with it)
    GRUT_REQUIRE(count, "grut_mcmc_sample_plan: count is null");
    GRUT_REQUIRE(first, "grut_mcmc_sample_plan: first is null");
    if (m) {
        GRUT_REQUIRE(sampled, "grut_mcmc_sample_plan: sampled is null");
        GRUT_REQUIRE(density, "grut_mcmc_sample_plan: density is null");
        GRUT_REQUIRE(scale, "grut_mcmc_sample_plan: scale is null");
        GRUT_REQUIRE(binoms, "grut_mcmc_sample_plan: binoms is null");
        GRUT_REQUIRE(source, "grut_mcmc_sample_plan: source is null");
        GRUT_REQUIRE(new_density_raw, "grut_mcmc_sample_plan: new_density_raw is null");
        GRUT_REQUIRE(new_scale_raw, "grut_mcmc_sample_plan: new_scale_raw is null");
    }
    hipLaunchKernelGGL(mcmc_plan_clear_kernel, dim3(blocks_for(n, kEvThreads)), dim3(kEvThreads), 0, s, n, count, first);
    if (m) {
        const dim3 grid(blocks_for(m, kEvThreads)), block(kEvThreads);
        hipLaunchKernelGGL(mcmc_plan_count_kernel, grid, block, 0, s, m, n, index_map ? n_map : n, sampled, index_map, source, count, first);
        hipLaunchKernelGGL(mcmc_plan_values_kernel, grid, block, 0, s, m, source, count, density, scale, scale_activated, binoms, n_max,
                           threshold, new_density_raw, new_scale_raw, new_density_act, new_scale_act);
    }
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_mcmc_relocate_rows(void* stream, const GrutMcmcTensor* tensors, uint32_t num_tensors, uint32_t m, const int64_t* source,
                                       const int64_t* dead_idx, const int32_t* first, const float* new_density, const float* new_scale) {
    using namespace grut;
    GRUT_REQUIRE(m < 0x80000000u, "grut_mcmc_relocate_rows: m (%u) must be below 2^31", m);
    GRUT_CHECK(check_tensors("grut_mcmc_relocate_rows", tensors, num_tensors, nullptr, m, new_density, new_scale));
    if (m == 0 || num_tensors == 0) return GRUT_OK;
    GRUT_REQUIRE(source, "grut_mcmc_relocate_rows: source is null");
    GRUT_REQUIRE(dead_idx, "grut_mcmc_relocate_rows: dead_idx is null");
    GRUT_REQUIRE(first, "grut_mcmc_relocate_rows: first is null");
    RowArgs a;
    memset(&a, 0, sizeof(a));
    a.num = num_tensors;
    uint64_t blocks = 0;
    for (uint32_t k = 0; k < num_tensors; ++k) {
        a.t[k] = tensors[k];
        a.block_start[k] = (uint32_t)blocks;
        blocks += ((uint64_t)m * tensors[k].row_elems + kRowWords - 1) / kRowWords;
        GRUT_REQUIRE(blocks <= 0x7fffffffull, "grut_mcmc_relocate_rows: too much work for one launch (%llu blocks)", (unsigned long long)blocks);
    }
    a.block_start[num_tensors] = (uint32_t)blocks;
    hipLaunchKernelGGL(mcmc_relocate_rows_kernel, dim3((uint32_t)blocks), dim3(kEvThreads), 0, reinterpret_cast<hipStream_t>(stream), a, m, source,
                       dead_idx, first, reinterpret_cast<const uint32_t*>(new_density), reinterpret_cast<const uint32_t*>(new_scale));
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_mcmc_append_rows(void* stream, const GrutMcmcTensor* tensors, void* const* outs, uint32_t num_tensors, uint32_t n, uint32_t m,
                                     const int64_t* source, const int32_t* count, const int32_t* first, const float* new_density,
                                     const float* new_scale) {
    using namespace grut;
    GRUT_REQUIRE(n < 0x80000000u && m < 0x80000000u && (uint64_t)n + m < 0x80000000ull,
                 "grut_mcmc_append_rows: n (%u), m (%u) and n + m must be below 2^31", n, m);
    GRUT_REQUIRE(outs || num_tensors == 0, "grut_mcmc_append_rows: outs is null");
    GRUT_CHECK(check_tensors("grut_mcmc_append_rows", tensors, num_tensors, outs, m, new_density, new_scale));
    GRUT_REQUIRE(m == 0 || n > 0, "grut_mcmc_append_rows: %u draws over no rows", m);
    if ((uint64_t)n + m == 0 || num_tensors == 0) return GRUT_OK;
    if (m) GRUT_REQUIRE(source, "grut_mcmc_append_rows: source is null");
    bool any_new = false;
    for (uint32_t k = 0; k < num_tensors; ++k) any_new |= tensors[k].role == GRUT_MCMC_ROLE_NEW_DENSITY || tensors[k].role == GRUT_MCMC_ROLE_NEW_SCALE;
    if (any_new) {
        GRUT_REQUIRE(count, "grut_mcmc_append_rows: count is null");
        GRUT_REQUIRE(first, "grut_mcmc_append_rows: first is null");
    }
    RowArgs a;
    memset(&a, 0, sizeof(a));
    a.num = num_tensors;
    uint64_t blocks = 0;
    for (uint32_t k = 0; k < num_tensors; ++k) {
        a.t[k] = tensors[k];
        a.out[k] = outs[k];
        a.block_start[k] = (uint32_t)blocks;
        const uint64_t body = ((uint64_t)n * tensors[k].row_elems + kBodyWords - 1) / kBodyWords;
        GRUT_REQUIRE(body <= 0x7fffffffull, "grut_mcmc_append_rows: tensors[%u] is too large", k);
        a.body_blocks[k] = (uint32_t)body;
        blocks += body + ((uint64_t)m * tensors[k].row_elems + kRowWords - 1) / kRowWords;
        GRUT_REQUIRE(blocks <= 0x7fffffffull, "grut_mcmc_append_rows: too much work for one launch (%llu blocks)", (unsigned long long)blocks);
    }
    a.block_start[num_tensors] = (uint32_t)blocks;
    hipLaunchKernelGGL(mcmc_append_rows_kernel, dim3((uint32_t)blocks), dim3(kEvThreads), 0, reinterpret_cast<hipStream_t>(stream), a, n, m, source,
                       count, first, reinterpret_cast<const uint32_t*>(new_density), reinterpret_cast<const uint32_t*>(new_scale));
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}
