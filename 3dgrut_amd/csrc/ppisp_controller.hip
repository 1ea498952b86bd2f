// ppisp_controller.hip — the PPISP per-camera controller (3dgrut_amd/ppisp.py: _PPISPController; the architecture the reference's exporter
// checks, export/usd/post_processing/ppisp_controller_weights.py) as fused HIP passes, all fp32:
//
//   hdr [H,W,3] -> conv1x1 3->16 -> max over 3x3 windows (dsH = H/3, dsW = W/3) -> ReLU -> conv1x1 16->32 -> ReLU -> conv1x1 32->64
//       -> adaptive average pool to 5x5 -> 1600 features (channel-major) ++ prior -> 128 -> 128 -> 128 (ReLU each) -> exposure [1], colour [8]
//
// Forward, three launches.
//   cnn_forward_kernel    a wave takes one UNIT: 64 consecutive downsampled pixels of one downsampled row, a lane per pixel.  The 2 720 CNN
//                         weights are read through the scalar cache (constant address space, wave-uniform indices).  The 64 outputs stay in
//                         registers; per column cell the unit touches, the wave's sum goes to scratch as P[channel][unit][gx].
//   pool_trunk0_kernel    block c finishes channel c's 25 cells (8 lanes per cell, rows then column chunks, fixed order; divides by the cell's
//                         pixel count) and multiplies them into trunk0's columns c*25 .. c*25+24: 64 blocks share the 820 KB matrix.
//   trunk_kernel          one block: adds the 64 partial products in channel order, the prior's column and the bias; trunk1, trunk2, heads
//                         (a wave per output row, lanes along the input, DPP sum).
// Backward (weight gradients only; the image is detached), five launches.  The CNN is recomputed from hdr.  Two identities keep the per-pixel
// work small: the gradient at conv3's output depends only on the cells a pixel lies in, so
//   dW3 = dFs x S,  S[cell][i] = sum of the ReLU'd conv2 output over the cell's pixels (the forward's pooling machinery on 32 channels),
//   dH2 (gradient at conv2's ReLU output) = sum over the pixel's cells of D2[cell][.],  D2 = dFs^T W3  (25 x 32, computed once),
// with dFs = dF / count.  What remains per pixel is conv2's transpose (512 FMA), the arg-max routing into conv1 (64 accumulators per lane)
// and conv2's weight gradient, a 32 x 17 GEMM (16 inputs + bias) with the pixel index as K: the wave stages its 64 pixels' (dZ2, h1) in LDS
// and runs 32 exact-fp32 MFMA 32x32x2 steps into 16 accumulator registers that persist over the wave's units.
//   trunk_backward_kernel one block: heads, trunk2, trunk1 (outer products written whole), dz0
//   trunk0_backward_kernel 51 blocks of 32 columns: dW0 = dz0 x [F, prior] written whole, dF = W0^T dz0, dFs = dF / count
//   d2_kernel             D2
//   cnn_backward_kernel   as above; one partial per block (waves added in order through LDS)
//   finish_kernel         fixed-order sums of the per-block partials and of S; dW3, db3
// No atomics, no allocation, no synchronisation; every summation order is a function of (h, w) alone, so two runs are bitwise equal.
// Max-pool ties go to the first maximum in row-major order (strict > while scanning); a ReLU passes gradient where its input is > 0.
#include "common.hpp"

namespace grut {
namespace {

constexpr int kC1 = 16, kC2 = 32, kC3 = 64, kGrid = 5, kCells = 25, kFeat = 1600, kIn = 1601, kHid = 128;
constexpr int kBlock = 256, kWaves = kBlock / GRUT_WAVE;
constexpr int kMaxDim = 16384;
constexpr uint32_t kMaxBwdBlocks = 512;   // partials: 512 x 1088 floats = 2.1 MiB
constexpr int kT0Cols = 32, kT0Blocks = (kIn + kT0Cols - 1) / kT0Cols;
constexpr int kStrideA = kC2 + 1, kStrideB = kC1 + 1;   // odd strides: a lane per row writes without bank conflicts
constexpr int kMfmaPartial = 1024, kBlockPartial = kMfmaPartial + 64;
enum { W_C1, B_C1, W_C2, B_C2, W_C3, B_C3, W_T0, B_T0, W_T1, B_T1, W_T2, B_T2, W_EX, B_EX, W_CO, B_CO };

typedef const float __attribute__((address_space(4))) cfloat;   // constant address space: uniform addresses load through the scalar cache
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ const cfloat* scalar_ptr(const float* p) { return reinterpret_cast<const cfloat*>(reinterpret_cast<uintptr_t>(p)); }
// The same pointer, opaque to the optimiser: loads through it stay where they are written.  Inside a loop over units this keeps the
// compiler from hoisting a layer's weights out of the loop, where they would not fit the scalar registers and would be parked in (and
// fetched back from) vector-register lanes one v_readlane at a time; rereading them from the scalar cache per unit is the cheap way.
__device__ __forceinline__ const cfloat* scalar_ptr_here(const float* p) {
    const cfloat* q = scalar_ptr(p);
    asm volatile("" : "+s"(q));
    return q;
}

struct Weights {
    const float* p[16];
};
struct Grads {
    float* p[16];
};
struct Geom {
    int h, w, dsh, dsw, nch;   // nch: units (64-pixel chunks) per downsampled row
    uint32_t units;
};

__host__ __device__ __forceinline__ int cell_lo(int g, int ds) { return g * ds / kGrid; }
__host__ __device__ __forceinline__ int cell_hi(int g, int ds) { return ((g + 1) * ds + kGrid - 1) / kGrid; }

Geom make_geom(int h, int w) {
    Geom g;
    g.h = h, g.w = w, g.dsh = h / 3, g.dsw = w / 3;
    g.nch = (g.dsw + GRUT_WAVE - 1) / GRUT_WAVE;
    g.units = (uint32_t)g.dsh * (uint32_t)g.nch;
    return g;
}
bool good_shape(int h, int w) { return h >= 3 && w >= 3 && h <= kMaxDim && w <= kMaxDim; }
uint32_t bwd_blocks(const Geom& g) {
    const uint32_t need = (g.units + kWaves - 1) / kWaves;
    return need < kMaxBwdBlocks ? need : kMaxBwdBlocks;
}

// scratch layouts (floats)
struct FwdScratch {
    size_t pool, part0, total;   // P[64][units][5]; part0[64][128]
};
FwdScratch fwd_scratch(const Geom& g) {
    FwdScratch s;
    s.pool = 0;
    s.part0 = (size_t)kC3 * g.units * kGrid;
    s.total = s.part0 + (size_t)kC3 * kHid;
    return s;
}
struct BwdScratch {
    size_t dz0, dfs, d2, pool, partials, total;   // dz0[128]; dFs[1600]; D2[25][32]; Q[32][units][5]; per-block partials
};
BwdScratch bwd_scratch(const Geom& g) {
    BwdScratch s;
    s.dz0 = 0;
    s.dfs = s.dz0 + kHid;
    s.d2 = s.dfs + kFeat;
    s.pool = s.d2 + kCells * kC2;
    s.partials = s.pool + (size_t)kC2 * g.units * kGrid;
    s.total = s.partials + (size_t)bwd_blocks(g) * kBlockPartial;
    return s;
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// conv1 on the 3x3 window, max (and the first arg-max's place in the window, row-major), ReLU, conv2.  (dy, dx) must be inside the
// downsampled grid.
template <bool ARG>
__device__ __forceinline__ void cnn_front(const Geom& g, const float* __restrict__ hdr, const Weights& wt, int dy, int dx, float (&m)[kC1],
                                          int (&arg)[kC1], float (&z2)[kC2]) {
    const cfloat* w1 = scalar_ptr_here(wt.p[W_C1]);
    const cfloat* b1 = scalar_ptr_here(wt.p[B_C1]);
    const cfloat* w2 = scalar_ptr_here(wt.p[W_C2]);
    const cfloat* b2 = scalar_ptr_here(wt.p[B_C2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float* row = hdr + ((size_t)(3 * dy + r) * g.w + 3 * (size_t)dx) * 3;
        float x[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) x[j] = row[j];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
            for (int k = 0; k < kC1; ++k) {
                const float v = fmaf(w1[3 * k + 2], x[3 * q + 2], fmaf(w1[3 * k + 1], x[3 * q + 1], fmaf(w1[3 * k], x[3 * q], b1[k])));
                if (r == 0 && q == 0) {
                    m[k] = v;
                    if (ARG) arg[k] = 0;
                } else {
                    const bool better = v > m[k];   // strict: a tie stays with the first maximum in row-major order
                    m[k] = better ? v : m[k];
                    if (ARG) {
                        arg[k] = better ? 3 * r + q : arg[k];
                        asm volatile("" : "+v"(arg[k]));   // selected now: the compiler otherwise keeps all 128 comparison masks for later
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kC2; ++i) {
        float v = b2[i];
#pragma unroll
        for (int k = 0; k < kC1; ++k) v = fmaf(w2[kC1 * i + k], fmaxf(m[k], 0.f), v);
        z2[i] = v;
    }
}

// the wave's sums of N channels over the lanes of each column cell the unit touches -> dst[channel][unit][gx]
template <int N>
__device__ __forceinline__ void pool_unit(const Geom& g, const float (&v)[N], bool valid, int dx, int x0, uint32_t u, int lane, float* __restrict__ dst) {
    const int x1 = min(x0 + GRUT_WAVE, g.dsw);
#pragma unroll
    for (int gx = 0; gx < kGrid; ++gx) {
        const int lo = cell_lo(gx, g.dsw), hi = cell_hi(gx, g.dsw);
        if (x0 >= hi || x1 <= lo) continue;   // wave-uniform
        const bool in = valid && dx >= lo && dx < hi;
#pragma unroll
        for (int q = 0; q < N / 16; ++q) {
            float part[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) part[j] = in ? v[16 * q + j] : 0.f;
            const float t = wave_reduce_scatter16(part, lane);
            if (lane < 16) dst[((size_t)(16 * q + lane) * g.units + u) * kGrid + gx] = t;
        }
    }
}

__global__ __launch_bounds__(kBlock) void cnn_forward_kernel(Geom g, const float* __restrict__ hdr, Weights wt, float* __restrict__ pool) {
    const int lane = lane_id();
    const uint32_t u = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + threadIdx.x / GRUT_WAVE);
    if (u >= g.units) return;
    const int dy = (int)(u / (uint32_t)g.nch), x0 = (int)(u % (uint32_t)g.nch) * GRUT_WAVE;
    const bool valid = x0 + lane < g.dsw;
    const int dx = valid ? x0 + lane : x0;   // a lane past the row's end recomputes the unit's first pixel and is left out of every sum
    float m[kC1], z2[kC2], y[kC3];
    int arg[kC1];
    cnn_front<false>(g, hdr, wt, dy, dx, m, arg, z2);
    const cfloat* w3 = scalar_ptr(wt.p[W_C3]);
    const cfloat* b3 = scalar_ptr(wt.p[B_C3]);
#pragma unroll
    for (int c = 0; c < kC3; ++c) {
        float v = b3[c];
#pragma unroll
        for (int i = 0; i < kC2; ++i) v = fmaf(w3[kC2 * c + i], fmaxf(z2[i], 0.f), v);
        y[c] = v;
    }
    pool_unit<kC3>(g, y, valid, dx, x0, u, lane, pool);
}

// Sum of one cell's terms of one channel of a pooled array laid out [channel][unit][gx]: rows of the cell outermost, then the column chunks
// that reach into the cell.  Lane j of the cell's 8 takes terms j, j + 8, ...; `red` (LDS, [32][8]) adds the eight in order.
__device__ __forceinline__ float cell_sum(const Geom& g, const float* __restrict__ chan, int cell, int j, float (*red)[8]) {
    float s = 0.f;
    if (cell < kCells) {
        const int gy = cell / kGrid, gx = cell % kGrid;
        const int h0 = cell_lo(gy, g.dsh), h1 = cell_hi(gy, g.dsh), lo = cell_lo(gx, g.dsw), hi = cell_hi(gx, g.dsw);
        const int c0 = lo / GRUT_WAVE, nc = (hi - 1) / GRUT_WAVE - c0 + 1;
        const int terms = (h1 - h0) * nc;
#pragma unroll 4
        for (int n = j; n < terms; n += 8) {
            const int dy = h0 + n / nc, cb = c0 + n % nc;
            s += chan[((size_t)dy * g.nch + cb) * kGrid + gx];
        }
    }
    red[threadIdx.x >> 3][j] = s;
    __syncthreads();
    float t = 0.f;
    if (cell < kCells && j == 0) {
        t = red[cell][0];
#pragma unroll
        for (int k = 1; k < 8; ++k) t += red[cell][k];
    }
    return t;   // lane j == 0 of the cell
}
__device__ __forceinline__ int cell_count(const Geom& g, int cell) {
    const int gy = cell / kGrid, gx = cell % kGrid;
    return (cell_hi(gy, g.dsh) - cell_lo(gy, g.dsh)) * (cell_hi(gx, g.dsw) - cell_lo(gx, g.dsw));
}

// block c: channel c's 25 features, then their share of trunk0's 128 pre-activations
__global__ __launch_bounds__(kBlock) void pool_trunk0_kernel(Geom g, const float* __restrict__ pool, Weights wt, float* __restrict__ part0,
                                                             float* __restrict__ saved) {
    __shared__ float red[kBlock / 8][8];
    __shared__ float feat[kCells];
    const int t = threadIdx.x, c = blockIdx.x, cell = t >> 3, j = t & 7;
    const float s = cell_sum(g, pool + (size_t)c * g.units * kGrid, cell, j, red);
    if (cell < kCells && j == 0) {
        const float f = s / (float)cell_count(g, cell);
        feat[cell] = f;
        if (saved) saved[c * kCells + cell] = f;
    }
    __syncthreads();
    if (t < kHid) {
        const float* row = wt.p[W_T0] + (size_t)t * kIn + c * kCells;
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < kCells; ++k) v = fmaf(row[k], feat[k], v);
        part0[c * kHid + t] = v;
    }
}

// out[o] = act(b[o] + W[o][:] . in) for `rows` rows of 128 inputs (b, in, out in LDS): a wave per row, rows dealt to the block's waves in turn
template <bool RELU>
__device__ __forceinline__ void dense128(const float* __restrict__ W, const float* b, const float* in, float* out, int rows) {
    const int lane = lane_id(), wave = threadIdx.x / GRUT_WAVE;
    const float i0 = in[lane], i1 = in[lane + GRUT_WAVE];
    constexpr int kBatch = 8;   // rows whose loads are in flight together: the layer costs rows / (4 kBatch) memory latencies, not rows / 4
    for (int base = wave; base < rows; base += kWaves * kBatch) {
        float w0[kBatch], w1[kBatch];
#pragma unroll
        for (int r = 0; r < kBatch; ++r) {
            const int o = min(base + r * kWaves, rows - 1);   // a row past the end rereads the last one and is dropped below
            w0[r] = W[(size_t)o * kHid + lane];
            w1[r] = W[(size_t)o * kHid + lane + GRUT_WAVE];
        }
#pragma unroll
        for (int r = 0; r < kBatch; ++r) {
            const int o = base + r * kWaves;
            const float s = wave_sum(fmaf(w1[r], i1, w0[r] * i0));
            if (lane == 0 && o < rows) out[o] = RELU ? fmaxf(s + b[o], 0.f) : s + b[o];
        }
    }
}

__global__ __launch_bounds__(kBlock) void trunk_kernel(const float* __restrict__ part0, const float* __restrict__ prior, Weights wt,
                                                       float* __restrict__ saved, float* __restrict__ out) {
    __shared__ float act[3][kHid];
    __shared__ float bias[2][kHid];
    __shared__ float head[9], head_bias[9];
    const int t = threadIdx.x;
    if (t >= kHid) {   // the later layers' biases come in while the first layer is summed
        bias[0][t - kHid] = wt.p[B_T1][t - kHid];
        bias[1][t - kHid] = wt.p[B_T2][t - kHid];
    }
    if (t < 9) head_bias[t] = t == 0 ? wt.p[B_EX][0] : wt.p[B_CO][t - 1];
    if (t < kHid) {
        float z = wt.p[B_T0][t];
#pragma unroll 16
        for (int c = 0; c < kC3; ++c) z += part0[c * kHid + t];
        z = fmaf(prior ? prior[0] : 0.f, wt.p[W_T0][(size_t)t * kIn + kFeat], z);
        act[0][t] = fmaxf(z, 0.f);
    }
    __syncthreads();
    dense128<true>(wt.p[W_T1], bias[0], act[0], act[1], kHid);
    __syncthreads();
    dense128<true>(wt.p[W_T2], bias[1], act[1], act[2], kHid);
    __syncthreads();
    dense128<false>(wt.p[W_EX], head_bias, act[2], head, 1);
    dense128<false>(wt.p[W_CO], head_bias + 1, act[2], head + 1, 8);
    __syncthreads();
    if (t < 9) out[t] = head[t];
    if (saved)
        for (int i = t; i < 3 * kHid; i += kBlock) saved[kFeat + i] = act[i / kHid][i % kHid];
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------
// dIn[i] = sum_o W[o][i] dz[o] (thread halves take 64 rows each, added in order), and dW = dz x in written whole
__device__ __forceinline__ float dense128_backward(const float* __restrict__ W, const float* dz, const float* in, float* __restrict__ gW,
                                                   float (*tmp)[kHid]) {
    const int t = threadIdx.x, i = t & (kHid - 1), half = t >> 7;
    float s = 0.f;
    for (int o = half * 64; o < half * 64 + 64; ++o) s = fmaf(W[o * kHid + i], dz[o], s);
    tmp[half][i] = s;
    for (int e = t; e < kHid * kHid; e += kBlock) gW[e] = dz[e >> 7] * in[e & (kHid - 1)];
    __syncthreads();
    return tmp[0][i] + tmp[1][i];
}

__global__ __launch_bounds__(kBlock) void trunk_backward_kernel(const float* __restrict__ saved, const float* __restrict__ grad_out, Weights wt,
                                                                Grads gr, float* __restrict__ dz0_out) {
    __shared__ float act[3][kHid], dz[2][kHid], tmp[2][kHid], go[9];
    const int t = threadIdx.x;
    for (int i = t; i < 3 * kHid; i += kBlock) act[i / kHid][i % kHid] = saved[kFeat + i];
    if (t < 9) go[t] = grad_out[t];
    __syncthreads();
    if (t < kHid) {
        float d = go[0] * wt.p[W_EX][t];
#pragma unroll
        for (int k = 0; k < 8; ++k) d = fmaf(go[1 + k], wt.p[W_CO][k * kHid + t], d);
        d = act[2][t] > 0.f ? d : 0.f;
        dz[0][t] = d;
        gr.p[B_T2][t] = d;
        gr.p[W_EX][t] = go[0] * act[2][t];
#pragma unroll
        for (int k = 0; k < 8; ++k) gr.p[W_CO][k * kHid + t] = go[1 + k] * act[2][t];
        if (t == 0) gr.p[B_EX][0] = go[0];
        if (t < 8) gr.p[B_CO][t] = go[1 + t];
    }
    __syncthreads();
    float d = dense128_backward(wt.p[W_T2], dz[0], act[1], gr.p[W_T2], tmp);
    if (t < kHid) {
        d = act[1][t] > 0.f ? d : 0.f;
        dz[1][t] = d;
        gr.p[B_T1][t] = d;
    }
    __syncthreads();
    d = dense128_backward(wt.p[W_T1], dz[1], act[0], gr.p[W_T1], tmp);
    if (t < kHid) {
        d = act[0][t] > 0.f ? d : 0.f;
        gr.p[B_T0][t] = d;
        dz0_out[t] = d;
    }
}

// block b: columns 32 b .. 32 b + 31 of trunk0.  Thread (column, group of 16 rows).
__global__ __launch_bounds__(kBlock) void trunk0_backward_kernel(Geom g, const float* __restrict__ saved, const float* __restrict__ prior,
                                                                 const float* __restrict__ dz0, Weights wt, Grads gr, float* __restrict__ dfs) {
    __shared__ float red[8][kT0Cols];
    __shared__ float dz[kHid];
    const int t = threadIdx.x, col = blockIdx.x * kT0Cols + (t & (kT0Cols - 1)), grp = t / kT0Cols;
    if (t < kHid) dz[t] = dz0[t];
    __syncthreads();
    float s = 0.f;
    if (col < kIn) {
        const float x = col < kFeat ? saved[col] : (prior ? prior[0] : 0.f);
        for (int o = grp * 16; o < grp * 16 + 16; ++o) {
            s = fmaf(wt.p[W_T0][(size_t)o * kIn + col], dz[o], s);
            gr.p[W_T0][(size_t)o * kIn + col] = dz[o] * x;
        }
    }
    red[grp][t & (kT0Cols - 1)] = s;
    __syncthreads();
    if (grp == 0 && col < kFeat) {
        float d = red[0][t];
#pragma unroll
        for (int k = 1; k < 8; ++k) d += red[k][t];
        dfs[col] = d / (float)cell_count(g, col % kCells);
    }
}

// D2[cell][i] = sum_c W3[c][i] dFs[c][cell]: block per cell
__global__ __launch_bounds__(GRUT_WAVE) void d2_kernel(const float* __restrict__ dfs, Weights wt, float* __restrict__ d2) {
    const int cell = blockIdx.x, i = threadIdx.x;
    if (i >= kC2) return;
    float s = 0.f;
    for (int c = 0; c < kC3; ++c) s = fmaf(wt.p[W_C3][c * kC2 + i], dfs[c * kCells + cell], s);
    d2[cell * kC2 + i] = s;
}

__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void cnn_backward_kernel(Geom g, const float* __restrict__ hdr, Weights wt, const float* __restrict__ d2,
                                                              float* __restrict__ pool, float* __restrict__ partials) {
    __shared__ float s_d2[kCells * kC2];
    __shared__ float s_g[kWaves][kGrid][kC2];
    __shared__ float s_a[kWaves][GRUT_WAVE * kStrideA];
    __shared__ float s_b[kWaves][GRUT_WAVE * kStrideB];
    const int lane = lane_id(), wave = threadIdx.x / GRUT_WAVE;
    for (int i = threadIdx.x; i < kCells * kC2; i += kBlock) s_d2[i] = d2[i];
    __syncthreads();

    f32x16 acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
    float acc1[64];   // [k][r, g, b, 1]
#pragma unroll
    for (int i = 0; i < 64; ++i) acc1[i] = 0.f;
    float* sa = s_a[wave];
    float* sb = s_b[wave];

    const uint32_t first = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wave), step = gridDim.x * kWaves;
    for (uint32_t u = first; u < g.units; u += step) {
        const int dy = (int)(u / (uint32_t)g.nch), x0 = (int)(u % (uint32_t)g.nch) * GRUT_WAVE;
        const int x1 = min(x0 + GRUT_WAVE, g.dsw);
        const bool valid = x0 + lane < g.dsw;
        const int dx = valid ? x0 + lane : x0;
        float m[kC1], z2[kC2];
        int arg[kC1];
        cnn_front<true>(g, hdr, wt, dy, dx, m, arg, z2);
        {   // S's partial: the ReLU'd conv2 output pooled like the forward's features
            float h2[kC2];
#pragma unroll
            for (int i = 0; i < kC2; ++i) h2[i] = fmaxf(z2[i], 0.f);
            pool_unit<kC2>(g, h2, valid, dx, x0, u, lane, pool);
        }
        wave_lds_sync();   // the previous unit's reads of s_g, s_a, s_b are done
        // the row's share of D2 per column cell: lane (i, half) takes gx = half, half + 2, half + 4
        for (int gx = lane >> 5; gx < kGrid; gx += 2) {
            float s = 0.f;
#pragma unroll
            for (int gy = 0; gy < kGrid; ++gy)
                if (dy >= cell_lo(gy, g.dsh) && dy < cell_hi(gy, g.dsh)) s += s_d2[(gy * kGrid + gx) * kC2 + (lane & 31)];
            s_g[wave][gx][lane & 31] = s;
        }
        wave_lds_sync();
        float dz2[kC2];
#pragma unroll
        for (int i = 0; i < kC2; ++i) dz2[i] = 0.f;
#pragma unroll
        for (int gx = 0; gx < kGrid; ++gx) {
            const int lo = cell_lo(gx, g.dsw), hi = cell_hi(gx, g.dsw);
            if (x0 >= hi || x1 <= lo) continue;   // wave-uniform
            const bool in = valid && dx >= lo && dx < hi;
#pragma unroll
            for (int i = 0; i < kC2; ++i) dz2[i] += in ? s_g[wave][gx][i] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kC2; ++i) {
            dz2[i] = z2[i] > 0.f ? dz2[i] : 0.f;
            sa[lane * kStrideA + i] = dz2[i];
        }
#pragma unroll
        for (int k = 0; k < kC1; ++k) sb[lane * kStrideB + k] = fmaxf(m[k], 0.f);
        // conv2's transpose and the max-pool's routing; then the window is read again (it is in the cache) and every pixel takes the
        // gradient of the channels whose first maximum it was
        const cfloat* w2 = scalar_ptr_here(wt.p[W_C2]);
        float dz1[kC1];
#pragma unroll
        for (int k = 0; k < kC1; ++k) dz1[k] = 0.f;
#pragma unroll
        for (int i = 0; i < kC2; ++i) {   // rows of W2 in the order they are stored
            if (i % 4 == 0) {   // four rows (64 scalar registers of weights) at a time: the next four are fetched after these are used up
                w2 = scalar_ptr_here(wt.p[W_C2]);
                asm volatile("" : "+v"(dz1[0]), "+v"(dz1[1]), "+v"(dz1[2]), "+v"(dz1[3]), "+v"(dz1[4]), "+v"(dz1[5]), "+v"(dz1[6]), "+v"(dz1[7]),
                             "+v"(dz1[8]), "+v"(dz1[9]), "+v"(dz1[10]), "+v"(dz1[11]), "+v"(dz1[12]), "+v"(dz1[13]), "+v"(dz1[14]), "+v"(dz1[15]));
            }
#pragma unroll
            for (int k = 0; k < kC1; ++k) dz1[k] = fmaf(w2[kC1 * i + k], dz2[i], dz1[k]);
        }
#pragma unroll
        for (int k = 0; k < kC1; ++k) {
            dz1[k] = m[k] > 0.f ? dz1[k] : 0.f;
            acc1[4 * k + 3] += dz1[k];
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float* row = hdr + ((size_t)(3 * dy + r) * g.w + 3 * (size_t)dx) * 3;
            float x[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) x[j] = row[j];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
#pragma unroll
                for (int k = 0; k < kC1; ++k) {
                    const float d = arg[k] == 3 * r + q ? dz1[k] : 0.f;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) acc1[4 * k + ch] = fmaf(d, x[3 * q + ch], acc1[4 * k + ch]);
                }
            }
        }
        wave_lds_sync();
        // D[i][n] += sum over the unit's pixels of dZ2[i] * (h1[n] for n < 16, 1 for n == 16): two pixels per MFMA step
        const int n = lane & 31, kk = lane >> 5;
#pragma unroll 4
        for (int s = 0; s < GRUT_WAVE / 2; ++s) {
            const int p = 2 * s + kk;
            const float a = sa[p * kStrideA + n];
            const float b = n < kC1 ? sb[p * kStrideB + n] : (n == kC1 ? 1.f : 0.f);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc2, 0, 0, 0);
        }
    }

    // block partial: the waves' accumulators added in wave order
    __syncthreads();
    float* red = &s_a[0][0];   // kWaves * 1088 floats fit: 4 * 64 * 33 = 8448
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave * kBlockPartial + r * GRUT_WAVE + lane] = acc2[r];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float part[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) part[j] = acc1[16 * q + j];
        const float t = wave_reduce_scatter16(part, lane);
        if (lane < 16) red[wave * kBlockPartial + kMfmaPartial + 16 * q + lane] = t;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kBlockPartial; e += kBlock) {
        float t = red[e];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) t += red[w * kBlockPartial + e];
        partials[(size_t)blockIdx.x * kBlockPartial + e] = t;
    }
}

// blocks 0..31: S for conv2 channel i, then column i of dW3 (block 0: db3 too); blocks 32..65: 32 elements each of the per-block partials
__global__ __launch_bounds__(kBlock) void finish_kernel(Geom g, uint32_t blocks, const float* __restrict__ dfs, const float* __restrict__ pool,
                                                        const float* __restrict__ partials, Grads gr) {
    __shared__ float red[kBlock / 8][8];
    __shared__ float S[kCells];
    const int t = threadIdx.x, slot = t >> 3, j = t & 7;
    if (blockIdx.x < kC2) {
        const int i = blockIdx.x;
        const float s = cell_sum(g, pool + (size_t)i * g.units * kGrid, slot, j, red);
        if (slot < kCells && j == 0) S[slot] = s;
        __syncthreads();
        if (t < kC3) {
            float v = 0.f;
#pragma unroll
            for (int cell = 0; cell < kCells; ++cell) v = fmaf(dfs[t * kCells + cell], S[cell], v);
            gr.p[W_C3][t * kC2 + i] = v;
        } else if (i == 0 && t < 2 * kC3) {
            const int c = t - kC3;
            float v = 0.f;
            for (int cell = 0; cell < kCells; ++cell) v = fmaf(dfs[c * kCells + cell], (float)cell_count(g, cell), v);
            gr.p[B_C3][c] = v;
        }
        return;
    }
    // lanes along the element (adjacent lanes read adjacent floats), eight groups of lanes over the blocks in turn
    const int el = t & 31, grp = t >> 5, e = (blockIdx.x - kC2) * 32 + el;   // < 34 * 32 = 1088
    float s = 0.f;
#pragma unroll 8
    for (uint32_t b = grp; b < blocks; b += 8) s += partials[(size_t)b * kBlockPartial + e];
    red[el][grp] = s;
    __syncthreads();
    if (grp != 0) return;
    float v = red[el][0];
#pragma unroll
    for (int k = 1; k < 8; ++k) v += red[el][k];
    if (e < kMfmaPartial) {   // the MFMA's C/D map: register r of lane l is D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31]
        const int r = e >> 6, l = e & 63, i = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), n = l & 31;
        if (n < kC1) gr.p[W_C2][i * kC1 + n] = v;
        else if (n == kC1) gr.p[B_C2][i] = v;
    } else {
        const int idx = e - kMfmaPartial, k = idx >> 2, ch = idx & 3;
        if (ch < 3) gr.p[W_C1][k * 3 + ch] = v;
        else gr.p[B_C1][k] = v;
    }
}

int check_common(const char* fn, int h, int w, const float* hdr, const float* const* weights, const float* scratch) {
    GRUT_REQUIRE(h >= 3 && w >= 3, "%s: h and w must be at least 3 (got %d x %d)", fn, h, w);
    GRUT_REQUIRE(h <= kMaxDim && w <= kMaxDim, "%s: h and w must be at most %d (got %d x %d)", fn, kMaxDim, h, w);
    GRUT_REQUIRE(hdr, "%s: hdr is NULL", fn);
    GRUT_REQUIRE(weights, "%s: weights is NULL", fn);
    for (int i = 0; i < 16; ++i) GRUT_REQUIRE(weights[i], "%s: weights[%d] is NULL", fn, i);
    GRUT_REQUIRE(scratch, "%s: scratch is NULL", fn);
    return GRUT_OK;
}

}  // namespace
}  // namespace grut

using namespace grut;

extern "C" uint64_t grut_ppisp_controller_forward_scratch(int h, int w) { return good_shape(h, w) ? fwd_scratch(make_geom(h, w)).total : 0; }
extern "C" uint64_t grut_ppisp_controller_backward_scratch(int h, int w) { return good_shape(h, w) ? bwd_scratch(make_geom(h, w)).total : 0; }

extern "C" int grut_ppisp_controller_forward(void* stream, int h, int w, const float* hdr, const float* prior, const float* const* weights,
                                             float* scratch, float* saved, float* out) {
    GRUT_CHECK(check_common("grut_ppisp_controller_forward", h, w, hdr, weights, scratch));
    GRUT_REQUIRE(out, "grut_ppisp_controller_forward: out is NULL");
    const Geom g = make_geom(h, w);
    const FwdScratch fs = fwd_scratch(g);
    Weights wt;
    for (int i = 0; i < 16; ++i) wt.p[i] = weights[i];
    const hipStream_t s = (hipStream_t)stream;
    cnn_forward_kernel<<<(g.units + kWaves - 1) / kWaves, kBlock, 0, s>>>(g, hdr, wt, scratch + fs.pool);
    GRUT_HIP(hipGetLastError());
    pool_trunk0_kernel<<<kC3, kBlock, 0, s>>>(g, scratch + fs.pool, wt, scratch + fs.part0, saved);
    GRUT_HIP(hipGetLastError());
    trunk_kernel<<<1, kBlock, 0, s>>>(scratch + fs.part0, prior, wt, saved, out);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

extern "C" int grut_ppisp_controller_backward(void* stream, int h, int w, const float* hdr, const float* prior, const float* const* weights,
                                              const float* saved, const float* grad_out, float* scratch, float* const* grads) {
    GRUT_CHECK(check_common("grut_ppisp_controller_backward", h, w, hdr, weights, scratch));
    GRUT_REQUIRE(saved, "grut_ppisp_controller_backward: saved is NULL");
    GRUT_REQUIRE(grad_out, "grut_ppisp_controller_backward: grad_out is NULL");
    GRUT_REQUIRE(grads, "grut_ppisp_controller_backward: grads is NULL");
    for (int i = 0; i < 16; ++i) GRUT_REQUIRE(grads[i], "grut_ppisp_controller_backward: grads[%d] is NULL", i);
    const Geom g = make_geom(h, w);
    const BwdScratch bs = bwd_scratch(g);
    const uint32_t blocks = bwd_blocks(g);
    Weights wt;
    Grads gr;
    for (int i = 0; i < 16; ++i) wt.p[i] = weights[i], gr.p[i] = grads[i];
    const hipStream_t s = (hipStream_t)stream;
    trunk_backward_kernel<<<1, kBlock, 0, s>>>(saved, grad_out, wt, gr, scratch + bs.dz0);
    GRUT_HIP(hipGetLastError());
    trunk0_backward_kernel<<<kT0Blocks, kBlock, 0, s>>>(g, saved, prior, scratch + bs.dz0, wt, gr, scratch + bs.dfs);
    GRUT_HIP(hipGetLastError());
    d2_kernel<<<kCells, GRUT_WAVE, 0, s>>>(scratch + bs.dfs, wt, scratch + bs.d2);
    GRUT_HIP(hipGetLastError());
    cnn_backward_kernel<<<blocks, kBlock, 0, s>>>(g, hdr, wt, scratch + bs.d2, scratch + bs.pool, scratch + bs.partials);
    GRUT_HIP(hipGetLastError());
    finish_kernel<<<kC2 + kBlockPartial / (kBlock / 8), kBlock, 0, s>>>(g, blocks, scratch + bs.dfs, scratch + bs.pool, scratch + bs.partials, gr);
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}
