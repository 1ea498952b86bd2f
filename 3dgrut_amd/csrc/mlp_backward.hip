// mlp_backward.hip — the backward of the NHT decoder's network (mlp.hip) as ONE fused HIP kernel plus a small ordered reduction.
// The contract: grut_mlp_backward in include/grut_amd.h.  Every index rule: mlp_layout.hpp ("the backward"), shared with the host emulation
// of tests/test_mlp_backward_cpu.py.  The same kernel with another input source and gradient sink is the backward of the NHT decode stage
// (grut_decode_backward): grad_features and grad_alpha instead of the gradient of assembled rows.
//
// Structure.  Persistent grid, one workgroup of four waves per CU; the workgroup builds the forward's bf16 weight image in LDS from the live
// fp32 `params` and then takes 128 pixels per step, wave w the 32 pixels 32 w .. 32 w + 31.  Per step a wave
//   1. recomputes the forward with the forward's rounding points, keeping every hidden layer's packed bf16 activation in registers
//      (the layer count is a template parameter, so the per-layer register arrays are indexed at compile time);
//   2. forms dZ of the output layer in fp32 (activation derivative from the recomputed output), rounds it ONCE to bf16, and walks the
//      layers down: dH = W^T dZ takes dZ's packed C / D registers as the B operand with no lane movement, and W^T fragments straight out
//      of the forward's image through ds_read_b64_tr_b16; the ReLU gate is read off the packed activation in the same register position;
//   3. for the weight gradient dW = dZ H^T, whose sum runs over the pixel (the lane of both operands), stores the very same packed dZ and
//      H fragments into two [pixel][neuron] LDS tiles of the workgroup, and multiplies the 32 x 32 tiles of dW that it owns from
//      transposed reads of both; those accumulators live in registers across ALL steps of the workgroup;
//   4. writes grad_input: feature columns from the C / D registers, the three direction columns through the SH Jacobian in fp32.
// At the end every workgroup writes its partial dW to its slice of the scratch, and mlp_backward_reduce_kernel sums the slices in workgroup
// order.  No atomics anywhere: the result depends on (configuration, P, grid) only.
// EXEC is all ones around every MFMA and every transposed read: tail pixels clamp their loads, get dZ = 0 and store nothing; the only
// branches around them are workgroup- or wave-uniform.
#include "common.hpp"
#include "mlp_layout.hpp"

namespace grut {
namespace {

#include "mlp_device.inl"

constexpr int kBlock = kBwdWaves * GRUT_WAVE;
constexpr int kKSteps = kBwdPixels / kStep;    // pixel k-steps of a weight-gradient tile per workgroup step
constexpr int kKB0Max = kMaxK0 / kTile;         // k blocks of the first layer at most
constexpr int kExPitch = 33, kShPitch = 17;      // floats per pixel of the two exchanges of grad_input (32 + 1, 16 + 1: no bank conflicts)
static_assert((kBwdPixels * (kExPitch + kShPitch)) * 4 <= 2 * kBwdPixels * 2 * kTile * 2, "the exchanges fit into the smallest pair of tiles");

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// two ds_read_b64_tr_b16 -> one 8-element fragment: elements 0..3 from `lo`, 4..7 from `hi`
__device__ __forceinline__ bf16x8 read_tr_frag(const unsigned char* lo, const unsigned char* hi) {
    const uint2 a = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)lo));
    const uint2 b = __builtin_bit_cast(uint2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)hi));
    return as_frag(make_uint4(a.x, a.y, b.x, b.y));
}

// The addresses of the transposed reads split into a per-lane base and a wave-uniform rest (the host emulation checks the identities):
//   layers >= 1   bwd_wt_read_offset(s, l, kb, tp, c, lane) = bwd_wt_read_offset(s, 1, 0, 0, 0, lane) - the same at lane 0
//                                                             + bwd_wt_read_offset(s, l, kb, tp, c, 0)
//   layer 0       (its last k block may clamp a k-step, per lane)  the same with (0, kb, 0, 0) in the two lane terms
//   bwd_stage_read_offset(blk, kk, c, lane) = bwd_stage_read_offset(0, 0, c, lane) + bwd_stage_read_offset(blk, kk, 0, 0)
// lane_part is the difference of the two lane terms.
__device__ __forceinline__ bf16x8 wt_frag(const unsigned char* image, const Shape& s, int layer, int kb, int tp, uint32_t lane_part) {
    return read_tr_frag(image + lane_part + bwd_wt_read_offset(s, layer, kb, tp, 0, 0), image + lane_part + bwd_wt_read_offset(s, layer, kb, tp, 1, 0));
}
__device__ __forceinline__ bf16x8 stage_frag(const unsigned char* tile, int blk, int kk, const uint32_t (&lane_base)[2]) {
    const uint32_t rest = bwd_stage_read_offset(blk, kk, 0, 0);
    return read_tr_frag(tile + lane_base[0] + rest, tile + lane_base[1] + rest);
}

// the lane's 16 bytes of the packed fragment of k-step t -> its pixel row of a staged tile.  lane_base[t & 1][c] is
// bwd_stage_store_offset(pixel, t & 1, c, h); the rest, 8192 (t >> 1), is uniform
__device__ __forceinline__ void stage_store(unsigned char* tile, int t, const uint32_t (&lane_base)[2][2], bf16x8 frag) {
    const uint4 v = __builtin_bit_cast(uint4, frag);
    const uint32_t rest = bwd_stage_store_offset(0, t & ~1, 0, 0);
    *reinterpret_cast<uint2*>(tile + lane_base[t & 1][0] + rest) = make_uint2(v.x, v.y);
    *reinterpret_cast<uint2*>(tile + lane_base[t & 1][1] + rest) = make_uint2(v.z, v.w);
}

// dH (fp32, C / D layout) -> dZ of the layer below: the gate is the packed activation in the same register position (non-zero after
// its ReLU), the result is rounded once to bf16 and is the next product's B operand as it stands
template <int MB>
__device__ __forceinline__ void gate_pack(const f32x16 (&acc)[MB], const bf16x8 (&hb)[2 * MB], bf16x8 (&dz)[2 * MB]) {
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const uint4 hv = __builtin_bit_cast(uint4, hb[2 * b + sub]);
            const uint32_t hw[4] = {hv.x, hv.y, hv.z, hv.w};
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                w[q] = pack_bf16((hw[q] & 0x00007fffu) ? acc[b][8 * sub + 2 * q] : 0.f, (hw[q] & 0x7fff0000u) ? acc[b][8 * sub + 2 * q + 1] : 0.f);
            dz[2 * b + sub] = as_frag(make_uint4(w[0], w[1], w[2], w[3]));
        }
}

// one 32 x 32 tile of a layer's dW += dZ tile (row block m) x H tile (k block kb)^T over the workgroup's 128 pixels.  m and kb may be
// run-time (wave-uniform) values: they go into the tiles' base, so that the k-step's part stays an immediate offset
__device__ __forceinline__ f32x16 dw_tile(const unsigned char* stage_dz, const unsigned char* stage_h, int m, int kb,
                                          const uint32_t (&rd)[2], f32x16 acc) {
    const unsigned char* a = stage_dz + bwd_stage_read_offset(m, 0, 0, 0);
    const unsigned char* b = stage_h + bwd_stage_read_offset(kb, 0, 0, 0);
#pragma unroll
    for (int kk = 0; kk < kKSteps; ++kk)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(stage_frag(a, 0, kk, rd), stage_frag(b, 0, kk, rd), acc, 0, 0, 0);
    return acc;
}

// a wave's tile of a partial dW -> the workgroup's slice: rows [32 m ..) x columns [32 kb ..) of the [rows][cols] matrix at dst
__device__ __forceinline__ void store_tile(float* __restrict__ dst, int rows, int cols, int m, int kb, int r, int h, const f32x16& acc) {
    const int k = kTile * kb + r;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = kTile * m + mlp_out_row(reg, h);
        if (row < rows && k < cols) dst[(size_t)row * cols + k] = acc[reg];
    }
}

// DECODE is the input source and the gradient sink: false, rows [P, F + 3] and grad_input [P, F + 3] through the SH
// Jacobian (grut_mlp_backward); true, the decode stage (grut_decode_backward): `input` is the feature map [P, F], the direction comes from
// decode_direction, grad_input is grad_features [P, F] (may be null) and grad_alpha [P] (may be null) takes the per-pixel sums.  `extra` is
// empty for the rows, and (DecodeArgs, grad_alpha) for the decode stage.
template <int WIDTH, int NH, int KB0, bool DECODE, class... Extra>
__global__ __launch_bounds__(kBlock) void mlp_backward_kernel(Shape shape, int n_out, int activation, const float* __restrict__ params,
                                                              const float* __restrict__ input, const float* __restrict__ grad_out, uint32_t P,
                                                              float* __restrict__ partials, float* __restrict__ grad_input, Extra... extra) {
    static_assert(sizeof...(Extra) == (DECODE ? 2 : 0), "(DecodeArgs, grad_alpha) for the decode stage, nothing for the rows");
    const DecodeArgs da = decode_args(extra...);
    float* const grad_alpha = decode_grad_alpha(extra...);
    constexpr int MB = WIDTH / kTile, KW = WIDTH / kStep;
    const Shape s{shape.n_features, shape.sh_degree, NH, WIDTH};   // the two template parameters as constants: most offsets fold
    constexpr int kSlotsH = (MB * MB + kBwdWaves - 1) / kBwdWaves, kSlots0 = (MB * KB0 + kBwdWaves - 1) / kBwdWaves;
    extern __shared__ __attribute__((aligned(16))) unsigned char image[];
    unsigned char* const stage_dz = image + image_bytes(s);
    unsigned char* const stage_h = stage_dz + bwd_stage_bytes(s);

    build_image(s, n_out, params, image, kBlock);
    __syncthreads();

    const int lane = threadIdx.x & (GRUT_WAVE - 1), r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / GRUT_WAVE));
    const int nk0 = ksteps_first(s), kb0 = bwd_kblocks(s, 0), cols = DECODE ? s.n_features : s.n_features + 3;
    const int n_sh = s.sh_degree * s.sh_degree;
    const bool need_p = partials != nullptr, need_x = grad_input != nullptr || (DECODE && grad_alpha != nullptr);
    const bool unpremultiply = DECODE && da.unpremultiply;

    // the per-lane parts of every LDS address
    uint32_t st[2][2], rd[2], wt_first[KB0];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        rd[a] = bwd_stage_read_offset(0, 0, a, lane);
#pragma unroll
        for (int c = 0; c < 2; ++c) st[a][c] = bwd_stage_store_offset(kTile * wave + r, a, c, h);
    }
    const uint32_t wt_lane = bwd_wt_read_offset(s, 1, 0, 0, 0, lane) - bwd_wt_read_offset(s, 1, 0, 0, 0, 0);   // layers >= 1
#pragma unroll
    for (int kb = 0; kb < KB0; ++kb) wt_first[kb] = bwd_wt_read_offset(s, 0, kb < kb0 ? kb : 0, 0, 0, lane) - bwd_wt_read_offset(s, 0, kb < kb0 ? kb : 0, 0, 0, 0);

    // this wave's tiles of every layer's dW, over all steps of the workgroup
    f32x16 dw_first[kSlots0], dw_hidden[NH > 1 ? NH - 1 : 1][kSlotsH], dw_out = zero16();
#pragma unroll
    for (int i = 0; i < kSlots0; ++i) dw_first[i] = zero16();
#pragma unroll
    for (int l = 0; l < (NH > 1 ? NH - 1 : 1); ++l)
#pragma unroll
        for (int i = 0; i < kSlotsH; ++i) dw_hidden[l][i] = zero16();

    const uint32_t steps = bwd_steps(P);
    for (uint32_t step = blockIdx.x; step < steps; step += gridDim.x) {
        const uint64_t pixel = (uint64_t)step * kBwdPixels + (uint64_t)(kTile * wave + r);
        const bool valid = pixel < P;
        const uint64_t src = valid ? pixel : (uint64_t)P - 1;   // a tail lane reads the last pixel, gets dZ = 0, stores nothing
        const float* row = input + src * cols;
        float dir[3], alpha = 1.f, a_s = 1.f;
        if constexpr (DECODE) {
            decode_direction(da, decode_direction_load(da, (uint32_t)src), dir);
            if (unpremultiply) alpha = da.alpha[src], a_s = fmaxf(alpha, 1e-8f);
        } else {
            dir[0] = 2.f * row[s.n_features] - 1.f, dir[1] = 2.f * row[s.n_features + 1] - 1.f, dir[2] = 2.f * row[s.n_features + 2] - 1.f;
        }
        const float dx_ = dir[0], dy_ = dir[1], dz_ = dir[2];
        const f32x16 sh = sh_values(dx_, dy_, dz_);

        // ---- 1. the forward again, with its rounding points; hb[l - 1] is the input of layer l ------------------------------------
        f32x16 acc[MB];
        bf16x8 hb[NH][KW], dz[KW];
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m] = zero16();
        const unsigned char* w = image + image_offset(s, 0, 0, 0, lane);
#pragma nounroll
        for (int t = 0; t < nk0; ++t) {
            const bf16x8 b = encode_step<DECODE>(s, t, h, row, sh, unpremultiply, a_s);
#pragma unroll
            for (int m = 0; m < MB; ++m)
                acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(*reinterpret_cast<const uint4*>(w + (size_t)frag_in_layer(nk0, m, t) * kFragBytes)),
                                                                 b, acc[m], 0, 0, 0);
        }
#pragma unroll
        for (int layer = 1; layer < NH; ++layer) {
            w = image + image_offset(s, layer, 0, 0, lane);
            pack_hidden<MB>(acc, hb[layer - 1]);
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                acc[m] = zero16();
#pragma unroll
                for (int t = 0; t < KW; ++t)
                    acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        as_frag(*reinterpret_cast<const uint4*>(w + (size_t)frag_in_layer(KW, m, t) * kFragBytes)), hb[layer - 1][t], acc[m], 0, 0, 0);
            }
        }
        pack_hidden<MB>(acc, hb[NH - 1]);
        w = image + image_offset(s, NH, 0, 0, lane);
        f32x16 o = zero16();
#pragma unroll
        for (int t = 0; t < KW; ++t)
            o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(*reinterpret_cast<const uint4*>(w + (size_t)frag_in_layer(KW, 0, t) * kFragBytes)),
                                                        hb[NH - 1][t], o, 0, 0, 0);

        // ---- 2. the output layer: dZ = grad_out x the activation's derivative, fp32, then ONE rounding to bf16 ----------------------
        float gy[8];   // DECODE: grad_out x the recomputed output after its activation, of this lane's output rows (for grad_alpha)
        {
            float g[8];
#pragma unroll
            for (int reg = 0; reg < 8; ++reg) {   // registers 0 .. 7 hold rows 0 .. 15
                const int orow = mlp_out_row(reg, h);
                const float z = o[reg];
                float d = 1.f;
                if (activation == GRUT_MLP_ACT_RELU) d = z > 0.f ? 1.f : 0.f;
                if (activation == GRUT_MLP_ACT_SIGMOID) {
                    const float y = 1.f / (1.f + __expf(-z));
                    d = y * (1.f - y);
                }
                float go = 0.f;
                if (valid && orow < n_out) go = grad_out[pixel * (uint64_t)n_out + orow];
                if constexpr (DECODE) {
                    float y = z;
                    if (activation == GRUT_MLP_ACT_RELU) y = fmaxf(z, 0.f);
                    if (activation == GRUT_MLP_ACT_SIGMOID) y = 1.f / (1.f + __expf(-z));
                    gy[reg] = go * y;
                    if (unpremultiply) go = go * a_s;   // the network's upstream gradient, formed before the derivative is applied
                }
                g[reg] = valid && orow < n_out ? go * d : 0.f;
            }
            dz[0] = as_frag(make_uint4(pack_bf16(g[0], g[1]), pack_bf16(g[2], g[3]), pack_bf16(g[4], g[5]), pack_bf16(g[6], g[7])));
        }
        if (need_p) {
            __syncthreads();   // the previous readers are done with both tiles
            stage_store(stage_dz, 0, st, dz[0]);   // rows 16 .. 31 of the tile stay as they are: those rows of the product are dropped
#pragma unroll
            for (int t = 0; t < KW; ++t) stage_store(stage_h, t, st, hb[NH - 1][t]);
            __syncthreads();
            if (wave < MB) dw_out = dw_tile(stage_dz, stage_h, 0, wave, rd, dw_out);   // tile `wave` of 1 x MB
        }
#pragma unroll
        for (int kb = 0; kb < MB; ++kb)   // the output matrix has 16 rows: one k-step
            acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wt_frag(image, s, NH, kb, 0, wt_lane), dz[0], zero16(), 0, 0, 0);
        gate_pack<MB>(acc, hb[NH - 1], dz);

        // ---- 3. hidden layers NH - 1 .. 1: dz is dZ of the layer, hb[layer - 1] its input ---------------------------------------------
#pragma unroll
        for (int layer = NH - 1; layer >= 1; --layer) {
            if (need_p) {
                __syncthreads();
#pragma unroll
                for (int t = 0; t < KW; ++t) {
                    stage_store(stage_dz, t, st, dz[t]);
                    stage_store(stage_h, t, st, hb[layer - 1][t]);
                }
                __syncthreads();
#pragma unroll
                for (int slot = 0; slot < kSlotsH; ++slot) {
                    const int tile = bwd_dw_tile(slot, wave);
                    if (tile < MB * MB)
                        dw_hidden[layer - 1][slot] = dw_tile(stage_dz, stage_h, tile / MB, tile % MB, rd, dw_hidden[layer - 1][slot]);
                }
            }
#pragma unroll
            for (int kb = 0; kb < MB; ++kb) {
                acc[kb] = zero16();
#pragma unroll
                for (int tp = 0; tp < KW; ++tp)
                    acc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wt_frag(image, s, layer, kb, tp, wt_lane), dz[tp], acc[kb], 0, 0, 0);
            }
            gate_pack<MB>(acc, hb[layer - 1], dz);
        }

        // ---- 4. the first layer: its input is the encoded row, encoded again -------------------------------------------------------------
        if (need_p) {
            __syncthreads();
#pragma unroll
            for (int t = 0; t < KW; ++t) stage_store(stage_dz, t, st, dz[t]);
#pragma nounroll
            for (int t = 0; t < nk0; ++t) {
                const uint4 v = __builtin_bit_cast(uint4, encode_step<DECODE>(s, t, h, row, sh, unpremultiply, a_s));
                const uint32_t rest = bwd_stage_store_offset(0, t & ~1, 0, 0);
                const uint32_t a0 = t & 1 ? st[1][0] : st[0][0], a1 = t & 1 ? st[1][1] : st[0][1];
                *reinterpret_cast<uint2*>(stage_h + a0 + rest) = make_uint2(v.x, v.y);
                *reinterpret_cast<uint2*>(stage_h + a1 + rest) = make_uint2(v.z, v.w);
            }
            __syncthreads();
#pragma unroll
            for (int slot = 0; slot < kSlots0; ++slot) {
                const int tile = bwd_dw_tile(slot, wave);
                if (tile < MB * kb0) dw_first[slot] = dw_tile(stage_dz, stage_h, tile / kb0, tile % kb0, rd, dw_first[slot]);
            }
        }
        if (need_x) {
            __syncthreads();   // both tiles are free.  They now carry dH of the encoded input from the C / D layout, where a pixel's rows are
                               // split over the two lane halves, to rows of 16 consecutive k per lane, and the SH columns to ONE lane per pixel
            float* ex = reinterpret_cast<float*>(stage_dz) + (size_t)(kTile * wave + r) * kExPitch;
            float* mine = reinterpret_cast<float*>(stage_dz) + (size_t)kBwdPixels * kExPitch + (size_t)(kTile * wave + r) * kShPitch;
            float* gx = grad_input + pixel * (uint64_t)cols;
            const bool store_x = valid && (!DECODE || grad_input != nullptr), need_a = DECODE && grad_alpha != nullptr;
            float sx = 0.f;   // DECODE: sum_j gx_j x_j, j ascending
            if constexpr (DECODE) {
                if (need_a) {   // (uniform) the SH slots are free here: they carry grad_out x y to ONE lane per pixel
#pragma unroll
                    for (int reg = 0; reg < 8; ++reg) mine[mlp_out_row(reg, h)] = gy[reg];
                }
            }
#pragma unroll
            for (int kb = 0; kb < KB0; ++kb) {
                if (kb >= kb0) break;   // (workgroup-uniform)
                f32x16 d = zero16();
#pragma unroll
                for (int tp = 0; tp < KW; ++tp)
                    d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wt_frag(image, s, 0, kb, tp, wt_first[kb]), dz[tp], d, 0, 0, 0);
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) ex[mlp_out_row(reg, h)] = d[reg];
                __syncthreads();
#pragma nounroll
                for (int i = 0; i < kStep; ++i) {   // lane half h takes k = 32 kb + 16 h + i of its pixel
                    const int k = kTile * kb + kStep * h + i;
                    const float v = ex[kStep * h + i];
                    if (k < s.n_features) {
                        if (store_x) gx[k] = unpremultiply ? v / a_s : v;
                    } else if (!DECODE && k < s.n_features + n_sh) {
                        mine[k - s.n_features] = v;
                    }
                }
                if constexpr (DECODE) {
                    if (need_a) {   // (uniform) both lane halves of a pixel walk its 32 columns of this k block, in order
#pragma nounroll
                        for (int i = 0; i < kTile; ++i) {
                            const int k = kTile * kb + i;
                            if (k < s.n_features) sx += ex[i] * (row[k] / a_s);   // x_k: the fp32 column the network saw, before its bf16 rounding
                        }
                    }
                }
                __syncthreads();
            }
            if constexpr (DECODE) {
                if (need_a && h == 0 && valid) {
                    float sy = 0.f;
                    for (int c = 0; c < n_out; ++c) sy += mine[c];
                    grad_alpha[pixel] = alpha >= 1e-8f ? sy - sx / a_s : 0.f;   // the gate of a_s = max(alpha, 1e-8f), inclusive
                }
            } else if (h == 0 && valid) {   // the SH Jacobian and the 2 of d = 2 u - 1, fp32, in the fixed order of the SH index
                const float x = dx_, y = dy_, z = dz_, xx = x * x, yy = y * y, zz = z * z;
                float jx = 0.f, jy = 0.f, jz = 0.f;
                if (s.sh_degree >= 2) {
                    jy += mine[1] * -0.48860251190291987f;
                    jz += mine[2] * 0.48860251190291987f;
                    jx += mine[3] * -0.48860251190291987f;
                }
                if (s.sh_degree >= 3) {
                    const float c2 = 1.0925484305920792f;
                    jx += mine[4] * (c2 * y), jy += mine[4] * (c2 * x);
                    jy += mine[5] * (-c2 * z), jz += mine[5] * (-c2 * y);
                    jz += mine[6] * (2.f * 0.94617469575755997f * z);
                    jx += mine[7] * (-c2 * z), jz += mine[7] * (-c2 * x);
                    jx += mine[8] * (2.f * 0.54627421529603959f * x), jy += mine[8] * (-2.f * 0.54627421529603959f * y);
                }
                if (s.sh_degree >= 4) {
                    const float c6 = 0.59004358992664352f, c7 = 2.8906114426405538f, c8 = 0.45704579946446572f, c9 = 0.3731763325901154f,
                                c10 = 1.4453057213202769f;
                    jx += mine[9] * (-6.f * c6 * x * y), jy += mine[9] * (c6 * (-3.f * xx + 3.f * yy));
                    jx += mine[10] * (c7 * y * z), jy += mine[10] * (c7 * x * z), jz += mine[10] * (c7 * x * y);
                    jy += mine[11] * (c8 * (1.f - 5.f * zz)), jz += mine[11] * (-10.f * c8 * y * z);
                    jz += mine[12] * (c9 * (15.f * zz - 3.f));
                    jx += mine[13] * (c8 * (1.f - 5.f * zz)), jz += mine[13] * (-10.f * c8 * x * z);
                    jx += mine[14] * (2.f * c10 * x * z), jy += mine[14] * (-2.f * c10 * y * z), jz += mine[14] * (c10 * (xx - yy));
                    jx += mine[15] * (c6 * (-3.f * xx + 3.f * yy)), jy += mine[15] * (6.f * c6 * x * y);
                }
                gx[s.n_features] = 2.f * jx;
                gx[s.n_features + 1] = 2.f * jy;
                gx[s.n_features + 2] = 2.f * jz;
            }
        }
    }

    // ---- the workgroup's partial of grad_params: every element of its slice is written by exactly one wave ---------------------------------
    if (need_p) {
        float* mine = partials + (size_t)blockIdx.x * num_params(s);
#pragma unroll
        for (int slot = 0; slot < kSlots0; ++slot) {
            const int tile = bwd_dw_tile(slot, wave);
            if (tile < MB * kb0) store_tile(mine, WIDTH, k0(s), tile / kb0, tile % kb0, r, h, dw_first[slot]);
        }
#pragma unroll
        for (int layer = 1; layer < NH; ++layer)
#pragma unroll
            for (int slot = 0; slot < kSlotsH; ++slot) {
                const int tile = bwd_dw_tile(slot, wave);
                if (tile < MB * MB) store_tile(mine + param_offset(s, layer), WIDTH, WIDTH, tile / MB, tile % MB, r, h, dw_hidden[layer - 1][slot]);
            }
        if (wave < MB) store_tile(mine + param_offset(s, NH), kOutRows, WIDTH, 0, wave, r, h, dw_out);
    }
}

// grad_params[i] = the workgroups' partials of element i, summed in workgroup order
__global__ __launch_bounds__(256) void mlp_backward_reduce_kernel(const float* __restrict__ partials, uint32_t n, uint32_t slices,
                                                                  float* __restrict__ grad_params) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float sum = partials[i];
    for (uint32_t b = 1; b < slices; ++b) sum += partials[(size_t)b * n + i];
    grad_params[i] = sum;
}

// the configurations the backward takes: the forward's, with at most kMaxLayers hidden layers and room for the two staged tiles
constexpr int kMaxLayers = 5;
bool taken(const Shape& s) { return s.n_hidden_layers <= kMaxLayers && bwd_lds_bytes(s) != 0; }

template <int WIDTH, int NH, int KB0, bool DECODE>
int launch(hipStream_t stream, const Shape& s, const GrutMlpConfig* c, const float* params, const float* input, const float* grad_out,
           uint32_t P, float* scratch, float* grad_input, float* grad_params, const DecodeArgs& da, float* grad_alpha) {
    int dev = 0, cus = 0;
    GRUT_HIP(hipGetDevice(&dev));
    GRUT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint32_t bytes = bwd_lds_bytes(s), grid = bwd_grid(P, (uint32_t)(cus > 0 ? cus : 1));
    if constexpr (DECODE) {
        if (bytes > 64u * 1024u)
            GRUT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_backward_kernel<WIDTH, NH, KB0, true, DecodeArgs, float*>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        mlp_backward_kernel<WIDTH, NH, KB0, true, DecodeArgs, float*><<<grid, kBlock, bytes, stream>>>(
            s, c->n_output_dims, c->output_activation, params, input, grad_out, P, grad_params ? scratch : nullptr, grad_input, da, grad_alpha);
    } else {
        if (bytes > 64u * 1024u)
            GRUT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_backward_kernel<WIDTH, NH, KB0, false>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        mlp_backward_kernel<WIDTH, NH, KB0, false><<<grid, kBlock, bytes, stream>>>(s, c->n_output_dims, c->output_activation, params, input, grad_out, P,
                                                                               grad_params ? scratch : nullptr, grad_input);
    }
    GRUT_HIP(hipGetLastError());
    if (grad_params) {
        const uint32_t n = num_params(s);
        mlp_backward_reduce_kernel<<<(n + 255u) / 256u, 256, 0, stream>>>(scratch, n, grid, grad_params);
        GRUT_HIP(hipGetLastError());
    }
    return GRUT_OK;
}


// the kernel's template parameters: width, hidden layers, and the first layer's k blocks at most (its dW tiles are registers)
template <bool DECODE>
int dispatch(hipStream_t st, const Shape& s, const GrutMlpConfig* config, const float* params, const float* input, const float* grad_out,
             uint32_t P, float* sc, float* grad_input, float* grad_params, const DecodeArgs& da, float* grad_alpha) {
    const int kb0 = s.width == 128 ? bwd_kblocks(s, 0) : kMaxK0 / kTile;
#define GRUT_MLP_BWD(W, N, K) \
    if (s.width == W && s.n_hidden_layers == N && kb0 == K) \
    return launch<W, N, K, DECODE>(st, s, config, params, input, grad_out, P, sc, grad_input, grad_params, da, grad_alpha)
#define GRUT_MLP_BWD_128(N) GRUT_MLP_BWD(128, N, 1); GRUT_MLP_BWD(128, N, 2); GRUT_MLP_BWD(128, N, 3); GRUT_MLP_BWD(128, N, 4)
    GRUT_MLP_BWD(64, 1, 4);
    GRUT_MLP_BWD(64, 2, 4);
    GRUT_MLP_BWD(64, 3, 4);
    GRUT_MLP_BWD(64, 4, 4);
    GRUT_MLP_BWD(64, 5, 4);
    GRUT_MLP_BWD_128(1);
    GRUT_MLP_BWD_128(2);
    GRUT_MLP_BWD(128, 3, 1);
    GRUT_MLP_BWD(128, 3, 2);
    GRUT_MLP_BWD(128, 3, 3);   // (K0 > 96 with 3 layers of 128 does not fit into LDS)
#undef GRUT_MLP_BWD_128
#undef GRUT_MLP_BWD
    set_last_error("%s: no kernel for width %d with %d hidden layers", DECODE ? "grut_decode_backward" : "grut_mlp_backward", s.width,
                   s.n_hidden_layers);
    return GRUT_ERR_BAD_INPUT;
}

}  // namespace
}  // namespace grut

using namespace grut;

extern "C" uint32_t grut_mlp_backward_lds_bytes(const GrutMlpConfig* config) {
    Shape s;
    return shape_of(config, &s) && taken(s) ? bwd_lds_bytes(s) : 0u;
}

extern "C" size_t grut_mlp_backward_scratch_bytes(const GrutMlpConfig* config, uint32_t P) {
    Shape s;
    if (!shape_of(config, &s) || !taken(s) || P == 0) return 0;
    return (size_t)bwd_grid(P, (uint32_t)kBwdMaxGrid) * num_params(s) * sizeof(float);
}

extern "C" int grut_mlp_backward(void* stream, const GrutMlpConfig* config, const float* params, const float* input, const float* grad_out,
                                 uint32_t P, void* scratch, float* grad_input, float* grad_params) {
    Shape s;
    GRUT_REQUIRE(shape_of(config, &s), "grut_mlp_backward: width must be 64 or 128, sh_degree 1..4, n_hidden_layers >= 1, the padded encoded "
                                       "width at most 128, n_output_dims 1..16 and the activation one of GRUT_MLP_ACT_*");
    GRUT_REQUIRE(taken(s), "grut_mlp_backward: the weight image and the two staged tiles of this configuration do not fit into LDS, or it "
                           "has more than 5 hidden layers (grut_mlp_backward_lds_bytes)");
    GRUT_REQUIRE(grad_input || grad_params, "grut_mlp_backward: grad_input and grad_params are both NULL, nothing to compute");
    GRUT_REQUIRE(P > 0 && params && input && grad_out, "grut_mlp_backward: num_pixels > 0, params, input and grad_out are required");
    GRUT_REQUIRE(!grad_params || scratch, "grut_mlp_backward: grad_params needs the scratch of grut_mlp_backward_scratch_bytes");
    GRUT_REQUIRE(((uintptr_t)params & 15u) == 0, "grut_mlp_backward: params must be 16-byte aligned");
    return dispatch<false>((hipStream_t)stream, s, config, params, input, grad_out, P, static_cast<float*>(scratch), grad_input, grad_params,
                           DecodeArgs{}, nullptr);
}

extern "C" int grut_decode_backward(void* stream, const GrutDecodeConfig* config, const float* params, const float* features, const float* alpha,
                                    const float* rays_dir, const float* rot, uint32_t num_views, uint32_t pixels_per_view, const float* grad_out,
                                    void* scratch, float* grad_features, float* grad_alpha, float* grad_params) {
    Shape s;
    DecodeArgs da;
    uint32_t P = 0;
    if (!decode_args_of("grut_decode_backward", config, alpha, rays_dir, rot, num_views, pixels_per_view, &da, &P)) return GRUT_ERR_BAD_INPUT;
    GRUT_REQUIRE(shape_of(&config->mlp, &s), "grut_decode_backward: width must be 64 or 128, sh_degree 1..4, n_hidden_layers >= 1, the padded encoded "
                                             "width at most 128, n_output_dims 1..16 and the activation one of GRUT_MLP_ACT_*");
    GRUT_REQUIRE(taken(s), "grut_decode_backward: the weight image and the two staged tiles of this configuration do not fit into LDS, or it "
                           "has more than 5 hidden layers (grut_mlp_backward_lds_bytes)");
    GRUT_REQUIRE(grad_features || grad_alpha || grad_params, "grut_decode_backward: grad_features, grad_alpha and grad_params are all NULL, nothing to compute");
    GRUT_REQUIRE(!grad_alpha || config->unpremultiply_alpha, "grut_decode_backward: grad_alpha needs unpremultiply_alpha (alpha has no gradient without it)");
    GRUT_REQUIRE(params && grad_out && (features || s.n_features == 0), "grut_decode_backward: params, features and grad_out are required");
    GRUT_REQUIRE(!grad_params || scratch, "grut_decode_backward: grad_params needs the scratch of grut_mlp_backward_scratch_bytes");
    GRUT_REQUIRE(((uintptr_t)params & 15u) == 0, "grut_decode_backward: params must be 16-byte aligned");
    return dispatch<true>((hipStream_t)stream, s, &config->mlp, params, features, grad_out, P, static_cast<float*>(scratch), grad_features, grad_params,
                          da, grad_alpha);
}
