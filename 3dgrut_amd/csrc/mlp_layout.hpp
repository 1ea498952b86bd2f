// mlp_layout.hpp — every index rule of the fused decoder MLP (mlp.hip), as __host__ __device__ functions of plain integers, so that a host
// program can run the kernel's chain with the very same arithmetic (tests/test_mlp_cpu.py emulates the 64 lanes of the MFMA with them).
//
// The model and the layout of `params`: grut_mlp_forward in include/grut_amd.h.  Everything here is about
// __builtin_amdgcn_mfma_f32_32x32x16_bf16 (D[32x32] += A[32x16] B[16x32]) with the activations kept TRANSPOSED, [neuron rows x 32 pixel
// columns]: A is a 32-row block of a weight matrix, B the layer's input, D the layer's output.  Lane l = 32 h + r holds
//   A fragment   A[row r][k = 8 h + j]       j = 0..7
//   B fragment   B[k = 8 h + j][column r]    j = 0..7
//   C / D        D[row (reg & 3) + 8 (reg >> 2) + 4 h][column r]    reg = 0..15
// A layer's D, after ReLU and packed to bf16, is the next layer's B with no lane movement: registers 8 s .. 8 s + 7 of row block b are
// the fragment of k-step t = 2 b + s.  The k order inside that step is then not the natural one; mlp_kperm states it, and because the
// weight image and the first layer's encoded input are laid out by the same rule, one rule covers all layers.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRUT_MLP_HD __host__ __device__ inline
#else
#define GRUT_MLP_HD inline
#endif

namespace grut_mlp {

constexpr int kTile = 32;             // pixels per wave step = rows of a weight block = the MFMA's M and N
constexpr int kStep = 16;             // the MFMA's K
constexpr int kFragBytes = 1024;      // one A fragment of all 64 lanes: 16 bytes each, lane-linear
constexpr int kOutRows = 16;          // rows of the output matrix in `params`
constexpr int kMaxK0 = 128;
constexpr uint32_t kLdsLimit = 160u * 1024u;   // what one workgroup may hold on gfx950

// the integers of a GrutMlpConfig that the layout depends on
struct Shape {
    int n_features, sh_degree, n_hidden_layers, width;
};

GRUT_MLP_HD int encoded_width(const Shape& s) { return s.n_features + s.sh_degree * s.sh_degree; }
GRUT_MLP_HD int k0(const Shape& s) { return (encoded_width(s) + kStep - 1) / kStep * kStep; }   // the first layer's K, padded with ones
GRUT_MLP_HD int row_blocks(const Shape& s) { return s.width / kTile; }
GRUT_MLP_HD int ksteps_first(const Shape& s) { return k0(s) / kStep; }
GRUT_MLP_HD int ksteps_hidden(const Shape& s) { return s.width / kStep; }

// which k of the layer's input element j of lane half h holds in k-step t
GRUT_MLP_HD int mlp_kperm(int t, int h, int j) { return kStep * t + 8 * (j >> 2) + 4 * h + (j & 3); }
// row of D that accumulator register reg of a lane of half h holds
GRUT_MLP_HD int mlp_out_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ---- `params`: the matrices in layer order, each row-major [out][in].  Layers 0 .. n_hidden_layers - 1 produce the hidden
// activations (layer 0: width x K0, the others width x width), layer n_hidden_layers is the output matrix (16 x width).
GRUT_MLP_HD int layer_in(const Shape& s, int layer) { return layer == 0 ? k0(s) : s.width; }
GRUT_MLP_HD int layer_out(const Shape& s, int layer) { return layer == s.n_hidden_layers ? kOutRows : s.width; }
GRUT_MLP_HD uint32_t param_offset(const Shape& s, int layer) {
    uint32_t o = 0;
    for (int l = 0; l < layer; ++l) o += (uint32_t)layer_out(s, l) * (uint32_t)layer_in(s, l);
    return o;
}
GRUT_MLP_HD uint32_t num_params(const Shape& s) { return param_offset(s, s.n_hidden_layers + 1); }

// ---- the weight image: fragments of 1 KiB, ordered (layer, row block, k-step); the output matrix is ONE row block whose rows beyond
// n_output_dims are zero.
GRUT_MLP_HD int layer_row_blocks(const Shape& s, int layer) { return layer == s.n_hidden_layers ? 1 : row_blocks(s); }
GRUT_MLP_HD int layer_ksteps(const Shape& s, int layer) { return layer == 0 ? ksteps_first(s) : ksteps_hidden(s); }
GRUT_MLP_HD uint32_t layer_first_frag(const Shape& s, int layer) {
    uint32_t f = 0;
    for (int l = 0; l < layer; ++l) f += (uint32_t)(layer_row_blocks(s, l) * layer_ksteps(s, l));
    return f;
}
GRUT_MLP_HD uint32_t num_frags(const Shape& s) { return layer_first_frag(s, s.n_hidden_layers + 1); }
GRUT_MLP_HD uint32_t image_bytes(const Shape& s) { return num_frags(s) * (uint32_t)kFragBytes; }
// fragment (row block m, k-step t) within its layer of nk k-steps
GRUT_MLP_HD int frag_in_layer(int nk, int m, int t) { return m * nk + t; }
// byte offset of lane `lane`'s 16 bytes of the fragment (layer, row block m, k-step t)
GRUT_MLP_HD uint32_t image_offset(const Shape& s, int layer, int m, int t, int lane) {
    return (layer_first_frag(s, layer) + (uint32_t)frag_in_layer(layer_ksteps(s, layer), m, t)) * (uint32_t)kFragBytes + (uint32_t)lane * 16u;
}

// Where the image's 16-byte chunk `chunk` (= fragment * 64 + lane) comes from: its 8 elements are params[*src + (j >> 2) * 8 + (j & 3)],
// j = 0..7 (two runs of four consecutive floats), or all zero when the function returns false (a padded output row).
GRUT_MLP_HD bool image_chunk_source(const Shape& s, int n_output_dims, uint32_t chunk, uint32_t* src) {
    uint32_t frag = chunk >> 6;
    const int lane = (int)(chunk & 63u), r = lane & 31, h = lane >> 5;
    int layer = 0;
    for (;; ++layer) {
        const uint32_t n = (uint32_t)(layer_row_blocks(s, layer) * layer_ksteps(s, layer));
        if (frag < n) break;
        frag -= n;
    }
    const int nk = layer_ksteps(s, layer), m = (int)frag / nk, t = (int)frag % nk;
    const int row = kTile * m + r;
    if (layer == s.n_hidden_layers && row >= n_output_dims) return false;
    *src = param_offset(s, layer) + (uint32_t)row * (uint32_t)layer_in(s, layer) + (uint32_t)mlp_kperm(t, h, 0);
    return true;
}

// ---- the encoded input: element k of a pixel's K0-vector is
//   k < F            column k of the input row
//   k < F + L^2      real SH polynomial k - F of d = 2 u - 1, u = columns F .. F + 2
//   otherwise        1
// mlp_input_element returns k itself for a feature column, -1 - (k - F) for an SH value and INT32_MIN for a one.
constexpr int kInputOne = INT32_MIN;
GRUT_MLP_HD int mlp_input_element(const Shape& s, int t, int h, int j) {
    const int k = mlp_kperm(t, h, j);
    if (k < s.n_features) return k;
    if (k < encoded_width(s)) return -1 - (k - s.n_features);
    return kInputOne;
}

// a configuration the kernel takes (the caller checks n_output_dims and the activation)
GRUT_MLP_HD bool shape_ok(const Shape& s) {
    return s.n_features >= 0 && s.sh_degree >= 1 && s.sh_degree <= 4 && s.n_hidden_layers >= 1 && s.n_hidden_layers <= 64 &&
           (s.width == 64 || s.width == 128) && k0(s) <= kMaxK0;
}
GRUT_MLP_HD uint32_t lds_bytes(const Shape& s) {
    if (!shape_ok(s)) return 0;
    const uint32_t b = image_bytes(s);
    return b <= kLdsLimit ? b : 0;
}

// ---- the backward (mlp_backward.hip) -----------------------------------------------------------------------------------------------------
// One workgroup of kBwdWaves waves takes kBwdPixels pixels per step, wave w the 32 pixels 32 w .. 32 w + 31.  Gradients keep the
// forward's orientation, [neuron rows x 32 pixel columns]: dZ of a layer in the C / D layout IS the B operand of dH = W^T dZ (k-step
// 2 b + s = registers 8 s .. 8 s + 7 of row block b, the k order of mlp_kperm), and the A operand W^T comes out of the forward's image
// through ds_read_b64_tr_b16 (bwd_wt_read_offset).  The weight gradient dW = dZ H^T sums over the pixel, the lane of both operands, so
// both cross LDS once: the workgroup stages its 128 pixels of dZ and H as [pixel][neuron] bf16 tiles (bwd_stage_*), and wave w owns the
// 32 x 32 tiles w, w + 4, .. of every layer's dW (bwd_dw_*), accumulated in registers over all steps of the workgroup.
//
// ds_read_b64_tr_b16, per group of 16 consecutive lanes: lane 4 q + p supplies the address of 4 consecutive 16-bit elements, row q of a
// 4 x 16 block at columns 4 p .. 4 p + 3; lane i receives column i, row q in its element q.
constexpr int kBwdWaves = 4, kBwdPixels = kBwdWaves * kTile;
constexpr int kBwdMaxGrid = 256;      // workgroups at most, whatever the device: the scratch is bounded by kBwdMaxGrid partials of grad_params

// 32-column blocks of a layer's input (K0 rounded up: the columns beyond K0 are computed and dropped)
GRUT_MLP_HD int bwd_kblocks(const Shape& s, int layer) { return (layer_in(s, layer) + kTile - 1) / kTile; }
// 32-column subtiles of a staged tile: wide enough for a hidden activation and for the encoded input
GRUT_MLP_HD int bwd_stage_subtiles(const Shape& s) { return row_blocks(s) > bwd_kblocks(s, 0) ? row_blocks(s) : bwd_kblocks(s, 0); }
GRUT_MLP_HD uint32_t bwd_stage_bytes(const Shape& s) { return (uint32_t)(kBwdPixels * bwd_stage_subtiles(s) * kTile * 2); }
// A staged tile [kBwdPixels pixel rows][32-column subtiles] of bf16: every subtile is a contiguous [128 pixels][32 neurons] block of 8 KiB
// with 64-byte rows whose 16-byte chunks are XOR-swizzled by the row (the conflict-free image of 8-row x 32-column subtiles, stacked):
// byte offset of chunk ch (8 neurons) of pixel row `row`.  No offset depends on the tile's width.
GRUT_MLP_HD uint32_t bwd_stage_offset(int row, int ch) {
    return (uint32_t)(kBwdPixels * 64 * (ch >> 2) + 64 * row + 16 * ((ch & 3) ^ ((row >> 2) & 3)));
}
// where lane half h of the wave's pixel row stores the 8 bytes of elements 4 c .. 4 c + 3 of a packed fragment of k-step t
// (neurons 16 t + 8 c + 4 h .. + 3)
GRUT_MLP_HD uint32_t bwd_stage_store_offset(int pixel, int t, int c, int h) { return bwd_stage_offset(pixel, 2 * t + c) + 8u * (uint32_t)h; }
// the address lane `lane` supplies to transposed read c (0, 1) of the fragment (32-neuron block blk, pixel k-step kk) of a staged tile:
// the lane then holds neuron 32 blk + (lane & 31), pixels 16 kk + 8 h + 4 c + q in element 4 c + q, as A or as B operand
GRUT_MLP_HD uint32_t bwd_stage_read_offset(int blk, int kk, int c, int lane) {
    const int h = lane >> 5, g = (lane >> 4) & 1, q = (lane & 15) >> 2, p = lane & 3;
    return bwd_stage_offset(kStep * kk + 8 * h + 4 * c + q, 4 * blk + 2 * g + (p >> 1)) + 8u * (uint32_t)(p & 1);
}
// the address lane `lane` supplies to transposed read c (0, 1) of the W^T fragment (k block kb of the layer's input, k-step tp of its
// output rows) in the FORWARD's image: the lane then holds W[row 16 tp + 8 c + 4 h + q][k = 32 kb + (lane & 31)] in element 4 c + q, the
// order of mlp_kperm.  A k-step beyond the layer's last (K0 not a multiple of 32) is clamped: those rows of dH are dropped.
GRUT_MLP_HD uint32_t bwd_wt_read_offset(const Shape& s, int layer, int kb, int tp, int c, int lane) {
    const int h = lane >> 5, g = (lane >> 4) & 1, q = (lane & 15) >> 2, p = lane & 3;
    const int row = kStep * tp + 8 * c + 4 * h + q, nk = layer_ksteps(s, layer);
    const int t = 2 * kb + g < nk ? 2 * kb + g : nk - 1;
    return image_offset(s, layer, row >> 5, t, 32 * (p & 1) + (row & 31)) + 8u * (uint32_t)(p >> 1);
}
// dW of a layer in 32 x 32 tiles, tile i = (row block i / kblocks, k block i % kblocks); wave w owns tiles w, w + kBwdWaves, ..
GRUT_MLP_HD int bwd_dw_tiles(const Shape& s, int layer) { return layer_row_blocks(s, layer) * bwd_kblocks(s, layer); }
GRUT_MLP_HD int bwd_dw_slots(const Shape& s, int layer) { return (bwd_dw_tiles(s, layer) + kBwdWaves - 1) / kBwdWaves; }
GRUT_MLP_HD int bwd_dw_tile(int slot, int wave) { return slot * kBwdWaves + wave; }

// LDS of the backward: the forward's image, then the staged dZ tile, then the staged H tile; 0 when it does not fit
GRUT_MLP_HD uint32_t bwd_lds_bytes(const Shape& s) {
    if (!lds_bytes(s)) return 0;
    const uint32_t b = image_bytes(s) + 2u * bwd_stage_bytes(s);
    return b <= kLdsLimit ? b : 0;
}
GRUT_MLP_HD uint32_t bwd_steps(uint32_t P) { return (uint32_t)(((uint64_t)P + kBwdPixels - 1) / kBwdPixels); }
GRUT_MLP_HD uint32_t bwd_grid(uint32_t P, uint32_t cus) {
    const uint32_t cap = cus < (uint32_t)kBwdMaxGrid ? (cus ? cus : 1u) : (uint32_t)kBwdMaxGrid, steps = bwd_steps(P);
    return steps < cap ? steps : cap;
}

}  // namespace grut_mlp
