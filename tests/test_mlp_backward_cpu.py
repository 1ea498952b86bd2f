"""CPU: the fused backward of the NHT decoder's network (csrc/mlp_backward.hip, 3dgrut_amd/tcnn.py) without a GPU.  The three new C
symbols and their refusals; a host emulation of the kernel's WHOLE chain - the 64 lanes of mfma_f32_32x32x16_bf16 from its A / B / C
maps, ds_read_b64_tr_b16 from its gather rule, every address from csrc/mlp_layout.hpp - against the plain int64 gradients; the torch
statement of the contract (mlp_backward_torch) against the float64 restatement (tests/mlp_backward_reference.py), which is also where
that file's tolerances are measured; and the switch.  What the kernel computes is covered by tests/test_mlp_backward_gpu.py."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import mlp_backward_reference as B
import mlp_reference as R
from test_mlp_cpu import GRID, GRID_P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("grut_mlp_backward", "grut_mlp_backward_lds_bytes", "grut_mlp_backward_scratch_bytes")
CHAIN_SHAPES = ((3, 1), (12, 3), (24, 3), (55, 4))      # (F, L): K0 = 16, 32, 48, 80, all with ones-padded columns
EMULATION_P = (1, 33, 129, 300)


@pytest.fixture()
def tcnn():
    return importlib.import_module("3dgrut_amd.tcnn")


# ---- 1. the ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_backward_symbols_are_declared_mirrored_and_exported(grut_lib):
    abi = importlib.import_module("3dgrut_amd._abi")
    header = open(os.path.join(ROOT, "include", "grut_amd.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b(int|uint32_t|size_t) {name}\(", header), name
        assert name in abi.EXPORTED_SYMBOLS
        assert hasattr(grut_lib, name) and getattr(grut_lib, name).argtypes, name
    assert abi.ABI_VERSION == 5 and grut_lib.grut_abi_version() == 5           # additive change
    assert len(grut_lib.grut_mlp_backward.argtypes) == 9

    def lds(*fields):
        return grut_lib.grut_mlp_backward_lds_bytes(ctypes.byref(abi.GrutMlpConfig(*fields)))

    def scratch(n, *fields):
        return grut_lib.grut_mlp_backward_scratch_bytes(ctypes.byref(abi.GrutMlpConfig(*fields)), n)

    # the forward's image, then two staged tiles of 128 pixels x max(width, K0 rounded up to 32) bf16
    assert lds(24, 3, 3, 128, 3, abi.MLP_ACT_SIGMOID) == (84 + 2 * 32) * 1024                 # the shipped shape is taken
    assert lds(24, 3, 3, 64, 3, abi.MLP_ACT_NONE) == (6 + 2 * 8 + 4 + 2 * 16) * 1024
    assert lds(112, 4, 1, 64, 16, abi.MLP_ACT_RELU) == (16 + 4 + 2 * 32) * 1024                # K0 = 128 sets the tiles' width
    assert lds(55, 4, 3, 128, 3, abi.MLP_ACT_NONE) == (20 + 64 + 8 + 64) * 1024
    assert lds(55, 4, 5, 64, 3, abi.MLP_ACT_NONE) != 0
    assert lds(55, 4, 5, 128, 3, abi.MLP_ACT_NONE) == 0                                       # 156 KiB of image: no room for the tiles
    assert lds(112, 4, 3, 128, 3, abi.MLP_ACT_NONE) == 0                                      # 104 + 64 KiB
    assert lds(24, 3, 6, 64, 3, abi.MLP_ACT_NONE) == 0                                        # more than 5 hidden layers
    assert lds(24, 3, 3, 32, 3, 0) == 0 and lds(24, 3, 3, 128, 17, 0) == 0 and grut_lib.grut_mlp_backward_lds_bytes(None) == 0
    # the scratch: min(ceil(P / 128), 256) partials of grad_params, whatever the device (include/grut_amd.h)
    shipped = (24, 3, 3, 128, 3, abi.MLP_ACT_SIGMOID)
    assert scratch(1, *shipped) == scratch(128, *shipped) == 40960 * 4
    assert scratch(129, *shipped) == 2 * 40960 * 4 and scratch(128 * 256, *shipped) == 256 * 40960 * 4
    assert scratch(1920 * 1080, *shipped) == scratch(2 ** 32 - 1, *shipped) == 256 * 40960 * 4
    assert scratch(0, *shipped) == 0 and scratch(100, 55, 4, 5, 128, 3, 0) == 0
    # a refused call launches nothing and says why (the pointers are never touched)
    ok, fits_not = abi.GrutMlpConfig(*shipped), abi.GrutMlpConfig(55, 4, 5, 128, 3, 0)
    sixteen, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)

    def refused(cfg, params, n, grad_input, grad_params):
        assert grut_lib.grut_mlp_backward(None, ctypes.byref(cfg), params, sixteen, sixteen, n, sixteen, grad_input, grad_params) == -1
        return grut_lib.grut_last_error()

    assert b"both NULL" in refused(ok, sixteen, 4, None, None)
    assert b"do not fit" in refused(fits_not, sixteen, 4, sixteen, sixteen)
    assert b"16-byte aligned" in refused(ok, odd, 4, sixteen, sixteen)
    assert b"num_pixels > 0" in refused(ok, sixteen, 0, sixteen, sixteen)
    assert b"width must be" in refused(abi.GrutMlpConfig(24, 3, 3, 32, 3, 0), sixteen, 4, sixteen, sixteen)


# ---- 2. the kernel's chain, emulated on the host ----------------------------------------------------------------------------------------------
EMULATION = r"""
// Runs the whole chain of csrc/mlp_backward.hip on the host, workgroup step by workgroup step and wave by wave: the 64 lanes of
// mfma_f32_32x32x16_bf16 emulated from the instruction's A / B / C maps, ds_read_b64_tr_b16 from its gather rule, every index and every
// LDS address from mlp_layout.hpp, exact small-integer data.  Reads one case, writes dH of the encoded input and grad_params per P.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mlp_layout.hpp"
using namespace grut_mlp;

typedef float Frag[64][8];
typedef float Acc[64][16];

// D = A B + C with lane l = 32 h + r holding A[r][8 h + j], B[8 h + j][r] and D[(reg & 3) + 8 (reg >> 2) + 4 h][r]
static void mfma(const Frag a, const Frag b, Acc acc) {
    static float A[32][16], B[16][32], D[32][32];
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) A[l & 31][8 * (l >> 5) + j] = a[l][j], B[8 * (l >> 5) + j][l & 31] = b[l][j];
    for (int l = 0; l < 64; ++l)
        for (int reg = 0; reg < 16; ++reg) D[(reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5)][l & 31] = acc[l][reg];
    for (int i = 0; i < 32; ++i)
        for (int k = 0; k < 16; ++k) {
            const float av = A[i][k];
            for (int n = 0; n < 32; ++n) D[i][n] += av * B[k][n];
        }
    for (int l = 0; l < 64; ++l)
        for (int reg = 0; reg < 16; ++reg) acc[l][reg] = D[(reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5)][l & 31];
}

static void die(const char* what, int a, int b) { printf("%s (%d, %d)\n", what, a, b); exit(1); }

// ds_read_b64_tr_b16 on an LDS of 16-bit elements (one float each here): per group of 16 consecutive lanes, lane 4 q + p supplies the byte
// address of row q, columns 4 p .. 4 p + 3 of a 4 x 16 block; lane i receives column i, row q in element q.  Two reads make a fragment.
static void tr_fragment(const std::vector<float>& lds, const uint32_t (&addr)[2][64], Frag out) {
    for (int c = 0; c < 2; ++c)
        for (int g = 0; g < 4; ++g) {
            float block[4][16];
            for (int q = 0; q < 4; ++q)
                for (int p = 0; p < 4; ++p) {
                    const uint32_t a = addr[c][16 * g + 4 * q + p];
                    if (a % 8 || a / 2 + 4 > lds.size()) die("transposed read: address", (int)a, 16 * g + 4 * q + p);
                    for (int e = 0; e < 4; ++e) block[q][4 * p + e] = lds[a / 2 + e];
                }
            for (int i = 0; i < 16; ++i)
                for (int q = 0; q < 4; ++q) out[16 * g + i][4 * c + q] = block[q][i];
        }
}

static bool is_bf16(float v) { unsigned u; memcpy(&u, &v, 4); return (u & 0xffffu) == 0; }

struct Wave {
    Frag enc[8], hb[5][8], dz[8];
    Acc acc[4], out, dw_first[4], dw_hidden[4][4], dw_out;
    bool valid[32];
    long pixel[32];
};
static Wave waves[kBwdWaves];

static void run(const Shape& s, int n_out, int relu_out, int P, const float* params, const float* enc, const float* gout, float* dh0, float* gp) {
    const int NH = s.n_hidden_layers, K0 = k0(s), MB = row_blocks(s), KW = ksteps_hidden(s), nk0 = ksteps_first(s), kb0 = bwd_kblocks(s, 0);
    if (NH > 5 || MB > 4) die("shape", NH, MB);
    std::vector<float> image((size_t)num_frags(s) * 64 * 8, NAN);
    for (uint32_t c = 0; c < num_frags(s) * 64u; ++c) {
        uint32_t src = 0;
        const bool live = image_chunk_source(s, n_out, c, &src);
        for (int j = 0; j < 8; ++j) image[(size_t)c * 8 + j] = live ? params[src + (j >> 2) * 8 + (j & 3)] : 0.f;
    }
    // the two staged tiles start as NaN: whatever the chain reads before writing it must land in rows or columns that are dropped
    std::vector<float> stage_dz(bwd_stage_bytes(s) / 2, NAN), stage_h(bwd_stage_bytes(s) / 2, NAN);
    if (bwd_stage_bytes(s) != (uint32_t)(kBwdPixels * bwd_stage_subtiles(s) * 64)) die("stage bytes", 0, 0);
    static Frag a, b;
    auto weights = [&](int layer, int m, int t, Frag f) {
        for (int l = 0; l < 64; ++l) memcpy(f[l], &image[image_offset(s, layer, m, t, l) / 2], 32);
    };
    auto wt = [&](int layer, int kb, int tp, Frag f) {   // a W^T fragment out of the forward's image
        uint32_t addr[2][64];
        for (int c = 0; c < 2; ++c)
            for (int l = 0; l < 64; ++l) {
                addr[c][l] = bwd_wt_read_offset(s, layer, kb, tp, c, l);
                // the kernel's split into a per-lane part and a uniform rest: one lane part for all layers >= 1, one per k block of layer 0
                const uint32_t lane_part = layer ? bwd_wt_read_offset(s, 1, 0, 0, 0, l) - bwd_wt_read_offset(s, 1, 0, 0, 0, 0)
                                                 : bwd_wt_read_offset(s, 0, kb, 0, 0, l) - bwd_wt_read_offset(s, 0, kb, 0, 0, 0);
                if (addr[c][l] != lane_part + bwd_wt_read_offset(s, layer, kb, tp, c, 0)) die("W^T address split", layer, l);
                if (addr[c][l] + 8 > image_bytes(s)) die("W^T address", layer, l);
            }
        tr_fragment(image, addr, f);
    };
    auto store = [&](std::vector<float>& tile, int wave, int t, const Frag f) {
        for (int l = 0; l < 64; ++l)
            for (int c = 0; c < 2; ++c) {
                const int r = l & 31, h = l >> 5;
                const uint32_t off = bwd_stage_store_offset(kTile * wave + r, t, c, h);
                if (off != bwd_stage_store_offset(kTile * wave + r, t & 1, c, h) + bwd_stage_store_offset(0, t & ~1, 0, 0)) die("store address split", t, l);
                if (off % 8 || off + 8 > bwd_stage_bytes(s)) die("store address", t, l);
                for (int e = 0; e < 4; ++e) {
                    if (!is_bf16(f[l][4 * c + e])) die("a staged value is not exact in bf16", t, l);
                    tile[off / 2 + e] = f[l][4 * c + e];
                }
            }
    };
    auto staged = [&](const std::vector<float>& tile, int blk, int kk, Frag f) {
        uint32_t addr[2][64];
        for (int c = 0; c < 2; ++c)
            for (int l = 0; l < 64; ++l) {
                addr[c][l] = bwd_stage_read_offset(blk, kk, c, l);
                if (addr[c][l] != bwd_stage_read_offset(0, 0, c, l) + bwd_stage_read_offset(blk, kk, 0, 0)) die("read address split", blk, l);
                if (addr[c][l] + 8 > bwd_stage_bytes(s)) die("read address", blk, l);
            }
        tr_fragment(tile, addr, f);
    };
    auto dw_tile = [&](int m, int kb, Acc acc) {
        for (int kk = 0; kk < kBwdPixels / kStep; ++kk) staged(stage_dz, m, kk, a), staged(stage_h, kb, kk, b), mfma(a, b, acc);
    };
    auto gate_pack = [&](Wave& w, int input) {   // dH in acc -> dZ of the layer below, gated by the packed activation hb[input]
        for (int blk = 0; blk < MB; ++blk)
            for (int sub = 0; sub < 2; ++sub)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const float v = w.hb[input][2 * blk + sub][l][j] != 0.f ? w.acc[blk][l][8 * sub + j] : 0.f;
                        if (!is_bf16(v) || std::fabs(v) > 256.f) die("dZ is not exact in bf16", input, l);
                        w.dz[2 * blk + sub][l][j] = v;
                    }
    };
    for (auto& w : waves) memset(w.dw_first, 0, sizeof w.dw_first), memset(w.dw_hidden, 0, sizeof w.dw_hidden), memset(w.dw_out, 0, sizeof w.dw_out);
    if (bwd_dw_slots(s, 0) > 4 || (NH > 1 && bwd_dw_slots(s, 1) > 4) || bwd_dw_slots(s, NH) != 1) die("slots", 0, 0);

    const uint32_t steps = bwd_steps((uint32_t)P);
    for (uint32_t step = 0; step < steps; ++step) {   // (one workgroup takes every step: the partials' sum is exact anyway)
        for (int wv = 0; wv < kBwdWaves; ++wv) {
            Wave& w = waves[wv];
            // ---- the forward again
            memset(w.acc, 0, sizeof w.acc);
            for (int r = 0; r < 32; ++r) w.pixel[r] = (long)step * kBwdPixels + kTile * wv + r, w.valid[r] = w.pixel[r] < P;
            for (int t = 0; t < nk0; ++t) {
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j) {
                        const int e = mlp_input_element(s, t, l >> 5, j);
                        const float* row = enc + (size_t)(w.valid[l & 31] ? w.pixel[l & 31] : P - 1) * K0;
                        w.enc[t][l][j] = e >= 0 ? row[e] : e == kInputOne ? 1.f : row[s.n_features + (-1 - e)];
                    }
                for (int m = 0; m < MB; ++m) weights(0, m, t, a), mfma(a, w.enc[t], w.acc[m]);
            }
            for (int layer = 1; layer <= NH; ++layer) {
                for (int blk = 0; blk < MB; ++blk)
                    for (int sub = 0; sub < 2; ++sub)
                        for (int l = 0; l < 64; ++l)
                            for (int j = 0; j < 8; ++j) w.hb[layer - 1][2 * blk + sub][l][j] = std::fmax(w.acc[blk][l][8 * sub + j], 0.f);
                if (layer < NH) {
                    memset(w.acc, 0, sizeof w.acc);
                    for (int m = 0; m < MB; ++m)
                        for (int t = 0; t < KW; ++t) weights(layer, m, t, a), mfma(a, w.hb[layer - 1][t], w.acc[m]);
                } else {
                    memset(w.out, 0, sizeof w.out);
                    for (int t = 0; t < KW; ++t) weights(layer, 0, t, a), mfma(a, w.hb[layer - 1][t], w.out);
                }
            }
            // ---- dZ of the output layer: registers 0 .. 7 hold rows 0 .. 15
            for (int l = 0; l < 64; ++l)
                for (int reg = 0; reg < 8; ++reg) {
                    const int orow = mlp_out_row(reg, l >> 5), r = l & 31;
                    const float d = relu_out ? (w.out[l][reg] > 0.f ? 1.f : 0.f) : 1.f;
                    w.dz[0][l][reg] = w.valid[r] && orow < n_out ? gout[(size_t)w.pixel[r] * n_out + orow] * d : 0.f;
                }
        }
        // ---- the output layer (the barriers of the kernel separate these loops over the waves)
        for (int wv = 0; wv < kBwdWaves; ++wv) {
            store(stage_dz, wv, 0, waves[wv].dz[0]);
            for (int t = 0; t < KW; ++t) store(stage_h, wv, t, waves[wv].hb[NH - 1][t]);
        }
        for (int wv = 0; wv < kBwdWaves; ++wv) {
            Wave& w = waves[wv];
            if (wv < MB) dw_tile(0, wv, w.dw_out);
            memset(w.acc, 0, sizeof w.acc);
            for (int kb = 0; kb < MB; ++kb) wt(NH, kb, 0, a), mfma(a, w.dz[0], w.acc[kb]);
            gate_pack(w, NH - 1);
        }
        // ---- hidden layers NH - 1 .. 1
        for (int layer = NH - 1; layer >= 1; --layer) {
            for (int wv = 0; wv < kBwdWaves; ++wv)
                for (int t = 0; t < KW; ++t) store(stage_dz, wv, t, waves[wv].dz[t]), store(stage_h, wv, t, waves[wv].hb[layer - 1][t]);
            for (int wv = 0; wv < kBwdWaves; ++wv) {
                Wave& w = waves[wv];
                for (int slot = 0; slot < bwd_dw_slots(s, layer); ++slot) {
                    const int tile = bwd_dw_tile(slot, wv);
                    if (tile < bwd_dw_tiles(s, layer)) dw_tile(tile / MB, tile % MB, w.dw_hidden[layer - 1][slot]);
                }
                memset(w.acc, 0, sizeof w.acc);
                for (int kb = 0; kb < MB; ++kb)
                    for (int tp = 0; tp < KW; ++tp) wt(layer, kb, tp, a), mfma(a, w.dz[tp], w.acc[kb]);
                gate_pack(w, layer - 1);
            }
        }
        // ---- the first layer
        for (int wv = 0; wv < kBwdWaves; ++wv) {
            for (int t = 0; t < KW; ++t) store(stage_dz, wv, t, waves[wv].dz[t]);
            for (int t = 0; t < nk0; ++t) store(stage_h, wv, t, waves[wv].enc[t]);
        }
        for (int wv = 0; wv < kBwdWaves; ++wv) {
            Wave& w = waves[wv];
            for (int slot = 0; slot < bwd_dw_slots(s, 0); ++slot) {
                const int tile = bwd_dw_tile(slot, wv);
                if (tile < bwd_dw_tiles(s, 0)) dw_tile(tile / kb0, tile % kb0, w.dw_first[slot]);
            }
            for (int kb = 0; kb < kb0; ++kb) {
                static Acc d;
                memset(d, 0, sizeof d);
                for (int tp = 0; tp < KW; ++tp) wt(0, kb, tp, a), mfma(a, w.dz[tp], d);
                for (int l = 0; l < 64; ++l)
                    for (int reg = 0; reg < 16; ++reg) {
                        const int k = kTile * kb + mlp_out_row(reg, l >> 5);
                        if (k < K0 && w.valid[l & 31]) dh0[(size_t)w.pixel[l & 31] * K0 + k] = d[l][reg];
                    }
            }
        }
    }
    // ---- every element of grad_params is written by exactly one wave
    std::vector<int> written(num_params(s), 0);
    auto store_tile = [&](uint32_t base, int rows, int cols, int m, int kb, const Acc acc) {
        for (int l = 0; l < 64; ++l)
            for (int reg = 0; reg < 16; ++reg) {
                const int row = kTile * m + mlp_out_row(reg, l >> 5), k = kTile * kb + (l & 31);
                if (row < rows && k < cols) gp[base + (size_t)row * cols + k] = acc[l][reg], ++written[base + (size_t)row * cols + k];
            }
    };
    for (int wv = 0; wv < kBwdWaves; ++wv) {
        for (int layer = 0; layer < NH; ++layer)
            for (int slot = 0; slot < bwd_dw_slots(s, layer); ++slot) {
                const int tile = bwd_dw_tile(slot, wv), kbs = bwd_kblocks(s, layer);
                if (tile < bwd_dw_tiles(s, layer))
                    store_tile(param_offset(s, layer), s.width, layer_in(s, layer), tile / kbs, tile % kbs,
                               layer == 0 ? waves[wv].dw_first[slot] : waves[wv].dw_hidden[layer - 1][slot]);
            }
        if (wv < MB) store_tile(param_offset(s, NH), kOutRows, s.width, 0, wv, waves[wv].dw_out);
    }
    for (uint32_t i = 0; i < num_params(s); ++i)
        if (written[i] != 1) die("grad_params element not written exactly once", (int)i, written[i]);
}

int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    int head[7];
    if (!in || !out || fread(head, 4, 7, in) != 7) die("input", 0, 0);
    const Shape s{head[0], head[1], head[2], head[3]};
    const int n_out = head[4], relu_out = head[5], rows = head[6], K0 = k0(s);
    if (!shape_ok(s)) die("shape not taken", 0, 0);
    std::vector<float> params(num_params(s)), enc((size_t)rows * K0), gout((size_t)rows * n_out);
    if (fread(params.data(), 4, params.size(), in) != params.size() || fread(enc.data(), 4, enc.size(), in) != enc.size() ||
        fread(gout.data(), 4, gout.size(), in) != gout.size())
        die("input arrays", 0, 0);
    for (int i = 3; i < argc; ++i) {
        const int P = atoi(argv[i]);
        if (P < 1 || P > rows) die("P", P, rows);
        std::vector<float> dh0((size_t)P * K0, NAN), gp(num_params(s), NAN);
        run(s, n_out, relu_out, P, params.data(), enc.data(), gout.data(), dh0.data(), gp.data());
        fwrite(dh0.data(), 4, dh0.size(), out);
        fwrite(gp.data(), 4, gp.size(), out);
    }
    fclose(out);
    return 0;
}
"""


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    """the host program, compiled once; fails on a tree without the backward's layout functions"""
    d = tmp_path_factory.mktemp("mlp_backward_lanes")
    src, exe = d / "lanes.cpp", d / "lanes"
    src.write_text(EMULATION)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "3dgrut_amd", "csrc"), str(src), "-o", str(exe)])
    return d, exe


@pytest.mark.parametrize("layers", [1, 2, 3, 5])
@pytest.mark.parametrize("width", [64, 128])
def test_lane_map_emulation_of_the_backward_reproduces_the_integer_gradients(emulator, width, layers):
    d, exe = emulator
    rows = max(EMULATION_P)
    for index, ((f, degree), n_out) in enumerate((shape, n) for shape in CHAIN_SHAPES for n in (3, 16)):
        act = ("none", "relu")[index % 2]
        cfg = R.Config(f, degree, layers, width, n_out, act)
        params, x, go = R.integer_network(cfg), R.integer_input(cfg, rows), B.integer_grad_out(cfg, rows)
        k0, n_sh = R.k0(cfg), degree ** 2
        enc = np.concatenate([x[:, :f], np.zeros((rows, n_sh), np.float32), np.ones((rows, k0 - f - n_sh), np.float32)], axis=1)
        with open(d / "case.bin", "wb") as fh:
            fh.write(np.array([f, degree, layers, width, n_out, act == "relu", rows], np.int32).tobytes())
            for a in (params, enc, go):
                fh.write(np.ascontiguousarray(a, np.float32).tobytes())
        done = subprocess.run([str(exe), str(d / "case.bin"), str(d / "out.bin"), *map(str, EMULATION_P)], capture_output=True, text=True)
        assert done.returncode == 0, (cfg, done.stdout + done.stderr)
        got = np.fromfile(d / "out.bin", np.float32)
        offset = 0
        for n in EMULATION_P:
            dh0 = got[offset:offset + n * k0].reshape(n, k0)
            gp = got[offset + n * k0:offset + n * k0 + R.n_params(cfg)]
            offset += n * k0 + R.n_params(cfg)
            want_x, want_p, (big_dz, big_sum) = B.integer_backward(params, x[:n], go[:n], cfg)
            assert big_dz <= 256 and big_sum < 2 ** 24
            assert np.array_equal(dh0[:, :f], want_x.astype(np.float32)), (cfg, n)
            assert not dh0[:, f:f + n_sh].any(), (cfg, n)                         # the SH columns meet zero weights
            assert np.array_equal(gp, want_p.astype(np.float32)), (cfg, n, np.argwhere(gp != want_p)[:4])
            if n == rows:
                assert np.count_nonzero(want_x) > want_x.size // 32 and np.count_nonzero(want_p) > want_p.size // 256   # not a dead network
        assert offset == got.size


# ---- 3. mlp_backward_torch against the restatement ----------------------------------------------------------------------------------------------
def test_backward_bf16_without_roundings_is_the_derivative_of_the_forward():
    """central differences on the network WITHOUT the roundings; with them off backward_bf16 is R.backward"""
    rng = np.random.default_rng(0)
    for act in ("none", "relu", "sigmoid"):
        cfg = R.Config(5, 4, 2, 16, 3, act)
        params = R.xavier_params(rng, cfg).astype(np.float64) * 2
        x = R.random_input(rng, 6, 5, 3.0).astype(np.float64)
        g = rng.normal(size=(6, 3))
        _, cache = R.forward(params, x, cfg, rounding=False)
        gx, gp = B.backward_bf16(cache, g, cfg, rounding=False)
        assert np.array_equal(gx, R.backward(cache, g, cfg)[0]) and np.array_equal(gp, R.backward(cache, g, cfg)[1])
        eps = 1e-6
        for arr, grad, picks in ((x, gx, [(0, 0), (1, 4), (2, 5), (3, 6), (4, 7), (5, 2)]), (params, gp, [0, 17, 16 * 32 + 3, 16 * 32 + 16 * 16 + 5])):
            for i in picks:
                keep = arr[i]
                arr[i] = keep + eps
                hi = (R.forward(params, x, cfg, rounding=False)[0] * g).sum()
                arr[i] = keep - eps
                lo = (R.forward(params, x, cfg, rounding=False)[0] * g).sum()
                arr[i] = keep
                assert abs((hi - lo) / (2 * eps) - grad[i]) <= 1e-6 * max(1.0, abs(grad[i])), (act, i)
        # and the roundings of dZ move it by no more than bf16's 2^-9 per rounded factor along the chain
        _, cache = R.forward(params, x, cfg)
        rx, rp = B.backward_bf16(cache, g, cfg)
        ux, up = R.backward(cache, g, cfg)
        assert 0 < np.abs(rx - ux).max() <= 4 * 2.0 ** -9 * np.abs(ux).max() and 0 < np.abs(rp - up).max() <= 4 * 2.0 ** -9 * np.abs(up).max()


def _deviation(tcnn, cfg, params, x, grad_out):
    """max |mlp_backward_torch (fp32, CPU) - backward_bf16 (float64)| of both gradients"""
    _, cache = R.forward(params, x, cfg)
    wx, wp = B.backward_bf16(cache, grad_out, cfg)
    gx, gp = tcnn.mlp_backward_torch(torch.from_numpy(params), torch.from_numpy(x), torch.from_numpy(grad_out).float(), tcnn.MlpConfig(*cfg))
    assert gx.dtype == gp.dtype == torch.float32 and gx.shape == wx.shape and gp.shape == wp.shape
    rows = R.matrices(cfg)[-1][1] * (R.OUT_ROWS - cfg.n_output_dims)
    assert not gp[-rows:].any() and not wp[-rows:].any()                          # the padded output rows: exactly zero
    return np.array([np.abs(gx.numpy() - wx).max(), np.abs(gp.numpy() - wp).max()])


def test_mlp_backward_torch_agrees_with_the_restatement(tcnn):
    worst = np.zeros(2)
    for index, (f, degree, width, layers, act, scale) in enumerate(GRID):
        cfg = R.Config(f, degree, layers, width, 3, act)
        rng = np.random.default_rng(1000 + index)
        params, x = R.xavier_params(rng, cfg), R.random_input(rng, GRID_P, f, scale)
        worst = np.maximum(worst, _deviation(tcnn, cfg, params, x, rng.normal(size=(GRID_P, 3))))
    for name in sorted(R.PARITY_CASES):
        cfg, params, x = R.parity_case(name)
        worst = np.maximum(worst, _deviation(tcnn, cfg, params, x, parity_grad_out(name)))
    print(f"\nmlp_backward_torch vs backward_bf16 over {len(GRID)} cases of {GRID_P} pixels and the parity cases: d/dx {worst[0]:.3e}, "
          f"d/dparams {worst[1]:.3e}  (BWD_GRAD_X_TOL {B.BWD_GRAD_X_TOL:.3e}, BWD_GRAD_PARAMS_TOL {B.BWD_GRAD_PARAMS_TOL:.3e})")
    assert worst[0] <= 2 * B.BWD_GRAD_X_TOL and worst[1] <= 2 * B.BWD_GRAD_PARAMS_TOL


def parity_grad_out(name):
    """grad_out ~ N(0, 1) of a parity case, the same array wherever it is called (the GPU test imports it)"""
    cfg, n_pixels, _, seed = R.PARITY_CASES[name]
    return np.random.default_rng(seed + 500).normal(size=(n_pixels, cfg.n_output_dims))


def test_mlp_backward_torch_on_the_gate_exact_cases(tcnn):
    worst = np.zeros(2)
    for name in sorted(B.GATE_EXACT_CASES):
        cfg, params, x, go = B.gate_exact_case(name)
        dev = _deviation(tcnn, cfg, params, x, go.astype(np.float64))
        print(f"\n{name}: mlp_backward_torch vs backward_bf16, d/dx {dev[0]:.3e}, d/dparams {dev[1]:.3e}")
        worst = np.maximum(worst, dev)
    print(f"\ngate-exact cases: d/dx {worst[0]:.3e}, d/dparams {worst[1]:.3e}  (GATE_EXACT_GRAD_X_TOL {B.GATE_EXACT_GRAD_X_TOL:.3e}, "
          f"GATE_EXACT_GRAD_PARAMS_TOL {B.GATE_EXACT_GRAD_PARAMS_TOL:.3e})")
    assert worst[0] <= 2 * B.GATE_EXACT_GRAD_X_TOL and worst[1] <= 2 * B.GATE_EXACT_GRAD_PARAMS_TOL
    assert B.GATE_EXACT_GRAD_X_TOL < B.BWD_GRAD_X_TOL / 10 and B.GATE_EXACT_GRAD_PARAMS_TOL < B.BWD_GRAD_PARAMS_TOL / 10   # no gate flips


def test_mlp_backward_torch_dtypes(tcnn):
    cfg = tcnn.MlpConfig(12, 3, 2, 64, 3, "sigmoid")
    rng = np.random.default_rng(4)
    params, x = torch.from_numpy(R.xavier_params(rng, R.Config(*cfg))), torch.from_numpy(R.random_input(rng, 9, 12, 3.0))
    go = torch.from_numpy(rng.normal(size=(9, 3))).float()
    gx, gp = tcnn.mlp_backward_torch(params, x, go, cfg)
    dx, dp = tcnn.mlp_backward_torch(params, x.double(), go, cfg)
    assert dx.dtype == dp.dtype == torch.float64 and gx.dtype == torch.float32
    _, cache = R.forward(params.numpy(), x.numpy(), R.Config(*cfg))
    wx, wp = B.backward_bf16(cache, go.numpy().astype(np.float64), R.Config(*cfg))
    assert np.abs(dx.numpy() - wx).max() <= 1e-9 and np.abs(dp.numpy() - wp).max() <= 1e-9   # float64 against float64: the same roundings
    assert not params.requires_grad and gx.requires_grad is False


# ---- 4. the switch ----------------------------------------------------------------------------------------------------------------------------------
def test_the_switch_is_off_by_default_idempotent_and_leaves_cpu_tensors_alone(tcnn):
    assert tcnn.install_fused_backward(False) is False                            # off by default
    cfg = tcnn.MlpConfig(24, 3, 3, 128, 3, "sigmoid")
    rng = np.random.default_rng(8)
    params, x = R.xavier_params(rng, R.Config(*cfg)), R.random_input(rng, 19, 24, 3.0)
    go = torch.from_numpy(rng.normal(size=(19, 3))).float()

    def grads():
        p, v = torch.from_numpy(params).requires_grad_(True), torch.from_numpy(x).requires_grad_(True)
        return torch.autograd.grad(tcnn.mlp(p, v, cfg), [v, p], go)

    before = grads()
    try:
        assert tcnn.install_fused_backward() is False
        assert tcnn.install_fused_backward() is True and tcnn.install_fused_backward(True) is True
        calls = tcnn.stats["hip_backward_calls"]
        after = grads()                                                           # a CPU tensor: today's path, today's gradients
        assert tcnn.stats["hip_backward_calls"] == calls
        assert all(torch.equal(a, b) for a, b in zip(before, after))
    finally:
        assert tcnn.install_fused_backward(False) is True
    assert tcnn.install_fused_backward(False) is False
