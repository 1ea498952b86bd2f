// mlp.hip — the NHT decoder's network (threedgrut/model/feature_decoder.py: tinycudann's NetworkWithInputEncoding) as ONE fused HIP
// forward kernel: encoding, every layer and the output activation, with nothing but the input row and the output row in memory.
// The model: grut_mlp_forward in include/grut_amd.h.  Every index rule: mlp_layout.hpp (shared with the host emulation of the tests).
// The same kernel with another input source is the NHT decode stage (grut_decode_forward): the feature map, the camera rays, the poses and
// alpha are read where they lie instead of assembled rows.
//
// Layout.  Persistent grid, one workgroup of four waves per CU (one wave per SIMD).  Each workgroup reads the fp32 `params` ITSELF,
// rounds them to bf16 and writes the fragment-ordered image into LDS before its first tile: there is no prepared copy of the weights
// anywhere, so a weight change of any kind (optimizer step, param.data.copy_ of the decoder's EMA) is seen by the next launch.
// A wave then takes kColTiles tiles of 32 pixels per step.  Activations stay in registers, transposed ([neuron rows x 32 pixel columns]):
// a layer is acc[m] = mfma_f32_32x32x16_bf16(W fragment (m, t) from LDS, H fragment t, acc[m]) over the row blocks m and k-steps t, and
// its fp32 result, after ReLU and packed pairwise to bf16, IS the next layer's H operand (registers 8 s .. 8 s + 7 of row block b are
// k-step 2 b + s).  One 16-byte LDS read per lane and fragment, lane-linear, shared by the kColTiles column tiles.
// EXEC is all ones around every MFMA: a tail tile clamps its loads to the last pixel and masks its stores; nothing branches per lane.
#include "common.hpp"
#include "mlp_layout.hpp"

namespace grut {
namespace {

#include "mlp_device.inl"

constexpr int kWavesPerBlock = 4, kBlock = kWavesPerBlock * GRUT_WAVE;
constexpr int kColTiles = 2;   // column tiles (of 32 pixels) that share one weight fragment read: LDS bytes per pixel halve

// DECODE is the input source: false, rows [P, F + 3] with the direction's u in the last three columns (grut_mlp_forward);
// true, the decode stage (grut_decode_forward): `input` is the feature map [P, F], the direction comes from decode_direction, and with
// da.unpremultiply the feature columns are divided by a_s = max(alpha, 1e-8f) and the result is multiplied by it.  Everything from the
// encoded input on is the same code.  `extra` is empty for the rows and one DecodeArgs for the decode stage.
template <int WIDTH, bool DECODE, class... Extra>
__global__ __launch_bounds__(kBlock) void mlp_forward_kernel(Shape s, int n_out, int activation, const float* __restrict__ params,
                                                             const float* __restrict__ input, uint32_t P, float* __restrict__ out, Extra... extra) {
    static_assert(sizeof...(Extra) == (DECODE ? 1 : 0), "one DecodeArgs for the decode stage, nothing for the rows");
    const DecodeArgs da = decode_args(extra...);
    constexpr int MB = WIDTH / kTile, KW = WIDTH / kStep;
    extern __shared__ __attribute__((aligned(16))) unsigned char image[];

    // ---- the weight image, from the live fp32 parameters -----------------------------------------------------------------------------
    build_image(s, n_out, params, image, kBlock);
    __syncthreads();

    const int lane = threadIdx.x & (GRUT_WAVE - 1), r = lane & 31, h = lane >> 5;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / GRUT_WAVE));
    const int nk0 = ksteps_first(s), nh = s.n_hidden_layers, cols = DECODE ? s.n_features : s.n_features + 3;
    const bool unpremultiply = DECODE && da.unpremultiply;
    const uint32_t steps = (uint32_t)(((uint64_t)P + kColTiles * kTile - 1) / (kColTiles * kTile));

    // DECODE: lane half h computes the direction of column tile h (once per pixel, not twice; the halves swap afterwards), from inputs
    // that were loaded one step ahead: the wave has nothing else in flight to hide that latency behind
    const auto direction_input = [&](uint32_t step) {
        const uint64_t mine = ((uint64_t)step * kColTiles + h) * kTile + r;
        return decode_direction_load(da, (uint32_t)(mine < P ? mine : (uint64_t)P - 1));
    };
    DirectionInput ahead{};
    if constexpr (DECODE) ahead = direction_input(blockIdx.x * kWavesPerBlock + wave < steps ? blockIdx.x * kWavesPerBlock + wave : 0u);
    for (uint32_t step = blockIdx.x * kWavesPerBlock + wave; step < steps; step += gridDim.x * kWavesPerBlock) {
        f32x16 acc[kColTiles][MB];
        uint64_t pixel[kColTiles];
        // ---- layer 0: the encoded input, k-step by k-step ---------------------------------------------------------------------------
        const float* row[kColTiles];
        f32x16 sh[kColTiles];
        float a_s[kColTiles], dir[kColTiles][3];
        if constexpr (DECODE) {
            static_assert(kColTiles == 2, "one column tile per lane half");
            const DirectionInput now = ahead;
            const uint32_t next = step + gridDim.x * kWavesPerBlock;
            ahead = direction_input(next < steps ? next : step);   // (a wave's last step loads its own inputs again)
            float d[3];
            decode_direction(da, now, d);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float other = __shfl_xor(d[i], 32);
                dir[0][i] = h ? other : d[i], dir[1][i] = h ? d[i] : other;
            }
        }
#pragma unroll
        for (int c = 0; c < kColTiles; ++c) {
            pixel[c] = ((uint64_t)step * kColTiles + c) * kTile + r;
            const uint64_t src = pixel[c] < P ? pixel[c] : (uint64_t)P - 1;   // a tail lane reads the last pixel and stores nothing
            row[c] = input + src * cols;
            a_s[c] = 1.f;
            if constexpr (DECODE) {
                sh[c] = sh_values(dir[c][0], dir[c][1], dir[c][2]);
                if (unpremultiply) a_s[c] = fmaxf(da.alpha[src], 1e-8f);
            } else {
                const float* u = row[c] + s.n_features;
                sh[c] = sh_values(2.f * u[0] - 1.f, 2.f * u[1] - 1.f, 2.f * u[2] - 1.f);
            }
#pragma unroll
            for (int m = 0; m < MB; ++m) acc[c][m] = zero16();
        }
        const unsigned char* w = image + image_offset(s, 0, 0, 0, lane);
#pragma nounroll
        for (int t = 0; t < nk0; ++t) {
            bf16x8 b[kColTiles];
#pragma unroll
            for (int c = 0; c < kColTiles; ++c) b[c] = encode_step<DECODE>(s, t, h, row[c], sh[c], unpremultiply, a_s[c]);
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                const bf16x8 a = as_frag(*reinterpret_cast<const uint4*>(w + (size_t)frag_in_layer(nk0, m, t) * kFragBytes));
#pragma unroll
                for (int c = 0; c < kColTiles; ++c) acc[c][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[c], acc[c][m], 0, 0, 0);
            }
        }
        // ---- hidden layers 1 .. nh - 1 ---------------------------------------------------------------------------------------------
        bf16x8 hb[kColTiles][KW];
        for (int layer = 1; layer < nh; ++layer) {
            w = image + image_offset(s, layer, 0, 0, lane);
#pragma unroll
            for (int c = 0; c < kColTiles; ++c) {
                pack_hidden<MB>(acc[c], hb[c]);
#pragma unroll
                for (int m = 0; m < MB; ++m) acc[c][m] = zero16();
            }
#pragma unroll
            for (int m = 0; m < MB; ++m)
#pragma unroll
                for (int t = 0; t < KW; ++t) {
                    const bf16x8 a = as_frag(*reinterpret_cast<const uint4*>(w + (size_t)frag_in_layer(KW, m, t) * kFragBytes));
#pragma unroll
                    for (int c = 0; c < kColTiles; ++c) acc[c][m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[c][t], acc[c][m], 0, 0, 0);
                }
        }
        // ---- the output layer: one row block, rows beyond n_out are zero in the image -----------------------------------------------
        w = image + image_offset(s, nh, 0, 0, lane);
        f32x16 o[kColTiles];
#pragma unroll
        for (int c = 0; c < kColTiles; ++c) {
            pack_hidden<MB>(acc[c], hb[c]);
            o[c] = zero16();
        }
#pragma unroll
        for (int t = 0; t < KW; ++t) {
            const bf16x8 a = as_frag(*reinterpret_cast<const uint4*>(w + (size_t)frag_in_layer(KW, 0, t) * kFragBytes));
#pragma unroll
            for (int c = 0; c < kColTiles; ++c) o[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, hb[c][t], o[c], 0, 0, 0);
        }
#pragma unroll
        for (int c = 0; c < kColTiles; ++c) {
            float* dst = out + pixel[c] * (uint64_t)n_out;
#pragma unroll
            for (int reg = 0; reg < 8; ++reg) {   // registers 0 .. 7 hold rows 0 .. 15
                const int orow = mlp_out_row(reg, h);
                float y = o[c][reg];
                if (activation == GRUT_MLP_ACT_RELU) y = fmaxf(y, 0.f);
                if (activation == GRUT_MLP_ACT_SIGMOID) y = 1.f / (1.f + __expf(-y));
                if (unpremultiply) y = y * a_s[c];
                if (pixel[c] < P && orow < n_out) dst[orow] = y;
            }
        }
    }
}

template <int WIDTH, bool DECODE>
int launch(hipStream_t stream, const Shape& s, const GrutMlpConfig* c, const float* params, const float* input, uint32_t P, float* out,
           const DecodeArgs& da) {
    int dev = 0, cus = 0;
    GRUT_HIP(hipGetDevice(&dev));
    GRUT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint32_t bytes = lds_bytes(s);
    const uint32_t steps = (uint32_t)(((uint64_t)P + kColTiles * kTile - 1) / (kColTiles * kTile));
    const uint32_t need = (steps + kWavesPerBlock - 1) / kWavesPerBlock;
    const uint32_t grid = need < (uint32_t)(cus > 0 ? cus : 1) ? need : (uint32_t)(cus > 0 ? cus : 1);
    if constexpr (DECODE) {
        if (bytes > 64u * 1024u)
            GRUT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_forward_kernel<WIDTH, true, DecodeArgs>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        mlp_forward_kernel<WIDTH, true, DecodeArgs><<<grid, kBlock, bytes, stream>>>(s, c->n_output_dims, c->output_activation, params, input, P, out, da);
    } else {
        if (bytes > 64u * 1024u)
            GRUT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mlp_forward_kernel<WIDTH, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)bytes));
        mlp_forward_kernel<WIDTH, false><<<grid, kBlock, bytes, stream>>>(s, c->n_output_dims, c->output_activation, params, input, P, out);
    }
    GRUT_HIP(hipGetLastError());
    return GRUT_OK;
}

}  // namespace
}  // namespace grut

using namespace grut;

extern "C" uint32_t grut_mlp_num_params(const GrutMlpConfig* config) {
    Shape s;
    return shape_of(config, &s) ? num_params(s) : 0u;
}

extern "C" uint32_t grut_mlp_lds_bytes(const GrutMlpConfig* config) {
    Shape s;
    return shape_of(config, &s) ? lds_bytes(s) : 0u;
}

extern "C" int grut_mlp_forward(void* stream, const GrutMlpConfig* config, const float* params, const float* input, uint32_t P, float* out) {
    Shape s;
    GRUT_REQUIRE(shape_of(config, &s), "grut_mlp_forward: width must be 64 or 128, sh_degree 1..4, n_hidden_layers >= 1, the padded encoded "
                                       "width at most 128, n_output_dims 1..16 and the activation one of GRUT_MLP_ACT_*");
    GRUT_REQUIRE(lds_bytes(s) != 0, "grut_mlp_forward: the weight image of this configuration does not fit into LDS (grut_mlp_lds_bytes)");
    GRUT_REQUIRE(P > 0 && params && input && out, "grut_mlp_forward: num_pixels > 0, params, input and out are required");
    GRUT_REQUIRE(((uintptr_t)params & 15u) == 0, "grut_mlp_forward: params must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    return s.width == 64 ? launch<64, false>(st, s, config, params, input, P, out, DecodeArgs{}) : launch<128, false>(st, s, config, params, input, P, out, DecodeArgs{});
}

extern "C" int grut_decode_forward(void* stream, const GrutDecodeConfig* config, const float* params, const float* features, const float* alpha,
                                   const float* rays_dir, const float* rot, uint32_t num_views, uint32_t pixels_per_view, float* out) {
    Shape s;
    DecodeArgs da;
    uint32_t P = 0;
    if (!decode_args_of("grut_decode_forward", config, alpha, rays_dir, rot, num_views, pixels_per_view, &da, &P)) return GRUT_ERR_BAD_INPUT;
    GRUT_REQUIRE(shape_of(&config->mlp, &s), "grut_decode_forward: width must be 64 or 128, sh_degree 1..4, n_hidden_layers >= 1, the padded encoded "
                                             "width at most 128, n_output_dims 1..16 and the activation one of GRUT_MLP_ACT_*");
    GRUT_REQUIRE(lds_bytes(s) != 0, "grut_decode_forward: the weight image of this configuration does not fit into LDS (grut_mlp_lds_bytes)");
    GRUT_REQUIRE(params && out && (features || s.n_features == 0), "grut_decode_forward: params, features and out are required");
    GRUT_REQUIRE(((uintptr_t)params & 15u) == 0, "grut_decode_forward: params must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    return s.width == 64 ? launch<64, true>(st, s, &config->mlp, params, features, P, out, da)
                         : launch<128, true>(st, s, &config->mlp, params, features, P, out, da);
}
