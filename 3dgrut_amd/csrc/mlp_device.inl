// mlp_device.inl — what the decoder MLP's forward (mlp.hip) and backward (mlp_backward.hip) share on the device: the fragment types, the
// bf16 pack, the SH polynomials, the decode stage's direction and the first layer's encoded-input fragment.  Included inside namespace grut's anonymous namespace, after
// common.hpp and mlp_layout.hpp.

using namespace grut_mlp;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// two floats -> two bf16 (round to nearest even), low half first
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ bf16x8 as_frag(uint4 v) { return __builtin_bit_cast(bf16x8, v); }

// the 16 real SH polynomials of the contract for d = (x, y, z)
__device__ __forceinline__ f32x16 sh_values(float x, float y, float z) {
    const float xx = x * x, yy = y * y, zz = z * z;
    f32x16 sh;
    sh[0] = 0.28209479177387814f;
    sh[1] = -0.48860251190291987f * y;
    sh[2] = 0.48860251190291987f * z;
    sh[3] = -0.48860251190291987f * x;
    sh[4] = 1.0925484305920792f * (x * y);
    sh[5] = -1.0925484305920792f * (y * z);
    sh[6] = 0.94617469575755997f * zz - 0.31539156525251999f;
    sh[7] = -1.0925484305920792f * (x * z);
    sh[8] = 0.54627421529603959f * (xx - yy);
    sh[9] = 0.59004358992664352f * (y * (-3.f * xx + yy));
    sh[10] = 2.8906114426405538f * (x * y * z);
    sh[11] = 0.45704579946446572f * (y * (1.f - 5.f * zz));
    sh[12] = 0.3731763325901154f * (z * (5.f * zz - 3.f));
    sh[13] = 0.45704579946446572f * (x * (1.f - 5.f * zz));
    sh[14] = 1.4453057213202769f * (z * (xx - yy));
    sh[15] = 0.59004358992664352f * (x * (-xx + 3.f * yy));
    return sh;
}

// element e (mlp_input_element) of a pixel, e wave-uniform: an SH value or a one (a feature column gives an unused value)
__device__ __forceinline__ float sh_or_one(int e, const f32x16& sh) {
    const int i = -1 - e;                                  // the SH index; negative for a feature, huge for a one
    float v = sh[__builtin_amdgcn_readfirstlane((i < 0 ? 0 : i) & 15)];   // a register picked by a SCALAR index: no lane ever differs
    asm volatile("" : "+v"(v));                            // (keeps the pick from being merged with the other half's into a per-lane index)
    return e == kInputOne ? 1.f : v;
}

// ---- the decode stage (grut_decode_forward / grut_decode_backward): where a pixel's direction and alpha come from ---------------------------
struct DecodeArgs {
    const float* alpha;          // [P]; read only with unpremultiply
    const float* rays;           // [P, 3] camera space; not read with center_ray
    const float* rot;            // [B, 9] row-major camera-to-world rotations
    uint32_t pixels_per_view;
    float sh_scale;
    int unpremultiply, center_ray;
};

// the kernels' trailing arguments: none for the rows [P, F + 3]; for the decode stage one DecodeArgs and, in the backward, grad_alpha
__device__ __forceinline__ DecodeArgs decode_args() { return DecodeArgs{}; }
__device__ __forceinline__ DecodeArgs decode_args(const DecodeArgs& a, float* = nullptr) { return a; }
__device__ __forceinline__ float* decode_grad_alpha() { return nullptr; }
__device__ __forceinline__ float* decode_grad_alpha(const DecodeArgs&, float* grad_alpha) { return grad_alpha; }

// What decode_direction reads of pixel `pixel` (< P: a tail lane passes the last pixel): the rotation of its view (per lane: a tile may
// straddle two views) and, unless center_ray, its camera ray.  Apart from the arithmetic, so that the forward can issue these loads one
// step ahead.
struct DirectionInput {
    float R[9], c[3];
};
__device__ __forceinline__ DirectionInput decode_direction_load(const DecodeArgs& a, uint32_t pixel) {
    DirectionInput in;
    const float* R = a.rot + (size_t)(pixel / a.pixels_per_view) * 9;
#pragma unroll
    for (int i = 0; i < 9; ++i) in.R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) in.c[i] = a.center_ray ? 0.f : a.rays[(size_t)pixel * 3 + i];   // (uniform)
    return in;
}

// d = 2 u - 1: u = (n sh_scale + 1) 0.5, n = w / max(|w|, 1e-12), w = R_b d_cam or, with center_ray, column 2 of R_b.  ONE function for the
// forward and the backward's recomputation.  sqrtf and / are the correctly rounded IEEE operations (hipcc's default,
// -fhip-fp32-correctly-rounded-divide-sqrt): no reciprocal anywhere.
__device__ __forceinline__ void decode_direction(const DecodeArgs& a, const DirectionInput& in, float (&d)[3]) {
    float w[3];
    if (a.center_ray) {   // (uniform)
        w[0] = in.R[2], w[1] = in.R[5], w[2] = in.R[8];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = in.R[3 * i] * in.c[0] + in.R[3 * i + 1] * in.c[1] + in.R[3 * i + 2] * in.c[2];
    }
    const float len = fmaxf(sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), 1e-12f);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float u = ((w[i] / len) * a.sh_scale + 1.f) * 0.5f;
        d[i] = 2.f * u - 1.f;
    }
}

// the B fragment of k-step t of the first layer: 8 elements of this lane's pixel, in the order of mlp_input_element.  Which kind of
// element j is depends on the lane half only, so both halves' kinds are wave-uniform and the lane picks its own by h.
// DECODE: `row` is the pixel's F feature columns alone, and with `unpremultiply` (uniform) a feature column is row[e] / a_s, an IEEE division.
template <bool DECODE = false>
__device__ __forceinline__ bf16x8 encode_step(const Shape& s, int t, int h, const float* __restrict__ row, const f32x16& sh,
                                              bool unpremultiply = false, float a_s = 1.f) {
    float v[8];
    if (kStep * (t + 1) <= s.n_features) {   // (wave-uniform) all 16 elements are feature columns
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row[mlp_input_element(s, t, h, j)];
        if (DECODE && unpremultiply) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = v[j] / a_s;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e0 = mlp_input_element(s, t, 0, j), e1 = mlp_input_element(s, t, 1, j), e = h ? e1 : e0;
            const float other = h ? sh_or_one(e1, sh) : sh_or_one(e0, sh);
            float feature = DECODE && s.n_features == 0 ? 0.f : row[e > 0 ? e : 0];   // (no feature column at all: nothing to read)
            if (DECODE && unpremultiply) feature = feature / a_s;
            v[j] = e >= 0 ? feature : other;
        }
    }
    return as_frag(make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])));
}

// a layer's result -> the next layer's operand: ReLU, then registers 8 s .. 8 s + 7 of row block b become k-step 2 b + s
template <int MB>
__device__ __forceinline__ void pack_hidden(const f32x16 (&acc)[MB], bf16x8 (&hb)[2 * MB]) {
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) w[q] = pack_bf16(fmaxf(acc[b][8 * sub + 2 * q], 0.f), fmaxf(acc[b][8 * sub + 2 * q + 1], 0.f));
            hb[2 * b + sub] = as_frag(make_uint4(w[0], w[1], w[2], w[3]));
        }
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    return z;
}

// the weight image, from the live fp32 parameters, by the whole workgroup of `block` threads (the caller synchronises)
__device__ __forceinline__ void build_image(const Shape& s, int n_out, const float* __restrict__ params, unsigned char* image, int block) {
    const uint32_t chunks = num_frags(s) * 64u;
    for (uint32_t c = threadIdx.x; c < chunks; c += block) {
        uint32_t src = 0;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (image_chunk_source(s, n_out, c, &src)) {
            const float4 a = *reinterpret_cast<const float4*>(params + src), b = *reinterpret_cast<const float4*>(params + src + 8);
            v = make_uint4(pack_bf16(a.x, a.y), pack_bf16(a.z, a.w), pack_bf16(b.x, b.y), pack_bf16(b.z, b.w));
        }
        *reinterpret_cast<uint4*>(image + (size_t)c * 16u) = v;
    }
}

// the layout's integers of a configuration; false for one that neither kernel takes
inline bool shape_of(const GrutMlpConfig* c, Shape* s) {
    if (!c) return false;
    *s = Shape{c->n_features, c->sh_degree, c->n_hidden_layers, c->width};
    return shape_ok(*s) && c->n_output_dims >= 1 && c->n_output_dims <= kOutRows && c->output_activation >= GRUT_MLP_ACT_NONE &&
           c->output_activation <= GRUT_MLP_ACT_SIGMOID;
}

// the checks that grut_decode_forward and grut_decode_backward share, and their kernel arguments; P = num_views * pixels_per_view
inline bool decode_args_of(const char* who, const GrutDecodeConfig* c, const float* alpha, const float* rays_dir, const float* rot,
                           uint32_t num_views, uint32_t pixels_per_view, DecodeArgs* da, uint32_t* P) {
    if (!c || !rot || num_views == 0 || pixels_per_view == 0 || (uint64_t)num_views * pixels_per_view > 0xffffffffull) {
        set_last_error("%s: config, rot, num_views > 0, pixels_per_view > 0 and num_views * pixels_per_view < 2^32 are required", who);
        return false;
    }
    if (c->unpremultiply_alpha && !alpha) {
        set_last_error("%s: unpremultiply_alpha needs alpha", who);
        return false;
    }
    if (!c->center_ray && !rays_dir) {
        set_last_error("%s: rays_dir may be NULL only with center_ray", who);
        return false;
    }
    *da = DecodeArgs{alpha, rays_dir, rot, pixels_per_view, c->sh_scale, c->unpremultiply_alpha != 0, c->center_ray != 0};
    *P = num_views * pixels_per_view;
    return true;
}
