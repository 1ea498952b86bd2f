// mlp_device.inl — what the decoder MLP's forward (mlp.hip) and backward (mlp_backward.hip) share on the device: the fragment types, the
// bf16 pack, the SH polynomials and the first layer's encoded-input fragment.  Included inside namespace grut's anonymous namespace, after
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

// the B fragment of k-step t of the first layer: 8 elements of this lane's pixel, in the order of mlp_input_element.  Which kind of
// element j is depends on the lane half only, so both halves' kinds are wave-uniform and the lane picks its own by h.
__device__ __forceinline__ bf16x8 encode_step(const Shape& s, int t, int h, const float* __restrict__ row, const f32x16& sh) {
    float v[8];
    if (kStep * (t + 1) <= s.n_features) {   // (wave-uniform) all 16 elements are feature columns
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = row[mlp_input_element(s, t, h, j)];
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e0 = mlp_input_element(s, t, 0, j), e1 = mlp_input_element(s, t, 1, j), e = h ? e1 : e0;
            const float other = h ? sh_or_one(e1, sh) : sh_or_one(e0, sh);
            const float feature = row[e > 0 ? e : 0];
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
