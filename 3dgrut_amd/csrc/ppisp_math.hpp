// ppisp_math.hpp — the per-pixel camera model of csrc/ppisp.hip and its parameter chain rules, as plain fp32 C++ that the device
// kernels inline and a host compiler accepts unchanged (the formulas can then be checked against a float64 restatement without a GPU).
//
// Stages, in order: exposure x = rgb 2^e; per-channel radial vignetting x_c *= clamp(1 + a1 r2 + a2 r2^2 + a3 r2^3, 0, 1);
// colour homography on (r, g, r+g+b) with intensity renormalisation; per-channel response curve (toe / shoulder power pieces meeting at
// `centre`, then a gamma).  A stage whose bit is missing from Prep::stages is the identity.
//
// Gradient conventions at the kinks (part of the contract, include/grut_amd.h):
//   vignetting clamp   the five parameters receive gradient where 0 <= p <= 1, INCLUSIVE (every alpha starts at 0, i.e. p == 1 exactly)
//   response curve     a channel whose curve input is <= 0 or >= 1 passes no gradient, neither to the input nor to its four parameters
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PPISP_HD __host__ __device__ __forceinline__
#else
#define PPISP_HD inline
#endif

namespace grut {
namespace ppisp {

enum : uint32_t { HAS_EXPOSURE = 1u, HAS_COLOR = 2u, HAS_VIGNETTING = 4u, HAS_CRF = 8u };

constexpr float kLn2 = 0.69314718055994531f;
constexpr float kTiny = 1.0e-20f;          // degenerate cross product / homography scale
constexpr float kIntensityEps = 1.0e-5f;
constexpr float kCurveEps = 1.0e-6f;

// Slots of the per-block gradient row, taken against the ACTIVATED quantities (the one-block finish kernel applies the chain rules):
// 0 exposure scale | 1..9 Hm row-major | 10..24 vignetting [c][cx, cy, a1, a2, a3] | 25..39 curve [c][toe, shoulder, gamma, centre, a]
constexpr int kSlotScale = 0, kSlotH = 1, kSlotVig = 10, kSlotCurve = 25, kRow = 48;   // 40 slots, rows padded to 3 x 16
#define PPISP_ACC(acc, i) (acc)[(i) >> 4][(i) & 15]

struct Curve {
    float toe, shoulder, gamma, centre, a, b, inv_centre, inv_rest;   // b = 1 - a, inv_rest = 1 / (1 - centre)
};
struct Prep {
    float scale;                          // 2^e
    float half_w, half_h, inv_extent;     // uv = (pc - (W/2, H/2)) / max(W, H)
    float vig[3][5];
    float H[9];
    Curve crf[3];
    uint32_t stages;
};

PPISP_HD float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }
PPISP_HD float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// ---- colour homography from the 8 latents (blue, red, green, neutral; two each) ----------------------------------------------------
struct Homography {
    float T[3][3], n[3], rp[3], rq[3], lam[3], H0[9], h22;   // rp, rq: the rows p < q of A = skew(n) T whose cross product gave lam
    int p, q;
    bool normalised;
};
// the four symmetric 2x2 maps, as (m00, m01 = m10, m11)
#define PPISP_LATENT_MAPS                                                                        \
    {{0.0480542f, -0.0043631f, 0.0481283f}, {0.0580570f, -0.0179872f, 0.0431061f},               \
     {0.0433336f, -0.0180537f, 0.0580500f}, {0.0128369f, -0.0034654f, 0.0128158f}}

PPISP_HD void cross3(const float* a, const float* b, float* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
PPISP_HD float norm2(const float* a) { return a[0] * a[0] + a[1] * a[1] + a[2] * a[2]; }
PPISP_HD void skew(const float* n, float (&K)[3][3]) {
    K[0][0] = 0.f;   K[0][1] = -n[2]; K[0][2] = n[1];
    K[1][0] = n[2];  K[1][1] = 0.f;   K[1][2] = -n[0];
    K[2][0] = -n[1]; K[2][1] = n[0];  K[2][2] = 0.f;
}

PPISP_HD void homography(const float* L, float* H, Homography& x) {
    const float M[4][3] = PPISP_LATENT_MAPS;
    float o[4][2];
    for (int k = 0; k < 4; ++k) {
        o[k][0] = M[k][0] * L[2 * k] + M[k][1] * L[2 * k + 1];
        o[k][1] = M[k][1] * L[2 * k] + M[k][2] * L[2 * k + 1];
    }
    // columns: the blue, red and green targets; n: the neutral one
    x.T[0][0] = o[0][0];       x.T[1][0] = o[0][1];       x.T[2][0] = 1.f;
    x.T[0][1] = 1.f + o[1][0]; x.T[1][1] = o[1][1];       x.T[2][1] = 1.f;
    x.T[0][2] = o[2][0];       x.T[1][2] = 1.f + o[2][1]; x.T[2][2] = 1.f;
    x.n[0] = 1.f / 3.f + o[3][0]; x.n[1] = 1.f / 3.f + o[3][1]; x.n[2] = 1.f;
    float K[3][3], A[3][3];
    skew(x.n, K);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = K[i][0] * x.T[0][j] + K[i][1] * x.T[1][j] + K[i][2] * x.T[2][j];
    x.p = 0, x.q = 1;
    cross3(A[0], A[1], x.lam);
    if (norm2(x.lam) < kTiny) {
        x.q = 2;
        cross3(A[0], A[2], x.lam);
        if (norm2(x.lam) < kTiny) {
            x.p = 1;
            cross3(A[1], A[2], x.lam);
        }
    }
    for (int j = 0; j < 3; ++j) {
        x.rp[j] = x.p == 0 ? A[0][j] : A[1][j];
        x.rq[j] = x.q == 1 ? A[1][j] : A[2][j];
    }
    // T diag(lam) S with S = [[-1,-1,1],[1,0,0],[0,1,0]]
    for (int i = 0; i < 3; ++i) {
        const float q0 = x.T[i][0] * x.lam[0], q1 = x.T[i][1] * x.lam[1], q2 = x.T[i][2] * x.lam[2];
        x.H0[3 * i + 0] = q1 - q0;
        x.H0[3 * i + 1] = q2 - q0;
        x.H0[3 * i + 2] = q0;
    }
    x.h22 = x.H0[8];
    x.normalised = fabsf(x.h22) > kTiny;
    const float inv = x.normalised ? 1.f / x.h22 : 1.f;
    for (int k = 0; k < 9; ++k) H[k] = x.H0[k] * inv;
}

// gH: dL/dHm (the normalised matrix) -> gL: dL/d latents.  The branch lam took is a constant.
PPISP_HD void homography_backward(const Homography& x, const float* gH, float* gL) {
    const float inv = x.normalised ? 1.f / x.h22 : 1.f;
    float g0[9], s = 0.f;
    for (int k = 0; k < 9; ++k) {
        g0[k] = gH[k] * inv;
        s += gH[k] * (x.H0[k] * inv);   // gH . Hm
    }
    if (x.normalised) g0[8] -= s * inv;
    float gT[3][3], glam[3] = {0.f, 0.f, 0.f};
    for (int i = 0; i < 3; ++i) {
        const float gq[3] = {g0[3 * i + 2] - g0[3 * i + 0] - g0[3 * i + 1], g0[3 * i + 0], g0[3 * i + 1]};   // row i of g0 S^T
        for (int k = 0; k < 3; ++k) {
            gT[i][k] = gq[k] * x.lam[k];
            glam[k] += gq[k] * x.T[i][k];
        }
    }
    float gp[3], gq[3], gA[3][3];
    cross3(x.rq, glam, gp);             // lam = a x b: ga = b x g, gb = g x a
    cross3(glam, x.rp, gq);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) gA[i][j] = i == x.p ? gp[j] : (i == x.q ? gq[j] : 0.f);
    // A = K T with K = skew(n): gT += K^T gA, gK = gA T^T
    float K[3][3], gK[3][3];
    skew(x.n, K);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            gT[i][j] += K[0][i] * gA[0][j] + K[1][i] * gA[1][j] + K[2][i] * gA[2][j];
            gK[i][j] = gA[i][0] * x.T[j][0] + gA[i][1] * x.T[j][1] + gA[i][2] * x.T[j][2];
        }
    const float go[4][2] = {{gT[0][0], gT[1][0]}, {gT[0][1], gT[1][1]}, {gT[0][2], gT[1][2]},
                            {gK[2][1] - gK[1][2], gK[0][2] - gK[2][0]}};
    const float M[4][3] = PPISP_LATENT_MAPS;
    for (int k = 0; k < 4; ++k) {
        gL[2 * k] = M[k][0] * go[k][0] + M[k][1] * go[k][1];
        gL[2 * k + 1] = M[k][1] * go[k][0] + M[k][2] * go[k][1];
    }
}

// ---- response curve's activated parameters from its four raw ones --------------------------------------------------------------------
PPISP_HD Curve make_curve(const float* raw) {
    Curve c;
    c.toe = 0.3f + softplus(raw[0]);
    c.shoulder = 0.3f + softplus(raw[1]);
    c.gamma = 0.1f + softplus(raw[2]);
    c.centre = fminf(fmaxf(sigmoid(raw[3]), kCurveEps), 1.f - kCurveEps);
    const float l = fmaxf((c.shoulder - c.toe) * c.centre + c.toe, kCurveEps);
    c.a = c.shoulder * c.centre / l;
    c.b = 1.f - c.a;
    c.inv_centre = 1.f / c.centre;
    c.inv_rest = 1.f / (1.f - c.centre);
    return c;
}
// g: gradients against (toe, shoulder, gamma, centre, a) -> graw[4]
PPISP_HD void curve_backward(const float* raw, const float* g, float* graw) {
    const Curve c = make_curve(raw);
    // a = shoulder centre / l with l = (shoulder - toe) centre + toe: a convex combination of two values >= 0.3, so its floor never binds
    const float il = 1.f / ((c.shoulder - c.toe) * c.centre + c.toe), a_l = c.a * il, ga = g[4];   // da/dl = -a / l
    const float gtoe = g[0] - ga * a_l * (1.f - c.centre);                                          // dl/dtoe = 1 - centre
    const float gsh = g[1] + ga * (c.centre * il - a_l * c.centre);                                 // dl/dshoulder = centre
    const float gcen = g[3] + ga * (c.shoulder * il - a_l * (c.shoulder - c.toe));
    const float sg = sigmoid(raw[3]);
    graw[0] = gtoe * sigmoid(raw[0]);       // d softplus = sigmoid
    graw[1] = gsh * sigmoid(raw[1]);
    graw[2] = g[2] * sigmoid(raw[2]);
    graw[3] = (sg >= kCurveEps && sg <= 1.f - kCurveEps) ? gcen * sg * (1.f - sg) : 0.f;
}

// ---- the block's prologue: every wave-uniform quantity, once ---------------------------------------------------------------------------
PPISP_HD void prepare(Prep& p, float res_w, float res_h, const float* exposure, const float* color, const float* vignetting, const float* crf) {
    p.stages = (exposure ? HAS_EXPOSURE : 0u) | (color ? HAS_COLOR : 0u) | (vignetting ? HAS_VIGNETTING : 0u) | (crf ? HAS_CRF : 0u);
    p.scale = exposure ? exp2f(exposure[0]) : 1.f;
    p.half_w = 0.5f * res_w;
    p.half_h = 0.5f * res_h;
    p.inv_extent = 1.f / fmaxf(res_w, res_h);
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 5; ++k) p.vig[c][k] = vignetting ? vignetting[5 * c + k] : 0.f;
    if (color) {
        Homography x;
        homography(color, p.H, x);
    } else {
        for (int k = 0; k < 9; ++k) p.H[k] = (k % 4 == 0) ? 1.f : 0.f;
    }
    const float zeros[4] = {0.f, 0.f, 0.f, 0.f};   // stage off: the curve is never evaluated, the fields only need values
    for (int c = 0; c < 3; ++c) p.crf[c] = make_curve(crf ? crf + 4 * c : zeros);
}

// ---- one pixel ---------------------------------------------------------------------------------------------------------------------------
// in: rgb; (px, py): pixel_coords (unused without the vignetting stage).  out: the processed colour.
// BWD: go = dL/dout -> gin = dL/drgb, and the parameter gradients are ADDED to acc (slots above).
template <bool BWD>
PPISP_HD void pixel(const Prep& P, const float* in, float px, float py, float* out, const float* go, float* gin, float (&acc)[3][16]) {
    const bool has_vig = P.stages & HAS_VIGNETTING, has_color = P.stages & HAS_COLOR, has_crf = P.stages & HAS_CRF;
    float x[3], f[3] = {1.f, 1.f, 1.f}, dx[3], dy[3], r2[3];
    bool pass[3] = {false, false, false};
    // exposure, vignetting
    if (has_vig) {
        const float u = (px - P.half_w) * P.inv_extent, v = (py - P.half_h) * P.inv_extent;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dx[c] = u - P.vig[c][0];
            dy[c] = v - P.vig[c][1];
            r2[c] = dx[c] * dx[c] + dy[c] * dy[c];
            const float r4 = r2[c] * r2[c];
            const float p = 1.f + P.vig[c][2] * r2[c] + P.vig[c][3] * r4 + P.vig[c][4] * (r4 * r2[c]);
            pass[c] = p >= 0.f && p <= 1.f;
            f[c] = fminf(fmaxf(p, 0.f), 1.f);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = in[c] * P.scale * f[c];
    // colour
    float z[3] = {x[0], x[1], x[2]}, v[3], I = 0.f, inv_den = 0.f, s = 0.f;
    if (has_color) {
        I = x[0] + x[1] + x[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) v[i] = P.H[3 * i] * x[0] + P.H[3 * i + 1] * x[1] + P.H[3 * i + 2] * I;
        const float den = v[2] + kIntensityEps;
        s = I / den;
        if (BWD) inv_den = 1.f / den;
        z[0] = s * v[0];
        z[1] = s * v[1];
        z[2] = s * v[2] - z[0] - z[1];
    }
    // response curve; its gradient to the input lands in gz
    float gz[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (!has_crf) {
            out[c] = z[c];
            if (BWD) gz[c] = go[c];
            continue;
        }
        const Curve& k = P.crf[c];
        const float zc = fminf(fmaxf(z[c], 0.f), 1.f);
        const bool lo = zc <= k.centre;
        const float w = lo ? zc : 1.f - zc;
        const float t = w * (lo ? k.inv_centre : k.inv_rest);
        const float e = lo ? k.toe : k.shoulder;
        const float lg = log2f(t), pw = exp2f(e * lg);   // t^e; t = 0 gives exp2(-inf) = 0
        const float y = lo ? k.a * pw : 1.f - k.b * pw;
        const float ym = fmaxf(y, 0.f), lgy = log2f(ym);
        const float o = exp2f(k.gamma * lgy);
        out[c] = o;
        if (BWD) {
            const bool active = z[c] > 0.f && z[c] < 1.f && y > 0.f;
            const float g = go[c];
            const float gy = g * k.gamma * o / y;
            const float common = gy * (lo ? k.a : k.b) * pw;        // |dy/dpw| weighted; dy/dt has the same sign in both pieces
            const float tl = common * lg * kLn2;
            const int s0 = kSlotCurve + 5 * c;
            PPISP_ACC(acc, s0 + 0) += (active && lo) ? tl : 0.f;    // toe: y = a t^toe
            PPISP_ACC(acc, s0 + 1) += (active && !lo) ? -tl : 0.f;  // shoulder: y = 1 - b t^shoulder
            PPISP_ACC(acc, s0 + 2) += active ? g * o * lgy * kLn2 : 0.f;
            PPISP_ACC(acc, s0 + 3) += active ? -common * e * (lo ? k.inv_centre : k.inv_rest) : 0.f;   // through t's denominator
            PPISP_ACC(acc, s0 + 4) += active ? gy * pw : 0.f;       // a (b = 1 - a): dy/da = t^e in both pieces
            gz[c] = active ? common * e / w : 0.f;
        }
    }
    if (!BWD) return;
    // colour, backwards
    float gx[3] = {gz[0], gz[1], gz[2]};
    if (has_color) {
        const float h[3] = {gz[0] - gz[2], gz[1] - gz[2], gz[2]};   // against s v
        const float gs = h[0] * v[0] + h[1] * v[1] + h[2] * v[2];
        float gv[3] = {s * h[0], s * h[1], s * h[2] - gs * s * inv_den};
        const float gI = gs * inv_den;
        const float u3[3] = {x[0], x[1], I};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) PPISP_ACC(acc, kSlotH + 3 * i + j) += gv[i] * u3[j];
        const float gu2 = P.H[2] * gv[0] + P.H[5] * gv[1] + P.H[8] * gv[2] + gI;
        gx[0] = P.H[0] * gv[0] + P.H[3] * gv[1] + P.H[6] * gv[2] + gu2;
        gx[1] = P.H[1] * gv[0] + P.H[4] * gv[1] + P.H[7] * gv[2] + gu2;
        gx[2] = gu2;
    }
    // vignetting and exposure, backwards
    float gscale = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float xe = in[c] * P.scale;   // before the falloff
        if (has_vig) {
            const float gp = pass[c] ? gx[c] * xe : 0.f;
            const float r4 = r2[c] * r2[c];
            const float gr2 = gp * (P.vig[c][2] + 2.f * P.vig[c][3] * r2[c] + 3.f * P.vig[c][4] * r4);
            const int s0 = kSlotVig + 5 * c;
            PPISP_ACC(acc, s0 + 0) += -2.f * gr2 * dx[c];
            PPISP_ACC(acc, s0 + 1) += -2.f * gr2 * dy[c];
            PPISP_ACC(acc, s0 + 2) += gp * r2[c];
            PPISP_ACC(acc, s0 + 3) += gp * r4;
            PPISP_ACC(acc, s0 + 4) += gp * (r4 * r2[c]);
        }
        const float ge = gx[c] * f[c];
        gscale += ge * in[c];
        gin[c] = ge * P.scale;
    }
    PPISP_ACC(acc, kSlotScale) += gscale;
}

// ---- the finish: one summed row against the activated quantities -> gradients of the raw parameter rows ----------------------------------
// Any output pointer may be null (its stage is absent or its gradient is not wanted).
PPISP_HD void finish(const float* row, const float* exposure, const float* color, const float* crf, float* g_exposure, float* g_color,
                     float* g_vignetting, float* g_crf) {
    if (g_exposure) g_exposure[0] = row[kSlotScale] * exp2f(exposure[0]) * kLn2;
    if (g_color) {
        Homography x;
        float H[9];
        homography(color, H, x);
        homography_backward(x, row + kSlotH, g_color);
    }
    if (g_vignetting)
        for (int k = 0; k < 15; ++k) g_vignetting[k] = row[kSlotVig + k];
    if (g_crf)
        for (int c = 0; c < 3; ++c) curve_backward(crf + 4 * c, row + kSlotCurve + 5 * c, g_crf + 4 * c);
}

}  // namespace ppisp
}  // namespace grut
