// The BatchNorm element math, written ONCE: the forward affine and the ReLU-mask rule built on it, x-hat, the backward
// expression, their lane-wise forms over a float4 (4 consecutive channels) and the sp passes' 8-channel chunk forms.  Every
// kernel that normalises, masks a gradient or forms dy - bn.hip's passes, the BatchNorm reduce that rides on the backward-data
// epilogue (bf16_tile.h), the operand-forming conv loaders (conv_split.hip) - calls these, so the forward pass and every
// backward pass take the SAME bit decision for the mask.
#pragma once
#include <hip/hip_runtime.h>

namespace mvg {

// ---- scalar definitions -----------------------------------------------------------------------------------------
// An explicit fma: the mask must not depend on the compiler's contraction setting.
__device__ __forceinline__ float bn_fwd(float y, float scale, float shift) { return __builtin_fmaf(y, scale, shift); }
// The ReLU mask without the activation: out > 0 <=> bn_fwd(y, scale, shift) > 0 (no residual on that unit).
__device__ __forceinline__ bool relu_on(float y, float scale, float shift) { return bn_fwd(y, scale, shift) > 0.f; }
__device__ __forceinline__ float relu_mask(bool on, float d) { return on ? d : 0.f; }
// Eval mode: one channel's (scale, shift) from the running statistics.  bn_eval_affine_kernel and its batched form
// (bn_eval_affine_batch_kernel: every BatchNorm of a network in one launch) both call this, so they leave the same bits.
__device__ __forceinline__ void bn_eval_affine_ch(float gamma, float beta, float rm, float rv, float eps, float &scale, float &shift) {
  const float sc = gamma / sqrtf(rv + eps);
  scale = sc;
  shift = beta - rm * sc;
}
__device__ __forceinline__ float xhat(float y, float mean, float invstd) { return (y - mean) * invstd; }
// dy = gamma invstd (dz - s1/n - x-hat s2/n).  The association is part of the definition: the build contracts
// multiply-adds, and the shape of this expression decides which ones.
__device__ __forceinline__ float bn_dy(float dz, float y, float mean, float invstd, float gamma, float s1, float s2, float inv_rows) {
  return gamma * invstd * (dz - s1 * inv_rows - (y - mean) * invstd * (s2 * inv_rows));
}

// ---- lane-wise application over a float4 ---------------------------------------------------------------------------
// map4(f, a, b, ...) = (f(a.x, b.x, ...), ..., f(a.w, b.w, ...)); an argument that is not a float4 goes to all four lanes.
template <int K>
__device__ __forceinline__ float lane(const float4 &v) { return K == 0 ? v.x : K == 1 ? v.y : K == 2 ? v.z : v.w; }
template <int K>
__device__ __forceinline__ unsigned lane(const uchar4 &v) { return K == 0 ? v.x : K == 1 ? v.y : K == 2 ? v.z : v.w; }
template <int K, typename S>
__device__ __forceinline__ S lane(const S &s) { return s; }
template <typename F, typename... A>
__device__ __forceinline__ float4 map4(F f, const A &...a) {
  return make_float4(f(lane<0>(a)...), f(lane<1>(a)...), f(lane<2>(a)...), f(lane<3>(a)...));
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 bn_fwd(float4 y, float4 scale, float4 shift) {
  return map4([](float y, float a, float b) { return bn_fwd(y, a, b); }, y, scale, shift);
}
__device__ __forceinline__ float4 bn_relu4(float4 y, float4 scale, float4 shift) {
  return map4([](float y, float a, float b) { return fmaxf(bn_fwd(y, a, b), 0.f); }, y, scale, shift);
}
__device__ __forceinline__ float4 relu4(float4 v) { return map4([](float v) { return fmaxf(v, 0.f); }, v); }
__device__ __forceinline__ float4 abs4(float4 v) { return map4([](float v) { return fabsf(v); }, v); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return map4([](float a, float b) { return a + b; }, a, b); }
__device__ __forceinline__ float4 mul4(float4 a, float k) { return map4([](float a, float k) { return a * k; }, a, k); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return map4([](float a, float b) { return a * b; }, a, b); }
// bit k of the nibble = (lane k came out > 0)
__device__ __forceinline__ unsigned relu_nibble(float4 o) {
  return (o.x > 0.f ? 1u : 0u) | (o.y > 0.f ? 2u : 0u) | (o.z > 0.f ? 4u : 0u) | (o.w > 0.f ? 8u : 0u);
}

// The ReLU mask applied to a gradient, three ways: from the nibble bn_apply recorded, from the activation, from y.
__device__ __forceinline__ float4 mask_bits4(float4 d, unsigned m4) {
  return make_float4(relu_mask(m4 & 1u, d.x), relu_mask(m4 & 2u, d.y), relu_mask(m4 & 4u, d.z), relu_mask(m4 & 8u, d.w));
}
__device__ __forceinline__ float4 mask_act4(float4 d, float4 act) {
  return map4([](float d, float a) { return relu_mask(a > 0.f, d); }, d, act);
}
__device__ __forceinline__ float4 mask_affine4(float4 d, float4 y, float4 scale, float4 shift) {
  return map4([](float d, float y, float a, float b) { return relu_mask(relu_on(y, a, b), d); }, d, y, scale, shift);
}

__device__ __forceinline__ void acc4(float4 &s, float4 d) { s = add4(s, d); }
__device__ __forceinline__ void max4(float4 &m, float4 d) { m = map4([](float m, float d) { return fmaxf(m, d); }, m, d); }
// s2 += dz * x-hat (the += on the product: one fma)
__device__ __forceinline__ void acc4_xhat(float4 &s, float4 d, float4 y, float4 mean, float4 invstd) {
  s = map4([](float s, float d, float y, float mu, float is) { return s += d * xhat(y, mu, is); }, s, d, y, mean, invstd);
}
__device__ __forceinline__ float4 bn_dy(float4 dz, float4 y, float4 mean, float4 invstd, float4 gamma, float4 s1, float4 s2, float inv_rows) {
  return map4([](auto... s) { return bn_dy(s...); }, dz, y, mean, invstd, gamma, s1, s2, inv_rows);
}

// ---- one 8-channel chunk: bn.hip's sp passes and the operand-forming loaders of conv_split.hip ------------------------
// The apply pass: o = [relu](bn_fwd(y, sc, sh) + residual) * osc, the residual (has_res) being r through its own affine
// (res_affine: bn_fwd(r, rs, rh)), r times rsi (res_scaled: an sp identity and its 2^-k) or r as it is.  Returns the ReLU
// mask as two bytes, low nibbles: one byte per 4 channels (bn_bwd_reduce_bits), taken from the unscaled value.
__device__ __forceinline__ unsigned bn_apply_chunk(const float (&y)[8], const float (&sc)[8], const float (&sh)[8], bool has_res,
                                                   const float (&r)[8], bool res_affine, const float (&rs)[8], const float (&rh)[8],
                                                   bool res_scaled, float rsi, bool relu, float osc, float (&o)[8]) {
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float x = bn_fwd(y[k], sc[k], sh[k]);                    // as bn_apply_kernel (mask rebuild in the backward)
    if (has_res) x += res_affine ? bn_fwd(r[k], rs[k], rh[k]) : (res_scaled ? r[k] * rsi : r[k]);
    if (relu) x = fmaxf(x, 0.f);
    m |= (x > 0.f ? 1u : 0u) << (k + (k >= 4 ? 4 : 0));
    o[k] = x * osc;                                          // after the mask decision
  }
  return m;
}
// The backward apply pass: o = bn_dy(dz, y, ...) * dsc; masked: dz first goes through the unit's ReLU mask, rebuilt from y (ms, mh)
__device__ __forceinline__ void bn_dy_chunk(const float (&dz)[8], const float (&y)[8], const float (&mean)[8], const float (&invstd)[8],
                                            const float (&gamma)[8], const float (&s1)[8], const float (&s2)[8], float inv_rows, float dsc,
                                            float (&o)[8], bool masked, const float (&ms)[8], const float (&mh)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float d = dz[k];
    if (masked) d = relu_mask(relu_on(y[k], ms[k], mh[k]), d);
    o[k] = bn_dy(d, y[k], mean[k], invstd[k], gamma[k], s1[k], s2[k], inv_rows) * dsc;
  }
}
// The backward apply pass of a unit on the running statistics (frozen BatchNorm): o = (gamma invstd) dz * dsc - no batch sums.
// f = gamma * invstd per channel, rounded once; masked as above.
__device__ __forceinline__ void bn_frozen_dy_chunk(const float (&dz)[8], const float (&y)[8], const float (&f)[8], float dsc, float (&o)[8],
                                                   bool masked, const float (&ms)[8], const float (&mh)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float d = dz[k];
    if (masked) d = relu_mask(relu_on(y[k], ms[k], mh[k]), d);
    o[k] = f[k] * d * dsc;
  }
}

}  // namespace mvg
