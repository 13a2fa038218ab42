// policy_common.h - what the policy kernels share (included by rollout.hip in front of the other policy_*.h): the Philox4x32-10 block behind every policy's
// random stream and the random-policy harness, the conversions from its words to uniforms and normals, the non-finite bit test, the two forms of the inverse
// action scaling and the 64-lane sum.
// The host forms are d3il_amd/policies.py philox4x32_10, philox_words, uniform24 and box_muller_f64.
#pragma once

namespace d3il {

// Philox4x32-10: key (k0, k1), counter (c0 .. c3) -> four words.  Every stream is key = seed, counter = (lo32, hi32 of env_offset + row, step word, tag): the
// fourth word keeps the streams apart (0: the random-policy harness; BET_TAG, BET_MLP_TAG, DDPM_GPT_TAG, IBC_TAG, ACT_TAG, CVAE_TAG, DDPM_ACT_TAG, BESO_TAG, DDPM_MLP_TAG, BC_GMM_TAG | layout bits: the policies).
__device__ __forceinline__ void philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned* out) {
  const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    unsigned n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3; k0 += W0; k1 += W1;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the block of a policy's stream for the row with global index ge = env_offset + row: key = seed, counter = (lo32, hi32 of ge, step word t, tag)
__device__ __forceinline__ void policy_philox(unsigned long long seed, unsigned long long ge, unsigned t, unsigned tag, unsigned* out) {
  philox4x32_10((unsigned)seed, (unsigned)(seed >> 32), (unsigned)ge, (unsigned)(ge >> 32), t, tag, out);
}
// the upper 24 bits of a word as a uniform in [0, 1 - 2^-24] (exact in f32)
__device__ __forceinline__ float policy_uniform24(unsigned r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }
// two standard normals from two Philox words: u1 in (0, 1], u2 in [0, 1), the precise library functions
__device__ __forceinline__ void policy_box_muller(unsigned ra, unsigned rb, float& n0, float& n1) {
  const float u1 = (float)((ra >> 8) + 1u) * (1.0f / 16777216.0f), u2 = policy_uniform24(rb);
  const float rad = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincosf(6.28318530717958647692f * u2, &s, &c);
  n0 = rad * c; n1 = rad * s;
}
// Exponent field all ones (NaN or +-Inf), read from the bits.  The device pass is built with -ffinite-math-only (build.py): a floating-point isnan / isinf folds
// to false and a select of a NaN constant may be dropped, so every policy kernel tests the integer bit pattern; the empty asm keeps the optimiser from
// looking through the bit cast and folding the test all the same.  Outputs of a hit row are put in with integer selects (0x7FC00000).
__device__ __forceinline__ bool policy_nonfinite(float x) {
  unsigned b = __float_as_uint(x);
  asm("" : "+v"(b));
  return (b & 0x7F800000u) == 0x7F800000u;
}
// The inverse scaling of an action component, clamp(v) scale + shift, in its two forms.  f64: as the reference's f64 scaler computes it - f64 product and sum of f32
// operands (no contraction: torch's f64 ops round twice), one rounding to f32.
__device__ __forceinline__ float policy_unscale_f64(float v, float lo, float hi, float scale, float shift) {
#pragma clang fp contract(off)
  const double c = (double)fminf(fmaxf(v, lo), hi);
  const double p = c * (double)scale;
  return (float)(p + (double)shift);
}
// f32: the product and the sum each rounded (no contraction) - policies.NativePolicy._action_tail with f64 = False
__device__ __forceinline__ float policy_unscale_f32(float v, float lo, float hi, float scale, float shift) {
#pragma clang fp contract(off)
  const float p = fminf(fmaxf(v, lo), hi) * scale;
  return p + shift;
}
// sum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ float policy_wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

}  // namespace d3il
