// policy_cvae.h - the whole inference of the batched conditional-VAE policy (policies.CVAEPolicy; agents/cvae_agent.py:155-170 around
// agents/models/vae/cvae.py:55-62 over common/mlp.py ResidualMLPNetwork) as ONE kernel.  Included by rollout.hip behind policy_resmlp.h, whose pieces the
// decoder is built from (the random stream, the bit test and the inverse scaling: policy_common.h).
//
// For environment n (s = the scaled state row, L = latent width, the decoder a Mish ResidualMLPNetwork on [s | z], f32 throughout):
//   1. z_a = clamp(z_in[n, a] or Box-Muller on philox4x32_10(seed, (env_offset + n, step word, CVAE_TAG | q)), -0.5, 0.5), component a = 4 q + m takes word m.
//      The reference clamps its PRIOR sample to +-0.5 (cvae.py:58): 2 (1 - Phi(0.5)) = 61.7 % of all latent components sit exactly on a bound.  Kept.
//   2. out = decoder([s | z]): state first, latent second
//   3. actions[n, a] = clamp(out_a, lo_a, hi_a) scale_a + shift_a (the product and the sum in f64 on the f32 operands, as the reference's f64 scaler does;
//      rounded to f32 once)
//
// Tiling: policy_resmlp.h's (16 rows per workgroup of eight waves, activations through LDS, one barrier per layer).  What differs from k_resmlp_f32: (a) the input
// row is assembled here - the latent is drawn ONCE per workgroup by waves 0 and 1 (thread (q, j): Philox call q of row j, two Box-Muller pairs,
// four components) and shared through 2.3 KB of LDS behind one more barrier, because the alternative - every lane draws what it needs - costs each
// lane of each wave eight Philox calls and eight Box-Muller pairs for its sixteen input features (a lane's features 4 s + g - obs hit one word of up to eight
// different calls): 4096 Philox calls per workgroup instead of 128, for the price of one barrier; (b) the input layer is the 64-column one (rm_input64); (c) the tail
// is fused: output bias, clamp, inverse scaling, bit tests; (d) the step word comes from device memory.
//
// LDS: xb 2 x NT x 64 float4 (16 / 32 KB), zs 16 x 36 words.  Vector stores only, no inline assembly beyond the empty register barrier of policy_nonfinite; every branch
// in front of a barrier depends on the wave index or on kernel arguments only.  NaN / Inf: the device pass is built with -ffinite-math-only, so the state row, the
// latent before its clamp and the outputs before theirs are tested on their bit patterns (exponent field all ones); a hit gives 0x7FC00000 in every action
// component of that environment (and in the z_out components that were hit).  Rows never mix: column j of every matrix-core product is row j.
#pragma once

namespace d3il {

constexpr unsigned CVAE_TAG = 0x43560000u;      // fourth counter word = TAG | q (q < 8): never 0, never BET_TAG, never a DDPM_GPT_TAG, IBC_TAG or ACT_TAG word
constexpr int CVAE_LMAX = 32, CVAE_INMAX = 64, CVAE_AMAX = 16, CVAE_ZSTRIDE = 36;

struct CvaeArgs {
  const float* state; const float* w_in; const float* b_in; const float* w_blk; const float* b_blk; const float* w_out; const float* b_out;
  const float* lo; const float* hi; const float* scale; const float* shift;
  const unsigned* t_dev; const float* z_in;
  float* actions; float* z_out;
  unsigned long long seed, env_offset;
  long n_env;
  int obs, L, A, nblk;
};

template <int HID>
__global__ __launch_bounds__(512) void k_cvae_decode(CvaeArgs a) {
  constexpr int NT = HID / 16, TPW = NT / 8;
  __shared__ mlp_f4 xb[2][NT * 64];
  __shared__ unsigned zs[16 * CVAE_ZSTRIDE];      // the 16 rows' clamped latents (bits; 0x7FC00000 where the unclamped value was NaN / Inf)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const int OBS = a.obs, L = a.L, A = a.A, nblk = a.nblk;
  const long n = a.n_env;
  const long row = (long)blockIdx.x * 16 + j;
  const bool live = row < n;
  const long rr = live ? row : (n - 1);
  // ---- 1. the latent, once per workgroup: thread (q, jz) of waves 0 and 1 owns components 4 q .. 4 q + 3 of row jz
  if (w < 2) {
    const int jz = tid & 15, q = tid >> 4;
    const long rowz = (long)blockIdx.x * 16 + jz;
    const bool livez = rowz < n;
    const long rz = livez ? rowz : (n - 1);
    if (4 * q < L) {
      float z[4];
      if (a.z_in) {
#pragma unroll
        for (int m = 0; m < 4; m++) z[m] = 4 * q + m < L ? a.z_in[rz * L + 4 * q + m] : 0.f;
      } else {
        const unsigned long long ge = a.env_offset + (unsigned long long)rz;
        unsigned r[4];
        policy_philox(a.seed, ge, *a.t_dev, CVAE_TAG | (unsigned)q, r);
        policy_box_muller(r[0], r[1], z[0], z[1]); policy_box_muller(r[2], r[3], z[2], z[3]);
      }
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const unsigned zb = policy_nonfinite(z[m]) ? 0x7FC00000u : __float_as_uint(fminf(fmaxf(z[m], -0.5f), 0.5f));
        zs[jz * CVAE_ZSTRIDE + 4 * q + m] = zb;
        if (a.z_out && livez && 4 * q + m < L) ((unsigned*)a.z_out)[rowz * L + 4 * q + m] = zb;
      }
    }
  }
  __syncthreads();
  // ---- 2. the input row [state | z]: lane (g, j) holds feature 4 s2 + g of row j
  float in_k[16];
#pragma unroll
  for (int s2 = 0; s2 < 16; s2++) {
    const int f = 4 * s2 + g, zi = f - OBS, zc = zi < 0 ? 0 : (zi > CVAE_LMAX - 1 ? CVAE_LMAX - 1 : zi);
    const float zv = __uint_as_float(zs[j * CVAE_ZSTRIDE + zc]);
    in_k[s2] = f < OBS ? a.state[rr * OBS + f] : (zi < L ? zv : 0.f);
  }
  unsigned bad = 0u;      // this lane's quarter of the input row, tested here: in_k is dead after the input layer
#pragma unroll
  for (int s2 = 0; s2 < 16; s2++) bad |= (unsigned)policy_nonfinite(in_k[s2]);
  // ---- the decoder's trunk (policy_resmlp.h): 64-column input layer from b_in, the residual blocks, the output tile by wave 0
  mlp_f4 xo[TPW];
  rm_input64<HID, true>(a.w_in, a.b_in, in_k, xo, w, lane, g);
  int buf = 0;
  rm_blocks<HID>(a.w_blk, a.b_blk, nblk, xb, xo, buf, w, lane, g);
  rm_store<HID, false>(xb[buf], xo, w, lane);
  __syncthreads();
  if (w != 0) return;      // (after the last barrier) the output tile and the tail are one wave's work
  const mlp_f4 acc = rm_tile<HID>((const mlp_f4*)a.w_out, xb[buf], mlp_f4{0.f, 0.f, 0.f, 0.f}, lane);
  // ---- 3. the tail: lane (g, j), register r = component 4 g + r of row j.  The row's verdict is the OR over its four lanes: each saw a quarter of the input row.
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    v[r] = acc[r] + a.b_out[4 * g + r];      // (b_out is padded to 16)
    bad |= 4 * g + r < A ? (unsigned)policy_nonfinite(v[r]) : 0u;
  }
  bad = rm_row_or(bad);
  if (live) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int c = 4 * g + r;
      if (c < A) {
        const unsigned yb = __float_as_uint(policy_unscale_f64(v[r], a.lo[c], a.hi[c], a.scale[c], a.shift[c]));
        ((unsigned*)a.actions)[row * A + c] = bad ? 0x7FC00000u : yb;
      }
    }
  }
}

}  // namespace d3il
