// policy_ddpm_gpt.h - everything between two block chains of the batched DDPM-GPT sampler (policies.DDPMGPTPolicy; agents/ddpm_agent.py:213-274,
// agents/models/diffusion/gc_diffusion.py:117-216 around diffusion_models.py DiffusionTransformerNetwork) as ONE kernel (included by rollout.hip).
//
// For environment n, window position j < W and chain index k (k = T - 1 .. 0 are the reverse steps, k = T is the init mode), all in f32:
//   1. z = ln_f(hk[n, j, :])                               (nn.LayerNorm, biased variance; hk = the last block's output at the action positions)
//   2. eps_a = w_pred[a] . z + b_pred[a], a < A            (the linear action_pred head)
//   3. x0_a = clamp(sched[k][0] x_a - sched[k][1] eps_a, lo_a, hi_a)          (bounds in scaled space)
//   4. mean_a = sched[k][2] x0_a + sched[k][3] x_a
//   5. noise_a = noise_in[n, j, a], or Box-Muller on philox4x32_10(seed, (env_offset + n, step word, DDPM_GPT_TAG | k << 8 | j << 1 | q)), component a = 4 q + m
//   6. x'_a = mean_a + sched[k][4] noise_a                 (k = 0: x' = mean, nothing is drawn)
//   7. k > 0: x[n, j, :] = x', xbuf[n, 2 + 2 j, c] = sum_a w_aemb[c][a] x'_a + bias_pos[j][c], and once per environment xbuf[n, 0, :] = temb[k - 1]
//   8. k = 0, j = len_n - 1: actions[n, a] = clamp(x'_a, lo_a, hi_a) scale_a + shift_a
// Init mode (k = T): steps 1 - 4 are skipped, x' = noise, step 7 runs with temb[T - 1].  Positions j >= len_n: x' = 0, token = bias_pos[j].
// As torch ops that is index_select, LayerNorm, the head, two scalings, clamp, the posterior mean, randn, add, addmm and two strided copies per sampling step.
//
// One wave owns one environment at a time and walks its W positions (the per-environment outputs - bad flag, action, time token - have one writer: no atomics);
// four waves per workgroup, a block-stride loop over the environments whose trip count is the same for every wave of a workgroup.  Lane l holds elements l and
// 64 + l of a row (loads and token stores are coalesced), rows a < 8 of w_pred at those two columns (16 registers) and rows l, 64 + l of w_aemb (16 registers).
// The LayerNorm statistics and the A head products are wave reductions, after which EVERY lane holds all eps_a: steps 3 - 6 run redundantly on every lane (a few
// dozen instructions), the token of step 7 is then 2 x A fused multiply-adds per lane with no further exchange, and lane a stores component a of x' / the action.
// No LDS, no scratch, no atomics; vector stores only; every branch in front of a shuffle is wave-uniform (kernel arguments and the environment's length).
//
// NaN / Inf: the device pass is built with -ffinite-math-only, so (as policy_bet.h) rows are tested on the integer bit patterns (exponent field all ones; the bits
// pass through an empty asm) of the hidden row, the normalised row, the incoming iterate and x' at the VALID positions; a hit sets the sticky bad[n] (cleared by the
// init launch, written by the environment's own wave), and at k = 0 a bad environment gets 0x7FC00000 in every action component by an integer select.
#pragma once

namespace d3il {

constexpr unsigned DDPM_GPT_TAG = 0x44470000u;      // fourth counter word = TAG | k << 8 | j << 1 | q: never 0 (k_policy_action) and never BET_TAG
constexpr int DG_NW = 4, DG_CMAX = 128, DG_AMAX = 8, DG_WMAX = 16, DG_TMAX = 255;


struct DdpmGptArgs {
  const float* hk; const float* ln_w; const float* ln_b; const float* w_pred; const float* b_pred; const float* w_aemb; const float* bias_pos; const float* temb;
  const float* sched; const float* lo; const float* hi; const float* scale; const float* shift;
  const long long* len; const unsigned* t_dev; const float* noise_in;
  float* x; float* xbuf; float* actions; int* bad; float* noise_out;
  unsigned long long seed, env_offset;
  long n_env;
  float eps;
  int C, A, W, T, k;
};

template <int CT>      // CT 72 / 120: C == CT at compile time (the reference's widths); CT 128: any supported C, at run time
__global__ __launch_bounds__(64 * DG_NW) void k_ddpm_gpt_step(DdpmGptArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = CT == DG_CMAX ? a.C : CT, A = a.A, W = a.W, T = a.T, k = a.k;
  const bool init = k == T;
  const bool c0 = lane < C, c1 = 64 + lane < C;
  // ---- per-lane constants: LayerNorm, the head's columns lane / 64 + lane, action_emb's rows lane / 64 + lane (zero beyond A and C)
  const float lw0 = c0 ? a.ln_w[lane] : 0.f, lb0 = c0 ? a.ln_b[lane] : 0.f, lw1 = c1 ? a.ln_w[64 + lane] : 0.f, lb1 = c1 ? a.ln_b[64 + lane] : 0.f;
  float wp0[DG_AMAX], wp1[DG_AMAX], we0[DG_AMAX], we1[DG_AMAX], bp[DG_AMAX], lo[DG_AMAX], hi[DG_AMAX];
#pragma unroll
  for (int q = 0; q < DG_AMAX; q++) {
    const bool in = q < A;
    wp0[q] = in && c0 ? a.w_pred[q * C + lane] : 0.f;
    wp1[q] = in && c1 ? a.w_pred[q * C + 64 + lane] : 0.f;
    we0[q] = in && c0 ? a.w_aemb[lane * A + q] : 0.f;
    we1[q] = in && c1 ? a.w_aemb[(64 + lane) * A + q] : 0.f;
    bp[q] = in ? a.b_pred[q] : 0.f;
    lo[q] = in ? a.lo[q] : 0.f;
    hi[q] = in ? a.hi[q] : 0.f;
  }
  const int al = lane < A ? lane : 0;      // the component this lane stores
  const float sc = a.scale[al], sh = a.shift[al];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
  if (!init) { const float* s = a.sched + 5 * k; s0 = s[0]; s1 = s[1]; s2 = s[2]; s3 = s[3]; s4 = s[4]; }
  const float* const trow = a.temb + (long)(k > 0 ? k - 1 : 0) * C;
  const float te0 = c0 ? trow[lane] : 0.f, te1 = c1 ? trow[64 + lane] : 0.f;
  const unsigned t = *a.t_dev;
  const float inv_c = 1.0f / (float)C;
  const long per_pass = (long)gridDim.x * DG_NW;
  const long passes = (a.n_env + per_pass - 1) / per_pass;
  for (long it = 0; it < passes; it++) {
    const long n = (it * gridDim.x + blockIdx.x) * DG_NW + wave;
    if (n >= a.n_env) continue;      // (the whole wave: no barrier in this kernel)
    long long ln = a.len[n];
    const int len = ln < 1 ? 1 : (ln > W ? W : (int)ln);
    int bad = init ? 0 : a.bad[n];
    const unsigned long long ge = a.env_offset + (unsigned long long)n;
    float* const xb = a.xbuf + n * (long)(2 * W + 1) * C;
    if (k > 0) {      // the next iterate's time token
      if (c0) xb[lane] = te0;
      if (c1) xb[64 + lane] = te1;
    }
    for (int j = 0; j < W; j++) {
      const bool valid = j < len;      // wave-uniform
      const long row = n * W + j;
      float xp[DG_AMAX], nz[DG_AMAX];
      // ---- 5. the noise of this (n, j, k)
      if (a.noise_in) {
#pragma unroll
        for (int q = 0; q < DG_AMAX; q++) nz[q] = q < A ? a.noise_in[row * A + q] : 0.f;
      } else if (k > 0) {
        const unsigned tag = DDPM_GPT_TAG | ((unsigned)k << 8) | ((unsigned)j << 1);
        unsigned r[4];
        philox4x32_10((unsigned)a.seed, (unsigned)(a.seed >> 32), (unsigned)ge, (unsigned)(ge >> 32), t, tag, r);
        policy_box_muller(r[0], r[1], nz[0], nz[1]); policy_box_muller(r[2], r[3], nz[2], nz[3]);
        if (A > 4) {
          philox4x32_10((unsigned)a.seed, (unsigned)(a.seed >> 32), (unsigned)ge, (unsigned)(ge >> 32), t, tag | 1u, r);
          policy_box_muller(r[0], r[1], nz[4], nz[5]); policy_box_muller(r[2], r[3], nz[6], nz[7]);
        } else {
          nz[4] = nz[5] = nz[6] = nz[7] = 0.f;
        }
      } else {
#pragma unroll
        for (int q = 0; q < DG_AMAX; q++) nz[q] = 0.f;
      }
      bool hit = false;
      if (init) {
#pragma unroll
        for (int q = 0; q < DG_AMAX; q++) xp[q] = nz[q];
      } else {
        // ---- 1. LayerNorm of the hidden row
        const float h0 = c0 ? a.hk[row * C + lane] : 0.f, h1 = c1 ? a.hk[row * C + 64 + lane] : 0.f;
        const float mean = policy_wave_sum(h0 + h1) * inv_c;
        const float d0 = c0 ? h0 - mean : 0.f, d1 = c1 ? h1 - mean : 0.f;
        const float rstd = 1.0f / sqrtf(policy_wave_sum(d0 * d0 + d1 * d1) * inv_c + a.eps);
        const float z0 = d0 * rstd * lw0 + lb0, z1 = d1 * rstd * lw1 + lb1;
        hit = __ballot(policy_nonfinite(h0) || policy_nonfinite(h1) || policy_nonfinite(z0) || policy_nonfinite(z1)) != 0ull;
        // ---- 2. the head, 3. clipped x0, 4. posterior mean, 6. the next iterate
#pragma unroll
        for (int q = 0; q < DG_AMAX; q++) {
          const float e = policy_wave_sum(fmaf(wp1[q], z1, wp0[q] * z0)) + bp[q];
          const float xq = q < A ? a.x[row * A + q] : 0.f;
          const float x0 = fminf(fmaxf(s0 * xq - s1 * e, lo[q]), hi[q]);
          const float m = s2 * x0 + s3 * xq;
          xp[q] = k == 0 ? m : m + s4 * nz[q];
          hit = hit || policy_nonfinite(xq);
        }
      }
#pragma unroll
      for (int q = 0; q < DG_AMAX; q++) {
        hit = hit || (q < A && policy_nonfinite(xp[q]));
        unsigned b = __float_as_uint(xp[q]);
        b = valid ? b : 0u;      // padded positions: x' = 0, the token is bias_pos[j]
        xp[q] = __uint_as_float(b);
      }
      bad |= (valid && hit) ? 1 : 0;
      // ---- this lane's component of x' and of the noise
      float xl = 0.f, nl = 0.f;
#pragma unroll
      for (int q = 0; q < DG_AMAX; q++) { xl = lane == q ? xp[q] : xl; nl = lane == q ? nz[q] : nl; }
      if (a.noise_out && lane < A) a.noise_out[row * A + lane] = nl;
      if (k > 0) {
        // ---- 7. the iterate and its action token
        if (lane < A) a.x[row * A + lane] = xl;
        const float* const bpos = a.bias_pos + (long)j * C;
        float t0 = c0 ? bpos[lane] : 0.f, t1 = c1 ? bpos[64 + lane] : 0.f;
        float u0 = 0.f, u1 = 0.f;
#pragma unroll
        for (int q = 0; q < DG_AMAX; q++) { u0 = fmaf(we0[q], xp[q], u0); u1 = fmaf(we1[q], xp[q], u1); }
        t0 += u0; t1 += u1;
        float* const tok = xb + (long)(2 + 2 * j) * C;
        if (c0) tok[lane] = t0;
        if (c1) tok[64 + lane] = t1;
      } else if (j == len - 1) {
        // ---- 8. the action of the newest valid position
        float lol = 0.f, hil = 0.f;
#pragma unroll
        for (int q = 0; q < DG_AMAX; q++) { lol = lane == q ? lo[q] : lol; hil = lane == q ? hi[q] : hil; }
        unsigned yb = __float_as_uint(fminf(fmaxf(xl, lol), hil) * sc + sh);
        yb = bad ? 0x7FC00000u : yb;
        if (lane < A) ((unsigned*)a.actions)[n * A + lane] = yb;
      }
    }
    if (lane == 0) a.bad[n] = bad;
  }
}

}  // namespace d3il
