// policy_beso.h - everything between two block chains of the batched BESO sampler (policies.BESONativePolicy; agents/beso_agent.py:316-443, k_diffusion/gc_sampling.py
// 107-114 and 217-256 around k_diffusion/score_wrappers.py GCDenoiser and score_gpts.py DiffusionGPT) as ONE kernel (included by rollout.hip).
//
// S sampling steps over sigmas[0 .. S-1] = linspace(sigma_max, sigma_min, S), sigmas[S] = 0.  For environment n, window position j < W and step index i (i = 0 .. S-1
// are the Euler-ancestral steps, i = -1 is the init mode), all in f32, in the reference's order of operations (NOT the merged form of BESOPolicy._sample_device):
//   1. z = ln_f(hk[n, j, :])                               (nn.LayerNorm, biased variance; hk = the last block's output at the action positions)
//   2. net_a = w_pred[a] . z + b_pred[a], a < A            (the linear action_pred head)
//   3. den_a = coef[i][1] net_a + coef[i][0] x_a           (GCDenoiser: c_out net + c_skip x)
//   4. d_a = (x_a - den_a) coef[i][2]                      (to_d with 1 / s_from from the table)
//   5. x'_a = x_a + d_a coef[i][3]                         (dt = s_down - s_from)
//   6. i < S - 1: x'_a += coef[i][4] noise_a               (s_up; s_down > 0 on every step but the last), noise_a = noise_in[n, j, a] or Box-Muller on
//      philox4x32_10(seed, (env_offset + n, step word, BESO_TAG | (i + 1) << 8 | j << 1 | q)), component a = 4 q + m
//   7. i < S - 1: x[n, j, :] = x', xbuf[n, 2 + 2 j, c] = sum_a w_aemb[c][a] (coef[i][5] x'_a) + bias_pos[j][c] (coef[i][5] = c_in of sigmas[i + 1]) and once per
//      environment xbuf[n, 0, :] = semb[i + 1]
//   8. i = S - 1, j = len_n - 1: a_new = clamp(x', lo, hi) (scaled space), actions[n, a] = a_new scale_a + shift_a, and a_new is pushed onto the environment's
//      action ring a_hist[n, W - 1, A] (newest entry last) in place
// Init mode: steps 1 - 6 are skipped; x'[j] = the ring entry (W - 1) - (len_n - 1) + j for j < len_n - 1 (the previous clamped scaled actions, oldest first),
// x'[len_n - 1] = sigma_max noise with ONE draw per environment (draw index 0, j = 0 in the counter; noise_in[n, 0, :] when given), bad[n] is cleared, step 7 runs
// with c_in0 = c_in(sigmas[0]) and semb[0].  Positions j >= len_n: x' = 0, token = bias_pos[j].
// As torch ops a sampling step is the time token, LayerNorm, the head, addmm, a strided copy, four element-wise updates, randn and an add.
//
// Work distribution as k_ddpm_gpt_step: one wave owns one environment at a time and walks its W positions (bad flag, action, ring and sigma token have one writer:
// no atomics); four waves per workgroup, a block-stride loop whose trip count is the same for every wave of a workgroup.  Lane l holds elements l and 64 + l of a
// row, rows a < 8 of w_pred at those two columns and rows l, 64 + l of w_aemb.  LayerNorm statistics and head products are wave reductions, after which every lane
// holds all net_a: steps 3 - 6 run redundantly on every lane, the token is 2 x A fused multiply-adds per lane, lane a stores component a.
// No LDS, no scratch, no atomics; vector stores only; every branch in front of a shuffle is wave-uniform (kernel arguments and the environment's length).
//
// NaN / Inf: tested on the integer bit patterns (policy_nonfinite; the device pass is built with -ffinite-math-only) of the hidden row, the normalised row, the
// incoming iterate and x' at the VALID positions; a hit sets the sticky bad[n] (cleared by the init launch), and at i = S - 1 a bad environment gets 0x7FC00000 in
// every action component and in the ring entry it pushes, by integer selects.
#pragma once

namespace d3il {

constexpr unsigned BESO_TAG = 0x42530000u;      // fourth counter word = TAG | draw << 8 | j << 1 | q; its upper half is no other policy's
constexpr int BS_NW = 4, BS_CMAX = 128, BS_AMAX = 8, BS_WMAX = 16, BS_SMAX = 254;

struct BesoArgs {
  const float* hk; const float* ln_w; const float* ln_b; const float* w_pred; const float* b_pred; const float* w_aemb; const float* bias_pos; const float* semb;
  const float* coef; const float* lo; const float* hi; const float* scale; const float* shift;
  const long long* len; const unsigned* t_dev; const float* noise_in;
  float* x; float* xbuf; float* a_hist; float* actions; int* bad; float* noise_out;
  unsigned long long seed, env_offset;
  long n_env;
  float eps, sigma_max, c_in0;
  int C, A, W, S, i;
};

// the A <= 8 normals of one (environment, draw, position): two Philox blocks, the second only where A > 4 (wave-uniform)
__device__ __forceinline__ void beso_normals(unsigned long long seed, unsigned long long ge, unsigned t, unsigned tag, int A, float* nz) {
  unsigned r[4];
  philox4x32_10((unsigned)seed, (unsigned)(seed >> 32), (unsigned)ge, (unsigned)(ge >> 32), t, tag, r);
  policy_box_muller(r[0], r[1], nz[0], nz[1]); policy_box_muller(r[2], r[3], nz[2], nz[3]);
  if (A > 4) {
    philox4x32_10((unsigned)seed, (unsigned)(seed >> 32), (unsigned)ge, (unsigned)(ge >> 32), t, tag | 1u, r);
    policy_box_muller(r[0], r[1], nz[4], nz[5]); policy_box_muller(r[2], r[3], nz[6], nz[7]);
  } else {
    nz[4] = nz[5] = nz[6] = nz[7] = 0.f;
  }
}

template <int CT>      // CT 72 / 120: C == CT at compile time (the reference's widths); CT 128: any supported C, at run time
__global__ __launch_bounds__(64 * BS_NW) void k_beso_step(BesoArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = CT == BS_CMAX ? a.C : CT, A = a.A, W = a.W, S = a.S, i = a.i;
  const bool init = i < 0, last = i == S - 1;
  const bool c0 = lane < C, c1 = 64 + lane < C;
  // ---- per-lane constants: LayerNorm, the head's columns lane / 64 + lane, action_emb's rows lane / 64 + lane (zero beyond A and C)
  const float lw0 = c0 ? a.ln_w[lane] : 0.f, lb0 = c0 ? a.ln_b[lane] : 0.f, lw1 = c1 ? a.ln_w[64 + lane] : 0.f, lb1 = c1 ? a.ln_b[64 + lane] : 0.f;
  float wp0[BS_AMAX], wp1[BS_AMAX], we0[BS_AMAX], we1[BS_AMAX], bp[BS_AMAX];
#pragma unroll
  for (int q = 0; q < BS_AMAX; q++) {
    const bool in = q < A;
    wp0[q] = in && c0 ? a.w_pred[q * C + lane] : 0.f;
    wp1[q] = in && c1 ? a.w_pred[q * C + 64 + lane] : 0.f;
    we0[q] = in && c0 ? a.w_aemb[lane * A + q] : 0.f;
    we1[q] = in && c1 ? a.w_aemb[(64 + lane) * A + q] : 0.f;
    bp[q] = in ? a.b_pred[q] : 0.f;
  }
  const int al = lane < A ? lane : 0;      // the component this lane stores
  const float sc = a.scale[al], sh = a.shift[al], lol = a.lo[al], hil = a.hi[al];
  float c_skip = 0.f, c_out = 0.f, inv_s = 0.f, dt = 0.f, s_up = 0.f, c_in = a.c_in0;
  if (!init) { const float* s = a.coef + 6 * i; c_skip = s[0]; c_out = s[1]; inv_s = s[2]; dt = s[3]; s_up = s[4]; c_in = s[5]; }
  const float* const srow = a.semb + (long)(last ? 0 : i + 1) * C;
  const float se0 = c0 ? srow[lane] : 0.f, se1 = c1 ? srow[64 + lane] : 0.f;
  const unsigned t = *a.t_dev;
  const float inv_c = 1.0f / (float)C;
  const long per_pass = (long)gridDim.x * BS_NW;
  const long passes = (a.n_env + per_pass - 1) / per_pass;
  for (long it = 0; it < passes; it++) {
    const long n = (it * gridDim.x + blockIdx.x) * BS_NW + wave;
    if (n >= a.n_env) continue;      // (the whole wave: no barrier in this kernel)
    long long ln = a.len[n];
    const int len = ln < 1 ? 1 : (ln > W ? W : (int)ln);
    int bad = init ? 0 : a.bad[n];
    const unsigned long long ge = a.env_offset + (unsigned long long)n;
    float* const xb = a.xbuf + n * (long)(2 * W + 1) * C;
    float* const ring = a.a_hist + n * (long)(W - 1) * A;      // (W = 1: no ring, never dereferenced)
    if (!last) {      // the next iterate's sigma token
      if (c0) xb[lane] = se0;
      if (c1) xb[64 + lane] = se1;
    }
    float nz0[BS_AMAX];      // init mode: the one draw of this environment
#pragma unroll
    for (int q = 0; q < BS_AMAX; q++) nz0[q] = 0.f;
    if (init) {
      if (a.noise_in) {
#pragma unroll
        for (int q = 0; q < BS_AMAX; q++) nz0[q] = q < A ? a.noise_in[n * W * A + q] : 0.f;
      } else {
        beso_normals(a.seed, ge, t, BESO_TAG, A, nz0);
      }
    }
    for (int j = 0; j < W; j++) {
      const bool valid = j < len;      // wave-uniform
      const long row = n * W + j;
      float xp[BS_AMAX], nz[BS_AMAX];
      bool hit = false;
      if (init) {
        // ---- the first iterate: previous actions, then sigma_max noise at the newest position
        const bool prev = j < len - 1, newest = j == len - 1;      // wave-uniform
        const float* const e = ring + (long)((W - 1) - (len - 1) + j) * A;
#pragma unroll
        for (int q = 0; q < BS_AMAX; q++) {
          nz[q] = j == 0 ? nz0[q] : 0.f;
          float v = 0.f;
          if (prev && q < A) v = e[q];
          xp[q] = newest ? a.sigma_max * nz0[q] : v;
        }
      } else {
        // ---- 6. the noise of this (n, j, i)
        if (last) {
#pragma unroll
          for (int q = 0; q < BS_AMAX; q++) nz[q] = 0.f;
        } else if (a.noise_in) {
#pragma unroll
          for (int q = 0; q < BS_AMAX; q++) nz[q] = q < A ? a.noise_in[row * A + q] : 0.f;
        } else {
          beso_normals(a.seed, ge, t, BESO_TAG | ((unsigned)(i + 1) << 8) | ((unsigned)j << 1), A, nz);
        }
        // ---- 1. LayerNorm of the hidden row
        const float h0 = c0 ? a.hk[row * C + lane] : 0.f, h1 = c1 ? a.hk[row * C + 64 + lane] : 0.f;
        const float mean = policy_wave_sum(h0 + h1) * inv_c;
        const float d0 = c0 ? h0 - mean : 0.f, d1 = c1 ? h1 - mean : 0.f;
        const float rstd = 1.0f / sqrtf(policy_wave_sum(d0 * d0 + d1 * d1) * inv_c + a.eps);
        const float z0 = d0 * rstd * lw0 + lb0, z1 = d1 * rstd * lw1 + lb1;
        hit = __ballot(policy_nonfinite(h0) || policy_nonfinite(h1) || policy_nonfinite(z0) || policy_nonfinite(z1)) != 0ull;
        // ---- 2. the head, 3. the Karras combination, 4. the derivative, 5. the Euler step, 6. the ancestral noise
#pragma unroll
        for (int q = 0; q < BS_AMAX; q++) {
          const float net = policy_wave_sum(fmaf(wp1[q], z1, wp0[q] * z0)) + bp[q];
          const float xq = q < A ? a.x[row * A + q] : 0.f;
          const float den = c_out * net + c_skip * xq;
          const float d = (xq - den) * inv_s;
          const float xe = xq + d * dt;
          xp[q] = last ? xe : xe + s_up * nz[q];
          hit = hit || policy_nonfinite(xq);
        }
      }
#pragma unroll
      for (int q = 0; q < BS_AMAX; q++) {
        hit = hit || (q < A && policy_nonfinite(xp[q]));
        unsigned b = __float_as_uint(xp[q]);
        b = valid ? b : 0u;      // padded positions: x' = 0, the token is bias_pos[j]
        xp[q] = __uint_as_float(b);
      }
      bad |= (valid && hit) ? 1 : 0;
      // ---- this lane's component of x' and of the noise
      float xl = 0.f, nl = 0.f;
#pragma unroll
      for (int q = 0; q < BS_AMAX; q++) { xl = lane == q ? xp[q] : xl; nl = lane == q ? nz[q] : nl; }
      if (a.noise_out && lane < A) a.noise_out[row * A + lane] = nl;
      if (!last) {
        // ---- 7. the iterate and its action token
        if (lane < A) a.x[row * A + lane] = xl;
        const float* const bpos = a.bias_pos + (long)j * C;
        float t0 = c0 ? bpos[lane] : 0.f, t1 = c1 ? bpos[64 + lane] : 0.f;
        float u0 = 0.f, u1 = 0.f;
#pragma unroll
        for (int q = 0; q < BS_AMAX; q++) { const float xs = c_in * xp[q]; u0 = fmaf(we0[q], xs, u0); u1 = fmaf(we1[q], xs, u1); }
        t0 += u0; t1 += u1;
        float* const tok = xb + (long)(2 + 2 * j) * C;
        if (c0) tok[lane] = t0;
        if (c1) tok[64 + lane] = t1;
      } else if (j == len - 1) {
        // ---- 8. the action of the newest valid position, and the ring
        const float an = fminf(fmaxf(xl, lol), hil);
        unsigned ab = __float_as_uint(an), yb = __float_as_uint(an * sc + sh);
        ab = bad ? 0x7FC00000u : ab;
        yb = bad ? 0x7FC00000u : yb;
        if (lane < A) {
          ((unsigned*)a.actions)[n * A + lane] = yb;
          if (W > 1) {
            for (int e = 0; e < W - 2; e++) ring[e * A + lane] = ring[(e + 1) * A + lane];
            ((unsigned*)ring)[(W - 2) * A + lane] = ab;
          }
        }
      }
    }
    if (lane == 0) a.bad[n] = bad;
  }
}

}  // namespace d3il
