// policy_gpt_bc.h - the tail of the batched BC-GPT policy (policies.GPTBCPolicy; agents/gpt_bc_agent.py:221-247 around agents/models/transformer/gpt_policy.py MinGPT,
// the BeT library's GPT with vocab_size = action_dim) as ONE small kernel (included by rollout.hip behind policy_common.h, whose policy_unscale_f64 it uses).
//
// Per row (= environment; h = the last block's output at the lane's last token):
//   1. x = ln_f(h)                                         (nn.LayerNorm, biased variance; the order of operations of k_bet_head)
//   2. o_a = w_head[a] . x, a < A                          (the head has no bias)
//   3. y_a = clamp(o_a, lo_a, hi_a) scale_a + shift_a      (clamp in f32; product and sum in f64 on the f32 operands, rounded once - the reference's scaler is f64)
// As torch ops that is a LayerNorm, a [N, C] x [C, A] product and three element-wise kernels.  There are no random numbers.
//
// One wave works on one row at a time in a block-stride loop (no barrier, no LDS: a wave's trip count is its own).  Lane l holds elements l and 64 + l of the row and
// of every head row (2 A registers, loaded once per wave); the LayerNorm statistics and the A dot products are wave reductions; lane a < A keeps and stores
// component a.  No atomics, no scratch; all stores are vector stores.
//
// NaN / Inf rows: the device pass is built with -ffinite-math-only, so h, the normalised row and the head outputs are tested on their bit patterns
// (policy_nonfinite) and a hit row gets 0x7FC00000 in every action component by an integer select (bad[row] = 1).  No other row changes.
#pragma once

namespace d3il {

constexpr int GB_NW = 4, GB_CMAX = 128, GB_AMAX = 16;

struct GptBcHeadArgs {
  const float* h; const float* ln_w; const float* ln_b; const float* w_head;
  const float* lo; const float* hi; const float* scale; const float* shift;
  float* actions; int* bad;
  long rows;
  float eps;
  int C, A;
};

__global__ __launch_bounds__(64 * GB_NW) void k_gpt_bc_head(GptBcHeadArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C, A = a.A;
  const bool in0 = lane < C, in1 = 64 + lane < C;
  float w0[GB_AMAX], w1[GB_AMAX];
#pragma unroll
  for (int c = 0; c < GB_AMAX; c++) {
    w0[c] = c < A && in0 ? a.w_head[c * C + lane] : 0.f;
    w1[c] = c < A && in1 ? a.w_head[c * C + 64 + lane] : 0.f;
  }
  const float lw0 = in0 ? a.ln_w[lane] : 0.f, lb0 = in0 ? a.ln_b[lane] : 0.f;
  const float lw1 = in1 ? a.ln_w[64 + lane] : 0.f, lb1 = in1 ? a.ln_b[64 + lane] : 0.f;
  const bool comp = lane < A;
  const int cl_i = comp ? lane : 0;
  const float cl = a.lo[cl_i], ch = a.hi[cl_i], sc = a.scale[cl_i], sh = a.shift[cl_i];
  const float inv_c = 1.0f / (float)C;
  for (long row = (long)blockIdx.x * GB_NW + wave; row < a.rows; row += (long)gridDim.x * GB_NW) {
    // ---- 1. LayerNorm of the row
    const float h0 = in0 ? a.h[row * C + lane] : 0.f, h1 = in1 ? a.h[row * C + 64 + lane] : 0.f;
    const float mean = policy_wave_sum(h0 + h1) * inv_c;
    const float d0 = in0 ? h0 - mean : 0.f, d1 = in1 ? h1 - mean : 0.f;
    const float rstd = 1.0f / sqrtf(policy_wave_sum(d0 * d0 + d1 * d1) * inv_c + a.eps);
    const float x0 = d0 * rstd * lw0 + lb0, x1 = d1 * rstd * lw1 + lb1;
    const bool bad_x = __ballot(policy_nonfinite(h0) || policy_nonfinite(h1) || policy_nonfinite(x0) || policy_nonfinite(x1)) != 0ull;
    // ---- 2. the head: component c ends up in lane c
    float mine = 0.f;
#pragma unroll
    for (int c = 0; c < GB_AMAX; c++) {
      if (c < A) {      // (a kernel argument: the whole wave takes the same side)
        const float dot = policy_wave_sum(fmaf(w1[c], x1, w0[c] * x0));
        mine = lane == c ? dot : mine;
      }
    }
    const bool bad_o = __ballot(comp && policy_nonfinite(mine)) != 0ull;
    const bool bad = bad_x | bad_o;
    // ---- 3. the action
    if (comp) {
      const unsigned yb = __float_as_uint(policy_unscale_f64(mine, cl, ch, sc, sh));
      ((unsigned*)a.actions)[row * A + lane] = bad ? 0x7FC00000u : yb;
    }
    if (a.bad && lane == 0) a.bad[row] = bad ? 1 : 0;
  }
}

}  // namespace d3il
