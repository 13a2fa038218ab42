// policy_bet.h - the sampling head of the batched Behaviour-Transformer policy (policies.BeTPolicy; agents/bet_agent.py:359-372,
// agents/models/bet/latent_generators/mingpt.py:155-186, action_ae/discretizers/k_means.py:111-138) as ONE kernel (included by rollout.hip).
//
// Per row (= environment; h = the last block's output at the lane's last token), all in f32:
//   1. x = ln_f(h)                                         (nn.LayerNorm, biased variance)
//   2. logit_v = w_head[v] . x, v < 64                     (the head has no bias)
//   3. p_v = exp(logit_v - max), S = sum p, c_v = inclusive prefix sums
//   4. u = 24 bits of philox4x32_10(seed, env_offset + row, t, BET_TAG) (or u_in[row])
//   5. bin = min(#{v : c_v <= u S}, 63)                    (inverse CDF: empty bins in front of the drawn one are skipped, 64 is never returned)
//   6. off_a = w_head[64 + bin A + a] . x                  (layout "(V A)")
//   7. y_a = clamp(centers[bin][a] + off_a, lo_a, hi_a) scale_a + shift_a
// As torch ops that is a [N, C] x [C, 64 (1 + A)] product of which 63 / 64 of the offset columns are thrown away, a softmax, a multinomial (device generator:
// the draw depends on batch order), a gather and four element-wise kernels.
//
// One wave works on one row at a time, lane = bin.  Lane v keeps w_head[v][0 .. C) in registers across the rows of its wave (a block-stride loop; the trip count
// is the same for the four waves of a workgroup, so the barrier inside is uniform).  The row of h is loaded coalesced (lane l: elements l and 64 + l), the LayerNorm
// statistics are wave reductions, the normalised row goes through LDS (every lane reads all of it: broadcast reads), max / sum are wave reductions, the prefix
// sums a six-step shuffle scan, the draw one ballot + pop count.  The A offset products: 8 lanes per action component (group a = lane / 8), lane sub = lane % 8
// takes the float4 chunks sub, sub + 8, .. of row 64 + bin A + a (the 64 A rows stay in L2: 245 KB for C = 120, A = 8), three shuffle steps per group;
// the products are written without a divergent branch in front of the shuffles.
// No atomics, no scratch; all stores are vector stores.
//
// NaN / Inf rows: the device pass is built with -ffinite-math-only (an FP isnan folds to false, an FP select of a NaN constant may be dropped; policy_f16x3.h
// "range / NaN guard").  So the row is tested on the integer bit patterns of h and of the normalised row (exponent field all ones; the bits pass through an empty
// asm) and the outputs of a bad row are put in with integer selects: bins = -1, every action component = 0x7FC00000.  The row's arithmetic still runs (on garbage);
// nothing of it is kept, and no index depends on it beyond bin, which the pop count bounds to 0 .. 63 whatever the comparisons gave.
#pragma once

namespace d3il {

constexpr unsigned BET_TAG = 0x42655448u;      // fourth counter word of the head's Philox stream (k_policy_action uses 0: the streams never coincide)
constexpr int BET_V = 64, BET_NW = 4, BET_CMAX = 128, BET_AMAX = 8;
typedef float bet_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bet_wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

struct BetHeadArgs {
  const float* h; const float* ln_w; const float* ln_b; const float* w_head; const float* centers;
  const float* lo; const float* hi; const float* scale; const float* shift;
  const unsigned* t_dev; const float* u_in;
  float* actions; int* bins; float* u_out; float* probs;
  unsigned long long seed, env_offset;
  long rows;
  float eps;
  int C, A;
};

template <int CT>      // register rows of CT floats: C <= CT (72 and 120 are the reference's widths; 128 serves every other supported C)
__global__ __launch_bounds__(64 * BET_NW) void k_bet_head(BetHeadArgs a) {
  __shared__ bet_f4 xs[BET_NW][BET_CMAX / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int C = a.C, A = a.A, C4 = C >> 2;
  // ---- this lane's row of the logit weights
  bet_f4 w[CT / 4];
#pragma unroll
  for (int q = 0; q < CT / 4; q++) w[q] = q < C4 ? *(const bet_f4*)(a.w_head + (long)lane * C + 4 * q) : bet_f4{0.f, 0.f, 0.f, 0.f};
  const float lw0 = lane < C ? a.ln_w[lane] : 0.f, lb0 = lane < C ? a.ln_b[lane] : 0.f;
  const float lw1 = 64 + lane < C ? a.ln_w[64 + lane] : 0.f, lb1 = 64 + lane < C ? a.ln_b[64 + lane] : 0.f;
  const int grp = lane >> 3, sub = lane & 7;      // offset products: component grp, chunk phase sub
  const bool comp = grp < A;
  float cl = 0.f, ch = 0.f, sc = 0.f, sh = 0.f;
  if (comp) { cl = a.lo[grp]; ch = a.hi[grp]; sc = a.scale[grp]; sh = a.shift[grp]; }
  const unsigned t = *a.t_dev;
  const float inv_c = 1.0f / (float)C;
  float* const xrow = (float*)xs[wave];
  const long per_pass = (long)gridDim.x * BET_NW;
  const long passes = (a.rows + per_pass - 1) / per_pass;
  for (long it = 0; it < passes; it++) {
    const long row = (it * gridDim.x + blockIdx.x) * BET_NW + wave;
    const bool live = row < a.rows;
    const long rr = live ? row : a.rows - 1;
    // ---- 1. LayerNorm of the row
    const float h0 = lane < C ? a.h[rr * C + lane] : 0.f, h1 = 64 + lane < C ? a.h[rr * C + 64 + lane] : 0.f;
    const float mean = policy_wave_sum(h0 + h1) * inv_c;
    const float d0 = lane < C ? h0 - mean : 0.f, d1 = 64 + lane < C ? h1 - mean : 0.f;
    const float rstd = 1.0f / sqrtf(policy_wave_sum(d0 * d0 + d1 * d1) * inv_c + a.eps);
    const float x0 = d0 * rstd * lw0 + lb0, x1 = d1 * rstd * lw1 + lb1;
    const bool bad = __ballot(policy_nonfinite(h0) || policy_nonfinite(h1) || policy_nonfinite(x0) || policy_nonfinite(x1)) != 0ull;
    if (lane < C) xrow[lane] = x0;      // (this wave's own slice: its reads of the previous pass were issued before these writes)
    if (64 + lane < C) xrow[64 + lane] = x1;
    __syncthreads();
    // ---- 2. logit of bin `lane`
    float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
    for (int q = 0; q < CT / 4; q++) {
      if (q < C4) {
        const bet_f4 xv = xs[wave][q];
        acc0 = fmaf(w[q][0], xv[0], acc0); acc1 = fmaf(w[q][1], xv[1], acc1);
        acc0 = fmaf(w[q][2], xv[2], acc0); acc1 = fmaf(w[q][3], xv[3], acc1);
      }
    }
    const float logit = acc0 + acc1;
    // ---- 3. softmax numerators and their prefix sums
    const float p = expf(logit - bet_wave_max(logit));
    float c = p;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const float up = __shfl_up(c, s); c += lane >= s ? up : 0.f; }
    const float S = __shfl(c, 63);
    // ---- 4. the uniform, 5. the bin
    float u;
    if (a.u_in) u = a.u_in[rr];
    else {
      const unsigned long long ge = a.env_offset + (unsigned long long)rr;
      unsigned r[4];
      philox4x32_10((unsigned)a.seed, (unsigned)(a.seed >> 32), (unsigned)ge, (unsigned)(ge >> 32), t, BET_TAG, r);
      u = policy_uniform24(r[0]);
    }
    const int cnt = __popcll(__ballot(c <= u * S));
    const int bin = cnt < BET_V - 1 ? cnt : BET_V - 1;
    // ---- 6. offsets of the drawn bin, 7. the action
    // (no divergent branch in front of the shuffles: groups beyond A repeat component A - 1, chunks beyond C re-read chunk 0 and add nothing)
    float part = 0.f;
    const float* wo = a.w_head + ((long)BET_V + (long)bin * A + (comp ? grp : A - 1)) * C;
#pragma unroll
    for (int j = 0; j < BET_CMAX / 32; j++) {
      const bool in = sub + 8 * j < C4;
      const int q = in ? sub + 8 * j : 0;
      const bet_f4 wv = *(const bet_f4*)(wo + 4 * q), xv = xs[wave][q];
      const float dot = fmaf(wv[3], xv[3], fmaf(wv[2], xv[2], fmaf(wv[1], xv[1], wv[0] * xv[0])));
      part += in ? dot : 0.f;
    }
    __builtin_amdgcn_wave_barrier();
    part += __shfl_xor(part, 1); part += __shfl_xor(part, 2); part += __shfl_xor(part, 4);
    __builtin_amdgcn_wave_barrier();
    if (live) {
      if (comp && sub == 0) {
        const float y = fminf(fmaxf(a.centers[bin * A + grp] + part, cl), ch) * sc + sh;
        unsigned yb = __float_as_uint(y);
        yb = bad ? 0x7FC00000u : yb;
        ((unsigned*)a.actions)[row * A + grp] = yb;
      }
      if (a.probs) a.probs[row * BET_V + lane] = p / S;
      if (lane == 0) {
        a.bins[row] = bad ? -1 : bin;
        if (a.u_out) a.u_out[row] = u;
      }
    }
  }
}

}  // namespace d3il
