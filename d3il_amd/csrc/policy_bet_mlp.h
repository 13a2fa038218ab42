// policy_bet_mlp.h - the whole inference of the batched BeT-MLP policy (policies.BeTMLPPolicy; agents/bet_mlp_agent.py:366-406 around BeTPolicy.generate_latents,
// same file 114-147, KMeansDiscretizer.decode_actions and common/mlp.py ResidualMLPNetwork) as ONE kernel.  Included by rollout.hip behind policy_resmlp.h: the trunk
// is k_resmlp_f32's, with rm_layer from that header and the rest as text of its own (see the note on k_resmlp_f32 there), the draw is steps 3 - 5 of policy_bet.h in
// the same order of operations (bet_wave_max; the random stream, the bit test and the inverse scaling policy_unscale_f64: policy_common.h).
//
// For environment n (s = the scaled state row, H = hidden width, V = 64 bins, the network a Mish ResidualMLPNetwork with a V (1 + A)-row output layer WITH bias):
//   1. h = input layer and residual blocks on s                                   (f32)
//   2. logit_v = w_out[v] . h + b_out[v], v < 64
//   3. p_v = exp(logit_v - max), S = sum p, c_v = inclusive prefix sums
//   4. u = 24 bits of philox4x32_10(seed, (env_offset + n, step word, BET_MLP_TAG)) (or u_in[n])
//   5. bin = min(#{v : c_v <= u S}, 63)                                           (inverse CDF: empty bins in front of the drawn one are skipped, 64 is never returned)
//   6. off_a = w_out[64 + bin A + a] . h + b_out[64 + bin A + a]                  (layout "(V A)": 1 / 64 of the offset rows are multiplied)
//   7. y_a = clamp(centers[bin][a] + off_a, lo_a, hi_a) scale_a + shift_a         (sum and clamp in f32; product and sum in f64 on the f32 operands, rounded once)
//
// Tiling: a workgroup of eight waves owns 16 rows.  The trunk is k_resmlp_f32's: the waves share the H / 16 output tiles of a layer, weights stream from L2, the
// activations go from layer to layer through LDS in B-operand order, one barrier per layer, the block count is a loop bound, the input layer is 32 columns (7 steps).
// The logit layer is four 16-row output tiles over K = H (waves 0 .. 3, one tile each); the 16 x 64 logits with their bias go to a padded LDS array behind one more
// barrier.  Then every wave serves two of the 16 rows, lane = bin: wave max, exp, six-step shuffle scan, ballot + pop count.  The offsets: eight lanes per action
// component (group a = lane / 8), lane sub = lane % 8 takes the float4 chunks sub, sub + 8, .. of row 64 + bin A + a - read row-major from global memory (at most
// 576 x 256 x 4 B, it stays in L2) - against the final hidden row read back from LDS, three shuffle steps per group, no divergent branch in front of a shuffle
// (groups beyond A repeat component A - 1).
//
// LDS: xb 2 x NT x 64 float4 (16 / 32 KB; xb[t][lane (g, j)] = features 16 t + 4 g + r of row j), lg 16 x 65 words.  Plain C++, the matrix-core builtin and vector
// stores only; no atomics, no scratch; every branch in front of a barrier depends on the wave index or on kernel arguments only.  NaN / Inf: the device pass is
// built with -ffinite-math-only, so the state row, the final hidden row and the logits are tested on their bit patterns (policy_nonfinite); a hit gives
// bins = -1 and 0x7FC00000 in every action component of that environment by integer selects.  The row's arithmetic still runs (on garbage), no index depends on it
// beyond bin, which the pop count bounds to 0 .. 63.  Rows never mix: column j of every matrix-core product is row j.
#pragma once

namespace d3il {

constexpr unsigned BET_MLP_TAG = 0x424D4C50u;      // fourth counter word: never 0, never BET_TAG, never a DDPM_GPT_TAG, IBC_TAG, ACT_TAG, CVAE_TAG or DDPM_ACT_TAG word
constexpr int BM_V = 64, BM_AMAX = 8, BM_OBSMAX = 28, BM_LSTRIDE = 65;

struct BetMlpArgs {
  const float* state; const float* w_in; const float* b_in; const float* w_blk; const float* b_blk; const float* w_logit; const float* b_logit;
  const float* w_off; const float* b_off; const float* centers;
  const float* lo; const float* hi; const float* scale; const float* shift;
  const unsigned* t_dev; const float* u_in;
  float* actions; int* bins; float* u_out; float* probs;
  unsigned long long seed, env_offset;
  long n_env;
  int obs, A, nblk;
};

template <int HID>
__global__ __launch_bounds__(512) void k_bet_mlp(BetMlpArgs a) {
  constexpr int NT = HID / 16, TPW = NT / 8, LAYER_F4 = NT * NT * 64;
  __shared__ mlp_f4 xb[2][NT * 64];
  __shared__ float lg[16 * BM_LSTRIDE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const int OBS = a.obs, A = a.A, nblk = a.nblk;
  const long n = a.n_env;
  const long rowj = (long)blockIdx.x * 16 + j;
  const long rj = rowj < n ? rowj : (n - 1);
  // ---- 1. the trunk, as k_resmlp_f32: lane (g, j) holds feature 4 s2 + g of row j
  float in_k[7];
#pragma unroll
  for (int s2 = 0; s2 < 7; s2++) { const int f = 4 * s2 + g; in_k[s2] = f < OBS ? a.state[rj * OBS + f] : 0.f; }
  unsigned bad_in = 0u;
#pragma unroll
  for (int s2 = 0; s2 < 7; s2++) bad_in |= (unsigned)policy_nonfinite(in_k[s2]);
  bad_in |= (unsigned)__shfl_xor((int)bad_in, 16); bad_in |= (unsigned)__shfl_xor((int)bad_in, 32);      // every wave, every lane of column j: the verdict on row j's state
  const mlp_f4* w_in4 = (const mlp_f4*)a.w_in;
  mlp_f4 xo[TPW];
#pragma unroll
  for (int q = 0; q < TPW; q++) {
    const int To = TPW * w + q;
    mlp_f4 acc = *(const mlp_f4*)(a.b_in + 16 * To + 4 * g);
    const mlp_f4 a0 = w_in4[(To * 64 + lane) * 2], a1 = w_in4[(To * 64 + lane) * 2 + 1];
#pragma unroll
    for (int s2 = 0; s2 < 7; s2++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s2 < 4 ? a0[s2] : a1[s2 - 4], in_k[s2], acc, 0, 0, 0);
    xo[q] = acc;
  }
  int buf = 0;
#pragma clang loop unroll(disable)
  for (int b = 0; b < nblk; b++) {
    mlp_f4 y[TPW];
#pragma unroll
    for (int q = 0; q < TPW; q++) xb[buf][(TPW * w + q) * 64 + lane] = mlp_f4{dd_mish(xo[q][0]), dd_mish(xo[q][1]), dd_mish(xo[q][2]), dd_mish(xo[q][3])};
    __syncthreads();
    rm_layer<HID, false>((const mlp_f4*)a.w_blk + (long)(2 * b) * LAYER_F4, a.b_blk + (2 * b) * HID, xb[buf], y, w, lane, g);
    buf ^= 1;
#pragma unroll
    for (int q = 0; q < TPW; q++) xb[buf][(TPW * w + q) * 64 + lane] = mlp_f4{dd_mish(y[q][0]), dd_mish(y[q][1]), dd_mish(y[q][2]), dd_mish(y[q][3])};
    __syncthreads();
    rm_layer<HID, true>((const mlp_f4*)a.w_blk + (long)(2 * b + 1) * LAYER_F4, a.b_blk + (2 * b + 1) * HID, xb[buf], xo, w, lane, g);
    buf ^= 1;
  }
#pragma unroll
  for (int q = 0; q < TPW; q++) xb[buf][(TPW * w + q) * 64 + lane] = xo[q];
  __syncthreads();
  // ---- 2. the logit layer: wave T < 4 owns bins 16 T .. 16 T + 15; lane (g, j), register r = bin 16 T + 4 g + r of row j
  if (w < 4) {
    const mlp_f4* wl = (const mlp_f4*)a.w_logit + (long)w * (NT * 64) + lane;
    mlp_f4 acc = *(const mlp_f4*)(a.b_logit + 16 * w + 4 * g), acc2 = mlp_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const mlp_f4 a4 = wl[t * 64], m4 = xb[buf][t * 64 + lane];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0], m4[0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1], m4[1], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[2], m4[2], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[3], m4[3], acc2, 0, 0, 0);
    }
    acc += acc2;
#pragma unroll
    for (int r = 0; r < 4; r++) lg[j * BM_LSTRIDE + 16 * w + 4 * g + r] = acc[r];
  }
  __syncthreads();
  // ---- 3 - 7. the draw and the tail: wave w serves rows 2 w and 2 w + 1 of the tile, lane = bin
  const int grp = lane >> 3, sub = lane & 7;      // offset products: component grp, chunk phase sub
  const bool comp = grp < A;
  const int cg = comp ? grp : A - 1;
  const float cl = a.lo[cg], ch = a.hi[cg], sc = a.scale[cg], sh = a.shift[cg];
  const unsigned t = *a.t_dev;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const int jr = 2 * w + k;
    const long row = (long)blockIdx.x * 16 + jr;
    const bool live = row < n;
    const long rr = live ? row : (n - 1);
    const float logit = lg[jr * BM_LSTRIDE + lane];
    const bool bad_s = __shfl((int)bad_in, jr) != 0;
    const bool bad_l = __ballot(policy_nonfinite(logit)) != 0ull;      // (every ballot stands on its own line: none sits behind a short-circuit)
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
      unsigned r4[4];
      policy_philox(a.seed, ge, t, BET_MLP_TAG, r4);
      u = policy_uniform24(r4[0]);
    }
    const int cnt = __popcll(__ballot(c <= u * S));
    const int bin = cnt < BM_V - 1 ? cnt : BM_V - 1;
    // ---- 6. offsets of the drawn bin (no divergent branch in front of the shuffles: groups beyond A repeat component A - 1)
    float part = 0.f;
    unsigned hb = 0u;
    const float* wo = a.w_off + ((long)bin * A + cg) * HID;
#pragma unroll
    for (int jj = 0; jj < HID / 32; jj++) {
      const int q = sub + 8 * jj;      // features 4 q .. 4 q + 3 of the final hidden row: tile q / 4, lane group q % 4
      const mlp_f4 wv = *(const mlp_f4*)(wo + 4 * q), xv = xb[buf][(q >> 2) * 64 + (q & 3) * 16 + jr];
      hb |= (unsigned)policy_nonfinite(xv[0]) | (unsigned)policy_nonfinite(xv[1]) | (unsigned)policy_nonfinite(xv[2]) | (unsigned)policy_nonfinite(xv[3]);
      part += fmaf(wv[3], xv[3], fmaf(wv[2], xv[2], fmaf(wv[1], xv[1], wv[0] * xv[0])));
    }
    __builtin_amdgcn_wave_barrier();
    part += __shfl_xor(part, 1); part += __shfl_xor(part, 2); part += __shfl_xor(part, 4);
    __builtin_amdgcn_wave_barrier();
    const bool bad_h = __ballot(hb != 0u) != 0ull;      // (the eight lanes of a group read the whole hidden row between them)
    const bool bad = bad_s | bad_l | bad_h;
    // ---- 7. the action
    if (live) {
      if (comp && sub == 0) {
        const float v = a.centers[bin * A + grp] + (part + a.b_off[bin * A + grp]);
        const unsigned yb = __float_as_uint(policy_unscale_f64(v, cl, ch, sc, sh));
        ((unsigned*)a.actions)[row * A + grp] = bad ? 0x7FC00000u : yb;
      }
      if (a.probs) a.probs[row * BM_V + lane] = p / S;
      if (lane == 0) {
        a.bins[row] = bad ? -1 : bin;
        if (a.u_out) a.u_out[row] = u;
      }
    }
  }
}

}  // namespace d3il
