// policy_bc_gmm.h - the whole inference of the batched BC-GMM policy (policies.BCGMMPolicy; agents/models/gmm/bc_gmm.py:13-90 around common/mlp.py ResidualMLPNetwork,
// sampled once per step as BC_Agent.predict, agents/bc_agent.py:240-271, would with model(state).sample()) as ONE kernel.  Included by rollout.hip behind
// policy_bet_mlp.h: the trunk is built from the pieces of policy_resmlp.h, the categorical draw is k_bet_mlp's in the same order of operations (bet_wave_max), the
// normals are policy_box_muller, the inverse scaling policy_unscale_f64 (with the random stream and the bit test: policy_common.h).
//
// For environment n (s = the scaled state row, H = hidden width = mlp_output_dim, G = n_gaussians <= 64, A = output_dim <= 8):
//   1. h = input layer and residual blocks on s                                        (f32)
//   2. f = Mish(W_o h + b_o)                                                           (the ResidualMLP's own output layer: no activation in front of it, mlp_output_act behind it)
//   3. logit_g = w_logit[g] . f + b_logit[g], g < G
//   4. p_g = exp(logit_g - max), c = inclusive prefix sums, S = c_{G-1};  u = 24 bits of word 0 of philox4x32_10(seed, (env_offset + n, step word, BC_GMM_TAG | 0)) (or u_in[n])
//      k = min(#{g < G : c_g <= u S}, G - 1)                                           (lanes g >= G take no part in the max, the sum, the count or the bit test)
//   5. mean_a = 0.01 tanh(w_mean[k A + a] . f + b_mean[k A + a])                       (layout "(G A)": 1 / G of the head rows are multiplied)
//   6. std_a = 1e-4 (std_mode 0: low_noise_eval, w_std is never read), or act(w_std[k A + a] . f + b_std[k A + a]) + min_std with act = exp (1) or torch's softplus (2)
//   7. x_a = mean_a + std_a z_a (product and sum rounded separately), z_a = z_in[n][a] or Box-Muller on the words of call q = 1 + a / 4 (tag BC_GMM_TAG | q), component
//      a = 4 (q - 1) + m from word m - words 0, 1 -> the cos and sin of one pair, words 2, 3 the other, as the CVAE latent
//   8. y_a = clamp(x_a, lo_a, hi_a) scale_a + shift_a                                  (clamp in f32; product and sum in f64 on the f32 operands, rounded once)
//
// Tiling: k_bet_mlp's, the trunk policy_resmlp.h's with the 28-column input layer.  One more square layer than k_bet_mlp - the trunk's output layer, no residual,
// Mish behind it.  The logit layer is ceil(G / 16) output tiles (wave T < ceil(G / 16), one tile each; the waves up to 3 beyond write
// zeros, so that no LDS word is read unwritten); 16 x 64 logits go to a padded LDS array
// behind one more barrier.  Then every wave serves two of the 16 rows: lane = component for the draw, and for the head rows eight lanes per action component
// (group a = lane / 8; lane sub = lane % 8 takes the float4 chunks sub, sub + 8, .. of row k A + a, read row-major from global memory - at most 2 x 512 x 256 x 4 B,
// it stays in L2) against f read back from LDS, three shuffle steps per group; groups beyond A repeat component A - 1, every lane makes its group's Philox call.
//
// LDS: xb 2 x NT x 64 float4 (16 / 32 KB), lg 16 x 65 words.  Plain C++, the matrix-core builtin and vector stores only; no atomics, no scratch; every branch in
// front of a barrier or shuffle depends on the wave index, the loop counter or kernel arguments (G, std_mode, the u_in / z_in pointers) only.  NaN / Inf: the device
// pass is built with -ffinite-math-only - tanhf, expf and the fminf / fmaxf clamp may turn a NaN into a finite number there -, so the state row, f, the logits
// g < G, the selected raw mean and raw std, the std itself (an overflowing exp) and the normals that are used are tested on their bit patterns
// (policy_nonfinite); a hit gives comps = -1 and 0x7FC00000 in every action component of that environment by integer selects.  The row's arithmetic still runs
// (on garbage); no index depends on it beyond k, which the pop count bounds to 0 .. G - 1.  Rows never mix: column j of every matrix-core product is row j.
#pragma once

namespace d3il {

constexpr unsigned BC_GMM_TAG = 0x474D0000u;      // fourth counter word = TAG | q (q = 0: the uniform, q = 1, 2: the normals); its upper half is no other tag's
constexpr int BG_GMAX = 64, BG_AMAX = 8, BG_OBSMAX = 28, BG_LSTRIDE = 65;
constexpr int BG_STD_LOW_NOISE = 0, BG_STD_EXP = 1, BG_STD_SOFTPLUS = 2;

struct BcGmmArgs {
  const unsigned* t_dev; const float* state; const float* w_in; const float* b_in; const float* w_blk; const float* b_blk; const float* w_feat; const float* b_feat;
  const float* w_logit; const float* b_logit; const float* w_mean; const float* b_mean; const float* w_std; const float* b_std;
  const float* lo; const float* hi; const float* scale; const float* shift;
  const float* u_in; const float* z_in;
  float* actions; int* comps; float* u_out; float* z_out; float* probs;
  unsigned long long seed, env_offset;
  long n_env;
  float min_std;
  int obs, G, A, nblk, std_mode;
};

template <int HID>
__global__ __launch_bounds__(512) void k_bc_gmm(BcGmmArgs a) {
  constexpr int NT = HID / 16, TPW = NT / 8;
  __shared__ mlp_f4 xb[2][NT * 64];
  __shared__ float lg[16 * BG_LSTRIDE];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const int OBS = a.obs, G = a.G, A = a.A, nblk = a.nblk, std_mode = a.std_mode;
  const long n = a.n_env;
  const long rowj = (long)blockIdx.x * 16 + j;
  const long rj = rowj < n ? rowj : (n - 1);
  // ---- 1. the trunk, as k_resmlp_f32: lane (g, j) holds feature 4 s2 + g of row j
  float in_k[7];
  rm_load_row28(a.state, rj, OBS, g, in_k);
  unsigned bad_in = 0u;
#pragma unroll
  for (int s2 = 0; s2 < 7; s2++) bad_in |= (unsigned)policy_nonfinite(in_k[s2]);
  bad_in = rm_row_or(bad_in);      // every wave, every lane of column j: the verdict on row j's state
  mlp_f4 xo[TPW];
  rm_input28<HID>(a.w_in, a.b_in, in_k, xo, w, lane, g);
  int buf = 0;
  rm_blocks<HID>(a.w_blk, a.b_blk, nblk, xb, xo, buf, w, lane, g);
  // ---- 2. the trunk's output layer on h as it is, Mish behind it: f
  rm_store<HID, false>(xb[buf], xo, w, lane);
  __syncthreads();
  rm_layer<HID, false>((const mlp_f4*)a.w_feat, a.b_feat, xb[buf], xo, w, lane, g);
  buf ^= 1;
  rm_store<HID, true>(xb[buf], xo, w, lane);
  __syncthreads();
  // ---- 3. the logit layer: wave T < ceil(G / 16) owns components 16 T .. 16 T + 15; lane (g, j), register r = component 16 T + 4 g + r of row j
  if (w < 4) {
    mlp_f4 acc = mlp_f4{0.f, 0.f, 0.f, 0.f};
    if (16 * w < G) acc = rm_tile<HID>((const mlp_f4*)a.w_logit + (long)w * (NT * 64), xb[buf], *(const mlp_f4*)(a.b_logit + 16 * w + 4 * g), lane);
#pragma unroll
    for (int r = 0; r < 4; r++) lg[j * BG_LSTRIDE + 16 * w + 4 * g + r] = acc[r];
  }
  __syncthreads();
  // ---- 4 - 8. the draws and the tail: wave w serves rows 2 w and 2 w + 1 of the tile
  const int grp = lane >> 3, sub = lane & 7;      // head rows: component grp, chunk phase sub
  const bool comp = grp < A, on = lane < G;
  const int cg = comp ? grp : A - 1;
  const float cl = a.lo[cg], ch = a.hi[cg], sc = a.scale[cg], sh = a.shift[cg];
  const unsigned t = *a.t_dev;
#pragma unroll
  for (int k2 = 0; k2 < 2; k2++) {
    const int jr = 2 * w + k2;
    const long row = (long)blockIdx.x * 16 + jr;
    const bool live = row < n;
    const long rr = live ? row : (n - 1);
    const float lraw = lg[jr * BG_LSTRIDE + lane];
    const float logit = on ? lraw : -3.4028234663852886e38f;      // (a masked lane: no finite logit lies below it; its numerator is set to 0 and it is not tested)
    const bool bad_s = __shfl((int)bad_in, jr) != 0;
    const bool bad_l = __ballot(on && policy_nonfinite(lraw)) != 0ull;      // (every ballot stands on its own line: none sits behind a short-circuit)
    // ---- 4. softmax numerators, their prefix sums, the uniform, the component
    const float pe = expf(logit - bet_wave_max(logit));
    const float p = on ? pe : 0.f;
    float c = p;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) { const float up = __shfl_up(c, s); c += lane >= s ? up : 0.f; }
    const float S = __shfl(c, 63);
    const unsigned long long ge = a.env_offset + (unsigned long long)rr;
    float u;
    if (a.u_in) u = a.u_in[rr];
    else {
      unsigned r4[4];
      policy_philox(a.seed, ge, t, BC_GMM_TAG, r4);
      u = policy_uniform24(r4[0]);
    }
    const bool below = on && c <= u * S;
    const int cnt = __popcll(__ballot(below));
    const int k = cnt < G - 1 ? cnt : G - 1;
    // ---- 7a. this group's normal
    float z;
    if (a.z_in) z = a.z_in[rr * A + cg];
    else {
      unsigned r4[4];
      policy_philox(a.seed, ge, t, BC_GMM_TAG | (unsigned)(1 + (cg >> 2)), r4);
      const bool second = (cg & 2) != 0;
      float n0, n1;
      policy_box_muller(second ? r4[2] : r4[0], second ? r4[3] : r4[1], n0, n1);
      z = (cg & 1) ? n1 : n0;
    }
    // ---- 5, 6. the head rows of the drawn component (no divergent branch in front of the shuffles: groups beyond A repeat component A - 1)
    const long hr = (long)k * A + cg;
    float pm = rm_row_part<HID>(a.w_mean + hr * HID, xb[buf], sub, jr), ps = 0.f;
    if (std_mode != BG_STD_LOW_NOISE) ps = rm_row_part<HID>(a.w_std + hr * HID, xb[buf], sub, jr);
    unsigned hb = 0u;
#pragma unroll
    for (int jj = 0; jj < HID / 32; jj++) {
      const int q = sub + 8 * jj;
      const mlp_f4 xv = xb[buf][(q >> 2) * 64 + (q & 3) * 16 + jr];
      hb |= (unsigned)policy_nonfinite(xv[0]) | (unsigned)policy_nonfinite(xv[1]) | (unsigned)policy_nonfinite(xv[2]) | (unsigned)policy_nonfinite(xv[3]);
    }
    __builtin_amdgcn_wave_barrier();
    pm += __shfl_xor(pm, 1); pm += __shfl_xor(pm, 2); pm += __shfl_xor(pm, 4);
    ps += __shfl_xor(ps, 1); ps += __shfl_xor(ps, 2); ps += __shfl_xor(ps, 4);
    __builtin_amdgcn_wave_barrier();
    const float mraw = pm + a.b_mean[hr];
    const float mean = 0.01f * tanhf(mraw);
    float sraw = 0.f, sd = 1e-4f;
    if (std_mode != BG_STD_LOW_NOISE) {
      sraw = ps + a.b_std[hr];
      const float act = std_mode == BG_STD_EXP ? expf(sraw) : (sraw > 20.f ? sraw : log1pf(expf(sraw)));
      sd = act + a.min_std;
    }
    hb |= (unsigned)policy_nonfinite(mraw) | (unsigned)policy_nonfinite(sraw) | (unsigned)policy_nonfinite(sd) | (unsigned)policy_nonfinite(z);
    const bool bad_h = __ballot(hb != 0u) != 0ull;      // (the eight lanes of a group read the whole feature row between them; every group is a used component)
    const bool bad = bad_s | bad_l | bad_h;
    // ---- 7b. the sample, 8. the action
    const float x = __fadd_rn(mean, __fmul_rn(sd, z));
    if (live) {
      if (comp && sub == 0) {
        const unsigned yb = __float_as_uint(policy_unscale_f64(x, cl, ch, sc, sh));
        ((unsigned*)a.actions)[row * A + grp] = bad ? 0x7FC00000u : yb;
        if (a.z_out) a.z_out[row * A + grp] = z;
      }
      if (a.probs && on) a.probs[row * G + lane] = p / S;
      if (lane == 0) {
        a.comps[row] = bad ? -1 : k;
        if (a.u_out) a.u_out[row] = u;
      }
    }
  }
}

}  // namespace d3il
