// policy_ddpm_mlp.h - the whole reverse chain of the batched DDPM-MLP policy (policies.DDPMNativePolicy; agents/ddpm_agent.py:213-274 around gc_diffusion.py:101-216
// over diffusion_models.py:20-118 and common/mlp.py ResidualMLPNetwork) as ONE kernel, on the Philox stream.  Included by rollout.hip behind policy_resmlp.h, whose
// pieces the denoiser is built from (the random stream, the bit test and the inverse scaling: policy_common.h).  k_ddpm_mlp_f32 (policy_f32.h) is the older
// chain for one shape with its noise in an HBM tensor; it stays as it is.
//
// For environment n (s = the scaled state row, x the iterate of width A, f32 throughout; sched [T][5] = (sra, srm1, c1, c2, sig) of policies.ddpm_schedule, sig[0] = 0):
//   1. x = z_0
//   2. for i = T - 1 .. 0:  eps = ResidualMLP([x | temb[i] | s])                    (column order x, time, state: DiffusionMLP.forward)
//                           x0  = clamp(sra[i] x - srm1[i] eps, lo, hi)
//                           x   = (c1[i] x0 + c2[i] x) + sig[i] z_k                 (k = 1 + (T - 1 - i); step i = 0 draws nothing and adds nothing)
//   3. actions[n, a] = clamp(x_a, lo_a, hi_a) scale_a + shift_a                     (product and sum in f32, each rounded: the tail of DDPMGPTPolicy)
// z_k: noise_in[k][n][a] or Box-Muller on philox4x32_10(seed, (env_offset + n, step word, DDPM_MLP_TAG | k << 1 | q)), component a = 4 q + m takes word m; the
// second call (q = 1) is made only where A > 4.  T draws per call: k = 0 .. T - 1.
//
// Tiling: policy_resmlp.h's (16 rows per workgroup of eight waves, activations through LDS, one barrier per layer).  What differs from k_cvae_decode: (a) the input
// layer is split by what its columns depend on.  The time embedding's share W_in[:, temb] temb[i] + b_in is the same for every row: the packer makes it a bias
// table tbias [T][HID].  The state's share W_in[:, state] s does not change along the chain: the 64-column input layer without its bias (rm_input64) once, held
// in TPW float4 per wave.  Per step the input layer is the A <= 8 columns of x: two matrix-core steps on weights held in registers.  That
// changes the summation order of the input layer only.  (b) Every wave computes the output tile and every lane keeps its row's x (as k_ddpm_mlp_f32): no barrier
// between the output layer and the next input layer.  (c) The noise is drawn ONCE per workgroup: wave 0 (lane j of each lane group: row j; one or two Philox calls,
// two or four Box-Muller pairs) draws z_k in front of the barrier the step has anyway and shares it through 1 KB of LDS, double-buffered by the parity of k so that
// a chain without blocks (one barrier per step) does not overwrite what a slower wave still reads.  The alternative - every lane of all eight waves draws its row's
// normals - makes 512 lanes do the work of 16 and puts two waves' worth of logf / sincosf on every SIMD per step; one wave's draw in front of a barrier costs the
// other waves the wait and nothing else.  (d) The step word comes from device memory; the tail is fused.
//
// LDS: xb 2 x NT x 64 float4 (16 / 32 KB), zs 2 x 16 x 8 floats (1 KB).  Vector stores only, no inline assembly beyond the empty register barrier of
// policy_nonfinite; every branch in front of a barrier or shuffle depends on the wave index or on kernel arguments only.  NaN / Inf: the device pass is built with
// -ffinite-math-only and fminf(fmaxf(..)) returns its bound for a NaN, so the state row, every draw the row uses, every eps and the final x are tested on their bit
// patterns (exponent field all ones); a hit sets bad[n] and gives 0x7FC00000 in every action component of that environment by an integer select.  The row's
// arithmetic still runs; rows never mix (column j of every matrix-core product is row j), so no other row changes and finite rows come out bit for bit as without
// the test.
//
// Resources (hipcc 7.2, gfx950, the flags of build.py, -Rpass-analysis=kernel-resource-usage):
//   k_ddpm_mlp_chain<128>: 125 VGPRs, 0 AGPRs, 106 SGPRs (12 spilled to VGPR lanes), scratch 0, LDS 17408 B, occupancy 4 waves / SIMD (two workgroups per CU)
//   k_ddpm_mlp_chain<256>: 215 VGPRs, 0 AGPRs, 106 SGPRs (15 spilled to VGPR lanes), scratch 0, LDS 33792 B, occupancy 2 waves / SIMD (one workgroup per CU)
// The SGPR spills are the per-component bounds and output biases (24 uniform values) next to 25 kernel arguments; they go to lanes of a VGPR, not to memory.
#pragma once

namespace d3il {

constexpr unsigned DDPM_MLP_TAG = 0x444D0000u;      // fourth counter word = TAG | k << 1 | q (k < 256, q < 2): an upper half no other tag has
constexpr int DM_AMAX = 8, DM_INMAX = 64, DM_TMAX = 255;

struct DdpmMlpArgs {
  const unsigned* t_dev; const float* state; const float* w_x; const float* w_s; const float* tbias; const float* w_blk; const float* b_blk; const float* w_out;
  const float* b_out; const float* sched; const float* lo; const float* hi; const float* scale; const float* shift; const float* noise_in;
  float* actions; int* bad; float* noise_out;
  unsigned long long seed, env_offset;
  long n_env;
  int obs, A, T, nblk;
};

template <int HID>
__global__ __launch_bounds__(512) void k_ddpm_mlp_chain(DdpmMlpArgs a) {
  constexpr int NT = HID / 16, TPW = NT / 8;
  __shared__ mlp_f4 xb[2][NT * 64];
  __shared__ mlp_f4 zs[2][16 * 2];      // the 16 rows' draw z_k, [k & 1][row][8]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const int OBS = a.obs, A = a.A, T = a.T, nblk = a.nblk;
  const long n = a.n_env;
  const long row = (long)blockIdx.x * 16 + j;
  const bool live = row < n;
  const long rr = live ? row : (n - 1);
  const unsigned tw = *a.t_dev;
  // z_k of row j by wave 0, into zs[k & 1] (and noise_out[k]); k = T: the last step draws nothing, noise_out gets zeros
  auto draw = [&](int k) {
    float z[DM_AMAX];
    if (k >= T) {
#pragma unroll
      for (int c = 0; c < DM_AMAX; c++) z[c] = 0.f;
    } else if (a.noise_in) {
#pragma unroll
      for (int c = 0; c < DM_AMAX; c++) z[c] = c < A ? a.noise_in[((long)k * n + rr) * A + c] : 0.f;
    } else {
      const unsigned long long ge = a.env_offset + (unsigned long long)rr;
      const unsigned tag = DDPM_MLP_TAG | ((unsigned)k << 1);
      unsigned r[4];
      policy_philox(a.seed, ge, tw, tag, r);
      policy_box_muller(r[0], r[1], z[0], z[1]); policy_box_muller(r[2], r[3], z[2], z[3]);
      if (A > 4) {
        policy_philox(a.seed, ge, tw, tag | 1u, r);
        policy_box_muller(r[0], r[1], z[4], z[5]); policy_box_muller(r[2], r[3], z[6], z[7]);
      } else {
        z[4] = z[5] = z[6] = z[7] = 0.f;
      }
    }
    if (g == 0) {      // (the four lane groups hold the same sixteen rows: one of them stores)
      if (k < T) {
        zs[k & 1][2 * j] = mlp_f4{z[0], z[1], z[2], z[3]};
        zs[k & 1][2 * j + 1] = mlp_f4{z[4], z[5], z[6], z[7]};
      }
      if (a.noise_out && live) {
#pragma unroll
        for (int c = 0; c < DM_AMAX; c++)
          if (c < A) a.noise_out[((long)k * n + row) * A + c] = z[c];
      }
    }
  };
  if (w == 0) draw(0);
  // ---- the state's share of the input layer, once: lane (g, j) holds feature 4 s2 + g of row j
  float lo[DM_AMAX], hi[DM_AMAX], bo[DM_AMAX];
#pragma unroll
  for (int c = 0; c < DM_AMAX; c++) { lo[c] = c < A ? a.lo[c] : 0.f; hi[c] = c < A ? a.hi[c] : 0.f; bo[c] = a.b_out[c]; }      // (b_out is padded to 16)
  unsigned bad = 0u;
  mlp_f4 xs[TPW];
  float wx[TPW][2];
  {
    float st_k[16];
#pragma unroll
    for (int s2 = 0; s2 < 16; s2++) { const int f = 4 * s2 + g; st_k[s2] = f < OBS ? a.state[rr * OBS + f] : 0.f; }
#pragma unroll
    for (int s2 = 0; s2 < 16; s2++) bad |= (unsigned)policy_nonfinite(st_k[s2]);
    rm_input64<HID, false>(a.w_s, nullptr, st_k, xs, w, lane, g);      // (no bias: it is in tbias)
#pragma unroll
    for (int q = 0; q < TPW; q++) {
      const int To = TPW * w + q;
      wx[q][0] = a.w_x[(To * 64 + lane) * 2];
      wx[q][1] = a.w_x[(To * 64 + lane) * 2 + 1];
    }
  }
  bad = rm_row_or(bad);
  __syncthreads();
  // ---- 1. x = z_0: every lane keeps its row's iterate
  float x[DM_AMAX];
  {
    const mlp_f4 za = zs[0][2 * j], zb = zs[0][2 * j + 1];
#pragma unroll
    for (int c = 0; c < 4; c++) { x[c] = za[c]; x[4 + c] = zb[c]; }
#pragma unroll
    for (int c = 0; c < DM_AMAX; c++) bad |= (unsigned)policy_nonfinite(x[c]);
  }
  int buf = 0;
  // ---- 2. the reverse chain
#pragma clang loop unroll(disable)
  for (int step = 0; step < T; step++) {
    const int i = T - 1 - step, k = step + 1;
    const float xk0 = g == 0 ? x[0] : (g == 1 ? x[1] : (g == 2 ? x[2] : x[3])), xk1 = g == 0 ? x[4] : (g == 1 ? x[5] : (g == 2 ? x[6] : x[7]));
    mlp_f4 xo[TPW];      // the wave's tiles of the residual stream
#pragma unroll
    for (int q = 0; q < TPW; q++) {
      const int To = TPW * w + q;
      mlp_f4 acc = *(const mlp_f4*)(a.tbias + (long)i * HID + 16 * To + 4 * g);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wx[q][0], xk0, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wx[q][1], xk1, acc, 0, 0, 0);
      xo[q] = acc + xs[q];
    }
    rm_blocks<HID>(a.w_blk, a.b_blk, nblk, xb, xo, buf, w, lane, g);
    rm_store<HID, false>(xb[buf], xo, w, lane);
    if (w == 0) draw(k);      // z_k of this step's update (k = T: zeros to noise_out only), in front of the barrier the output layer needs anyway
    __syncthreads();
    const mlp_f4 acc = rm_tile<HID>((const mlp_f4*)a.w_out, xb[buf], mlp_f4{0.f, 0.f, 0.f, 0.f}, lane);      // (every wave: each keeps its rows' x)
    buf ^= 1;
    // epsilon of row j sits in lanes (0, j) and (1, j), registers 0 .. 3: every lane group of every wave takes it and does the same update on its copy of x
    float e[DM_AMAX];
#pragma unroll
    for (int c = 0; c < DM_AMAX; c++) e[c] = __shfl(acc[c & 3], ((c >> 2) << 4) + j) + bo[c];
    const float sra = a.sched[i * 5], srm1 = a.sched[i * 5 + 1], c1 = a.sched[i * 5 + 2], c2 = a.sched[i * 5 + 3], sig = a.sched[i * 5 + 4];
    float z[DM_AMAX];
    if (i > 0) {      // (uniform: the loop counter)
      const mlp_f4 za = zs[k & 1][2 * j], zb = zs[k & 1][2 * j + 1];
#pragma unroll
      for (int c = 0; c < 4; c++) { z[c] = za[c]; z[4 + c] = zb[c]; }
    } else {
#pragma unroll
      for (int c = 0; c < DM_AMAX; c++) z[c] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < DM_AMAX; c++) {
      bad |= c < A ? ((unsigned)policy_nonfinite(e[c]) | (unsigned)policy_nonfinite(z[c])) : 0u;
      const float p = fminf(fmaxf(sra * x[c] - srm1 * e[c], lo[c]), hi[c]);      // clipped x0 prediction
      const float xn = (c1 * p + c2 * x[c]) + sig * z[c];
      x[c] = c < A ? xn : 0.f;
    }
  }
  // ---- 3. the tail: lane (0, j) of wave 0 stores row j
  if (live && w == 0 && g == 0) {
#pragma unroll
    for (int c = 0; c < DM_AMAX; c++) bad |= c < A ? (unsigned)policy_nonfinite(x[c]) : 0u;
#pragma unroll
    for (int c = 0; c < DM_AMAX; c++) {
      if (c < A) {
        const unsigned yb = __float_as_uint(policy_unscale_f32(x[c], lo[c], hi[c], a.scale[c], a.shift[c]));
        ((unsigned*)a.actions)[row * A + c] = bad ? 0x7FC00000u : yb;
      }
    }
    a.bad[row] = bad ? 1 : 0;
  }
}

}  // namespace d3il
