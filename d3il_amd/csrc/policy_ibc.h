// policy_ibc.h - the whole inference of the batched Implicit-BC policy (policies.IBCPolicy; agents/ibc_agent.py:248-286 around
// agents/models/ibc/samplers/langevin_mcmc.py:129-163,236-286 and agents/models/ibc/ebms.py:21-51 over common/mlp.py ResidualMLPNetwork) as ONE kernel
// (included by rollout.hip).
//
// For environment n, sample s < 64 and chain index k < K (E = the energy network on the row [state | x], Mish, no norm, in f32; the samples x themselves are carried
// in f64 and rounded to f32 where they enter the network - as the reference does, whose float64 bounds array promotes the samples at the first clamp while
// ResidualMLPNetwork.forward casts its input to f32; the f32 rounding of twenty updates of x would otherwise be the largest error of the chain):
//   1. x_a = x0_in[n, s, a], or lo_a + u (hi_a - lo_a) with u = 24 bits of philox4x32_10(seed, (env_offset + n, step word, IBC_TAG | s << 2 | q)), component a = 4 q + m
//   2. K times: g = dE/dx (forward pass that keeps the Mish derivatives, analytic backward pass down to the action columns of the input layer);
//      z_a = noise_scale * (noise_in[k, n, s, a] or Box-Muller on Philox with the fourth word IBC_TAG | 1 << 14 | k << 8 | s << 2 | q);
//      d_a = clamp(coef[k][0] g_a + coef[k][1] z_a, -clip_a, clip_a);  x_a = clamp(x_a - d_a, lo_a, hi_a)
//   3. E_s of the final x (forward only); p_s = exp(-(E_s - min E)), inclusive prefix sums c; u = u_in[n] or Philox with the fourth word IBC_TAG | 2 << 14;
//      pick = min(#{s : c_s <= u c_63}, 63); actions[n, a] = x[pick, a] scale_a + shift_a
// As torch ops one call is K autograd passes and one forward pass of the network on 64 rows per environment, with two dozen small kernels between them.
//
// Tiling.  A workgroup of eight waves owns ONE environment and walks its four row tiles of 16 samples one after the other, each through the whole chain; the
// samples (f64) and final energies of the 64 rows live in 4.3 KB of LDS, where wave 0 does step 3 - one launch, no atomics, no workspace.  Within a row tile the
// scheme is k_resmlp_f32's: the eight waves share the HID / 16 output tiles of a layer (wave w: tiles TPW w .. TPW (w + 1) - 1), the weights stream from L2, the
// activations go from layer to layer through LDS in B-operand order, one barrier per layer.  Backwards the SAME scheme runs on the packed transposes: output tile
// To of W^T lands on the lane and register that held pre-activation To in the forward pass, so the Mish derivatives of both pre-activations of every block stay in
// registers (2 TPW float4 per block, IBC_MAXB register sets picked by uniform selects) and are multiplied in place.  The chain starts from g = w_out (the energy's
// single output row) and ends with the 16-row tile of the input layer's action columns, which wave 0 computes; its lane (g, j) then owns components g and 4 + g of
// row j: noise, update, the new iterate into LDS, from where every lane takes its share of the next input row.
// Why one row tile at a time: two tiles would halve the L2 weight traffic but double the stored derivatives (128 registers at hidden 256 / 4 blocks, next to
// the 64 of a weight fragment set: past the 256 a wave of a 512-thread workgroup may hold); four tiles also need 128 KB of LDS.  DESIGN section 27.2.
//
// Vector stores only, no inline assembly beyond the empty register barrier of the bit tests, every branch in front of a shuffle or barrier is workgroup-uniform
// (kernel arguments only).  NaN / Inf: the device pass is built with -ffinite-math-only, so the state row, every start point, gradient, update, iterate and final
// energy is tested on its bit pattern (exponent field all ones); a hit anywhere in the environment gives picks = -1 and 0x7FC00000 in every action component.
#pragma once

namespace d3il {

constexpr unsigned IBC_TAG = 0x49420000u;      // fourth counter word = TAG | kind << 14 | k << 8 | s << 2 | q: never 0, never BET_TAG, never a DDPM_GPT_TAG word
constexpr int IBC_S = 64, IBC_AMAX = 8, IBC_KMAX = 63, IBC_MAXB = 4, IBC_NW = 8;
typedef float ibc_f4 __attribute__((ext_vector_type(4)));

// Mish and its derivative in dd_mish's form: n = e^x, p = n (n + 2), t = p / (p + 2); mish = x t, mish' = t + x 4 n (n + 1) / (p + 2)^2; x > 20: x and 1
__device__ __forceinline__ void ibc_mish(float x, float& m, float& d) {
  if (x > 20.f) { m = x; d = 1.f; return; }
  const float n = expf(x), p = n * (n + 2.f), q = p + 2.f, t = p / q;
  m = x * t;
  d = t + x * (4.f * n * (n + 1.f)) / (q * q);
}
__device__ __forceinline__ ibc_f4 ibc_mish4(const ibc_f4 x, ibc_f4& d) {
  ibc_f4 m;
#pragma unroll
  for (int r = 0; r < 4; r++) { float mm, dd; ibc_mish(x[r], mm, dd); m[r] = mm; d[r] = dd; }
  return m;
}
// the start point lo + u (hi - lo), every operation rounded to f32 (no contraction into a fused multiply-add: the host form is three separate f32 operations)
__device__ __forceinline__ float ibc_start(float lo, float hi, float u) {
#pragma clang fp contract(off)
  const float span = hi - lo;
  const float prod = u * span;
  return lo + prod;
}
// y[q] = (RES ? y[q] : 0) + (bias) + W m for the wave's output tiles TPW w + q of one packed HID x HID layer (xin: the 16 rows in LDS, B-operand order).
// Feature step t outside, the wave's tiles inside: one activation fragment is live at a time and the weight fragments stream through (few registers next to
// the stored derivatives).
template <int HID, bool BIAS, bool RES>
__device__ __forceinline__ void ibc_layer(const ibc_f4* __restrict__ wl, const float* __restrict__ bias, const ibc_f4* xin, ibc_f4* y, int w, int lane, int g) {
  constexpr int NT = HID / 16, TPW = NT / IBC_NW;
  const ibc_f4* const wt = wl + (long)(TPW * w) * (NT * 64) + lane;
  ibc_f4 acc[TPW][4];
#pragma unroll
  for (int q = 0; q < TPW; q++) {
    acc[q][0] = BIAS ? *(const ibc_f4*)(bias + 16 * (TPW * w + q) + 4 * g) : ibc_f4{0.f, 0.f, 0.f, 0.f};
    acc[q][1] = RES ? y[q] : ibc_f4{0.f, 0.f, 0.f, 0.f};
    acc[q][2] = ibc_f4{0.f, 0.f, 0.f, 0.f}; acc[q][3] = ibc_f4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const ibc_f4 m = xin[t * 64 + lane];
#pragma unroll
    for (int q = 0; q < TPW; q++) {
      const ibc_f4 a = wt[q * (NT * 64) + t * 64];
#pragma unroll
      for (int r = 0; r < 4; r++) acc[q][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], m[r], acc[q][r], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < TPW; q++) y[q] = (acc[q][0] + acc[q][1]) + (acc[q][2] + acc[q][3]);
}
// the derivatives of block b among the IBC_MAXB register sets: uniform selects (the block loops stay loops, the sets stay registers)
template <int TPW>
__device__ __forceinline__ void ibc_keep(ibc_f4 (*d)[TPW], int b, const ibc_f4* v) {
#pragma unroll
  for (int bb = 0; bb < IBC_MAXB; bb++)
#pragma unroll
    for (int q = 0; q < TPW; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) d[bb][q][r] = b == bb ? v[q][r] : d[bb][q][r];
}
template <int TPW>
__device__ __forceinline__ void ibc_take(const ibc_f4 (*d)[TPW], int b, ibc_f4* v) {
#pragma unroll
  for (int q = 0; q < TPW; q++) v[q] = d[0][q];
#pragma unroll
  for (int bb = 1; bb < IBC_MAXB; bb++)
#pragma unroll
    for (int q = 0; q < TPW; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) v[q][r] = b == bb ? d[bb][q][r] : v[q][r];
}

struct IbcArgs {
  const float* state; const float* w_in; const float* b_in; const float* w_blk; const float* b_blk; const float* w_out; const float* b_out;
  const float* wT_blk; const float* wT_act; const float* coef; const float* lo; const float* hi; const float* clip; const float* scale; const float* shift;
  const unsigned* t_dev; const float* x0_in; const float* noise_in; const float* u_in;
  float* actions; int* picks; float* x_final; float* energies; float* x0_out; float* noise_out; float* u_out;
  unsigned long long seed, env_offset;
  long n_env;
  float noise_scale;
  int obs, A, nblk, K;
};

template <int HID>
__global__ __launch_bounds__(64 * IBC_NW) void k_ibc_langevin(IbcArgs a) {
  constexpr int NT = HID / 16, TPW = NT / IBC_NW, LAYER_F4 = NT * NT * 64;
  __shared__ ibc_f4 xb[2][NT * 64];      // the 16 rows' activations / gradients, [t][lane] float4 = features 16 t + 4 g + r of row j
  __shared__ float se[IBC_S];            // the environment's 64 final energies
  __shared__ double sx[IBC_S * IBC_AMAX];      // and its 64 samples: the current iterate of the row tile in flight, the final one of those before it
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const int A = a.A, OBS = a.obs, nblk = a.nblk, K = a.K;
  const long n = blockIdx.x;      // (the grid is the environment count: no tail rows)
  const unsigned t_word = *a.t_dev;
  const unsigned long long ge = a.env_offset + (unsigned long long)n;
  const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32), c0 = (unsigned)ge, c1 = (unsigned)(ge >> 32);
  const ibc_f4* const w_in4 = (const ibc_f4*)a.w_in;
  const ibc_f4* const w_out4 = (const ibc_f4*)a.w_out;
  const ibc_f4* const wT_act4 = (const ibc_f4*)a.wT_act;
  const ibc_f4* const w_blk4 = (const ibc_f4*)a.w_blk;
  const ibc_f4* const wT_blk4 = (const ibc_f4*)a.wT_blk;
  int bad = 0;
  float st_k[7];      // the lane's share of the state part of the input row: feature 4 s2 + g
#pragma unroll
  for (int s2 = 0; s2 < 7; s2++) {
    const int f = 4 * s2 + g;
    st_k[s2] = f < OBS ? a.state[n * OBS + f] : 0.f;
    bad |= policy_nonfinite(st_k[s2]) ? 1 : 0;
  }
  // Wave 0 keeps the samples: lane (g, j) owns components g and 4 + g of row j (start point, noise, update); the other waves read them from LDS.
  const int qa = g, qb = 4 + g;
  const bool ina = qa < A, inb = qb < A;
  const float lo_a = ina ? a.lo[qa] : 0.f, hi_a = ina ? a.hi[qa] : 0.f, cl_a = ina ? a.clip[qa] : 0.f;
  const float lo_b = inb ? a.lo[qb] : 0.f, hi_b = inb ? a.hi[qb] : 0.f, cl_b = inb ? a.clip[qb] : 0.f;

#pragma clang loop unroll(disable)
  for (int rt = 0; rt < IBC_S / 16; rt++) {
    const int s = 16 * rt + j;
    const long row = n * IBC_S + s;
    // ---- 1. the start point
    if (w == 0) {
      float xa, xc;
      if (a.x0_in) {
        xa = ina ? a.x0_in[row * A + qa] : 0.f;
        xc = inb ? a.x0_in[row * A + qb] : 0.f;
      } else {
        unsigned r[4], r2[4] = {0u, 0u, 0u, 0u};
        philox4x32_10(k0, k1, c0, c1, t_word, IBC_TAG | ((unsigned)s << 2), r);
        if (A > 4) philox4x32_10(k0, k1, c0, c1, t_word, IBC_TAG | ((unsigned)s << 2) | 1u, r2);
        unsigned ra = r[0], rb = r2[0];
#pragma unroll
        for (int m = 1; m < 4; m++) { ra = g == m ? r[m] : ra; rb = g == m ? r2[m] : rb; }
        xa = ina ? ibc_start(lo_a, hi_a, policy_uniform24(ra)) : 0.f;
        xc = inb ? ibc_start(lo_b, hi_b, policy_uniform24(rb)) : 0.f;
      }
      bad |= (policy_nonfinite(xa) || policy_nonfinite(xc)) ? 1 : 0;
      sx[s * IBC_AMAX + qa] = (double)xa; sx[s * IBC_AMAX + qb] = (double)xc;
      if (a.x0_out) {
        if (ina) a.x0_out[row * A + qa] = xa;
        if (inb) a.x0_out[row * A + qb] = xc;
      }
    }
    __syncthreads();
    // ---- 2. the chain, then (k == K) 3. the energy of the final x
#pragma clang loop unroll(disable)
    for (int k = 0; k <= K; k++) {
      const bool last = k == K;
      // ---- forward: the input layer on [state | x]
      float in_k[7];
#pragma unroll
      for (int s2 = 0; s2 < 7; s2++) {
        const int f = 4 * s2 + g - OBS, fc = f < 0 ? 0 : (f > IBC_AMAX - 1 ? IBC_AMAX - 1 : f);
        const float xv = (float)sx[s * IBC_AMAX + fc];
        in_k[s2] = (f >= 0 && f < A) ? xv : st_k[s2];
      }
      ibc_f4 xo[TPW], dx[IBC_MAXB][TPW], du[IBC_MAXB][TPW];
#pragma unroll
      for (int q = 0; q < TPW; q++) {
        const int To = TPW * w + q;
        ibc_f4 acc = *(const ibc_f4*)(a.b_in + 16 * To + 4 * g);
        const ibc_f4 a0 = w_in4[(To * 64 + lane) * 2], a1 = w_in4[(To * 64 + lane) * 2 + 1];
#pragma unroll
        for (int s2 = 0; s2 < 7; s2++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s2 < 4 ? a0[s2] : a1[s2 - 4], in_k[s2], acc, 0, 0, 0);
        xo[q] = acc;
      }
      // ---- forward: the blocks x + l2(mish(l1(mish(x)))); the derivatives of both Mish stay where they are
#pragma unroll
      for (int b = 0; b < IBC_MAXB; b++)
#pragma unroll
        for (int q = 0; q < TPW; q++) { dx[b][q] = ibc_f4{0.f, 0.f, 0.f, 0.f}; du[b][q] = ibc_f4{0.f, 0.f, 0.f, 0.f}; }
#pragma clang loop unroll(disable)
      for (int b = 0; b < nblk; b++) {
        ibc_f4 y[TPW], d[TPW];
#pragma unroll
        for (int q = 0; q < TPW; q++) xb[0][(TPW * w + q) * 64 + lane] = ibc_mish4(xo[q], d[q]);
        ibc_keep<TPW>(dx, b, d);
        __syncthreads();
        ibc_layer<HID, true, false>(w_blk4 + (long)(2 * b) * LAYER_F4, a.b_blk + (2 * b) * HID, xb[0], y, w, lane, g);
#pragma unroll
        for (int q = 0; q < TPW; q++) xb[1][(TPW * w + q) * 64 + lane] = ibc_mish4(y[q], d[q]);
        ibc_keep<TPW>(du, b, d);
        __syncthreads();
        ibc_layer<HID, true, true>(w_blk4 + (long)(2 * b + 1) * LAYER_F4, a.b_blk + (2 * b + 1) * HID, xb[1], xo, w, lane, g);
      }
      ibc_f4 gy[TPW];
      if (last) {
#pragma unroll
        for (int q = 0; q < TPW; q++) gy[q] = xo[q];      // 3. the output layer reads the residual stream itself
      } else {
        // ---- backward: g = w_out, then per block gx = gy + m'(x) . W1^T (m'(u) . W2^T gy), last block first
#pragma unroll
        for (int q = 0; q < TPW; q++) gy[q] = w_out4[(TPW * w + q) * 64 + 16 * g];      // (output row 0 of the packed tile: W_out[0][16 To + 4 g + r])
#pragma clang loop unroll(disable)
        for (int b = nblk - 1; b >= 0; b--) {
          ibc_f4 v[TPW], d[TPW];
#pragma unroll
          for (int q = 0; q < TPW; q++) xb[0][(TPW * w + q) * 64 + lane] = gy[q];
          __syncthreads();
          ibc_layer<HID, false, false>(wT_blk4 + (long)(2 * b + 1) * LAYER_F4, nullptr, xb[0], v, w, lane, g);
          ibc_take<TPW>(du, b, d);
#pragma unroll
          for (int q = 0; q < TPW; q++) xb[1][(TPW * w + q) * 64 + lane] = v[q] * d[q];
          __syncthreads();
          ibc_layer<HID, false, false>(wT_blk4 + (long)(2 * b) * LAYER_F4, nullptr, xb[1], v, w, lane, g);
          ibc_take<TPW>(dx, b, d);
#pragma unroll
          for (int q = 0; q < TPW; q++) gy[q] += v[q] * d[q];
        }
      }
      // ---- one 16-row output tile on what is in gy, by wave 0: the energy (w_out on the residual stream) or the action columns of the input layer on the
      // gradient, g_a = W_in[:, obs + a] . g (lane (g', j), register r: component 4 g' + r of row j; the energy is component 0)
#pragma unroll
      for (int q = 0; q < TPW; q++) xb[0][(TPW * w + q) * 64 + lane] = gy[q];
      __syncthreads();
      if (w == 0) {
        const ibc_f4* const wt4 = last ? w_out4 : wT_act4;
        ibc_f4 acc = ibc_f4{0.f, 0.f, 0.f, 0.f}, acc2 = ibc_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; t++) {
          const ibc_f4 a4 = wt4[t * 64 + lane], m4 = xb[0][t * 64 + lane];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0], m4[0], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1], m4[1], acc2, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[2], m4[2], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[3], m4[3], acc2, 0, 0, 0);
        }
        acc += acc2;
        if (last) {
          const float e = acc[0] + a.b_out[0];      // (lanes (0, j))
          if (g == 0) {
            bad |= policy_nonfinite(e) ? 1 : 0;
            se[s] = e;
            if (a.energies) a.energies[row] = e;
          }
          if (a.x_final) {
            if (ina) a.x_final[row * A + qa] = (float)sx[s * IBC_AMAX + qa];
            if (inb) a.x_final[row * A + qb] = (float)sx[s * IBC_AMAX + qb];
          }
        } else {
          // this lane's two components: 4 g' + r = g (lane (0, j), register g) and 4 + g (lane (1, j), register g)
          float ga = 0.f, gb = 0.f;
#pragma unroll
          for (int m = 0; m < 4; m++) {      // (register m of lanes (0, j) / (1, j), wanted by the lanes with g == m)
            const float va = __shfl(acc[m], j), vb = __shfl(acc[m], 16 + j);
            ga = g == m ? va : ga; gb = g == m ? vb : gb;
          }
          // ---- the noise of this (n, s, k)
          float za, zb;
          const long nbase = (((long)k * a.n_env + n) * IBC_S + s) * A;
          if (a.noise_in) {
            za = ina ? a.noise_in[nbase + qa] : 0.f;
            zb = inb ? a.noise_in[nbase + qb] : 0.f;
          } else {
            const unsigned tag = IBC_TAG | (1u << 14) | ((unsigned)k << 8) | ((unsigned)s << 2);
            unsigned r[4];
            float nz[8];
            philox4x32_10(k0, k1, c0, c1, t_word, tag, r);
            policy_box_muller(r[0], r[1], nz[0], nz[1]); policy_box_muller(r[2], r[3], nz[2], nz[3]);
            if (A > 4) {
              philox4x32_10(k0, k1, c0, c1, t_word, tag | 1u, r);
              policy_box_muller(r[0], r[1], nz[4], nz[5]); policy_box_muller(r[2], r[3], nz[6], nz[7]);
            } else {
              nz[4] = nz[5] = nz[6] = nz[7] = 0.f;
            }
            za = nz[0]; zb = nz[4];
#pragma unroll
            for (int m = 1; m < 4; m++) { za = g == m ? nz[m] : za; zb = g == m ? nz[4 + m] : zb; }
          }
          if (a.noise_out) {
            if (ina) a.noise_out[nbase + qa] = za;
            if (inb) a.noise_out[nbase + qb] = zb;
          }
          // ---- the Langevin update, in f64 on the f32 gradient and noise
          // (the bit tests below look at the f32 casts: conservative - a finite f64 beyond FLT_MAX would mark the environment where the reference would clip
          // it; out of reach with f32 gradients and steps <= 1)
          const double hs = (double)a.coef[2 * k], st = (double)a.coef[2 * k + 1], ns = (double)a.noise_scale;
          const double raw_a = hs * (double)ga + st * ((double)za * ns), raw_b = hs * (double)gb + st * ((double)zb * ns);
          const double xn_a = fmin(fmax(sx[s * IBC_AMAX + qa] - fmin(fmax(raw_a, -(double)cl_a), (double)cl_a), (double)lo_a), (double)hi_a);
          const double xn_b = fmin(fmax(sx[s * IBC_AMAX + qb] - fmin(fmax(raw_b, -(double)cl_b), (double)cl_b), (double)lo_b), (double)hi_b);
          bad |= (ina && (policy_nonfinite(ga) || policy_nonfinite((float)raw_a) || policy_nonfinite((float)xn_a))) ? 1 : 0;
          bad |= (inb && (policy_nonfinite(gb) || policy_nonfinite((float)raw_b) || policy_nonfinite((float)xn_b))) ? 1 : 0;
          if (ina) sx[s * IBC_AMAX + qa] = xn_a;
          if (inb) sx[s * IBC_AMAX + qb] = xn_b;
        }
      }
      __syncthreads();      // the new iterate is in LDS; xb[0] is written again by the next forward pass
    }
  }
  // ---- 3. softmax over the 64 energies, one draw, the action (wave 0)
  const int bad_env = __syncthreads_or(bad);
  if (w != 0) return;
  const float e = se[lane];
  float emin = e;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) emin = fminf(emin, __shfl_xor(emin, m));
  const float p = expf(-(e - emin));
  float c = p;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) { const float up = __shfl_up(c, m); c += lane >= m ? up : 0.f; }
  const float S = __shfl(c, 63);
  float u;
  if (a.u_in) u = a.u_in[n];
  else {
    unsigned r[4];
    philox4x32_10(k0, k1, c0, c1, t_word, IBC_TAG | (2u << 14), r);
    u = policy_uniform24(r[0]);
  }
  const int cnt = __popcll(__ballot(c <= u * S));
  const int pick = cnt < IBC_S - 1 ? cnt : IBC_S - 1;
  if (lane < A) {
    unsigned yb = __float_as_uint((float)(sx[pick * IBC_AMAX + lane] * (double)a.scale[lane] + (double)a.shift[lane]));
    yb = bad_env ? 0x7FC00000u : yb;
    ((unsigned*)a.actions)[n * A + lane] = yb;
  }
  if (lane == 0) {
    a.picks[n] = bad_env ? -1 : pick;
    if (a.u_out) a.u_out[n] = u;
  }
}

}  // namespace d3il
