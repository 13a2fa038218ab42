// policy_ddpm_act.h - the whole reverse-diffusion chain and the per-lane chunk bookkeeping of the batched DDPM-ACT policy (policies.DDPMACTPolicy;
// agents/ddpm_encdec_agent.py:222-257 around diffusion_policy.py:117-217 Diffusion.sample and diffusion_models.py:844-905 DiffusionEncDec.forward, no goals) as ONE
// kernel (included by rollout.hip after policy_act.h, whose building blocks it uses; the random stream and the bit test: policy_common.h).
//
// Per environment n (persistent device state: counter[n], chunk[n][Ta][A], the chunk already clamped and inverse-scaled; the window win[n][S][obs] left-aligned with
// len[n] valid rows, policies._History.padded):
//   due = counter[n] == Ta (or outside 0 .. Ta).  A due environment with L = len[n] window rows computes a new chunk:
//   1. state tokens s_i = (W_tok win[n][i] + b_tok) + pos[i], i < L (once: they do not change along the chain)
//   2. x = noise_in[n][T] or Box-Muller normals of chain index T (x_in: the given iterate)
//   3. for i = T - 1 .. 0 (test hook: k_start .. k_stop, none for k_stop > k_start):
//        encoder on [temb[i], s_0 .. s_{L-1}] with its causal mask (the time token sees itself, s_i the time token and s_0 .. s_i), final LayerNorm: 1 + L rows
//        action tokens (W_act x_t + b_act) + pos[L - 1 + t], t < Ta; decoder: x + proj(causal self-attention(ln1 x) + cross-attention(ln1 x, the 1 + L encoder rows,
//        unmasked)), x + fc2(gelu(fc1(ln2 x))), final LayerNorm; eps = head
//        x0 = clamp(sched[i][0] x - sched[i][1] eps, lo, hi); mean = sched[i][2] x0 + sched[i][3] x; x = mean + sched[i][4] noise_i (i = 0: x = mean, nothing drawn)
//   4. chunk[n][t][a] = clamp(x, lo_a, hi_a) scale_a + shift_a (two f32 operations), counter[n] = 0
//   Every environment then emits actions[n] = chunk[n][counter[n]] and stores counter[n] + 1.
// The encoder pass of step i does not depend on the iterate, but it does depend on i: keeping T encoder outputs would take T x 6 rows of 4 KB per workgroup, so
// the encoder is run again in every chain step (2 layers x 6 tokens next to 4 layers x 4 tokens with two attentions); only the state tokens are kept.
//
// Tiling: the scheme of policy_act.h.  A workgroup of four waves owns 16 environments, a 16-row tile is the 16 environments at one token, wave w owns output tile
// w = head w, v_mfma_f32_16x16x4_f32 with four accumulator chains, residual streams, keys, values, state tokens and the iterate in registers; LDS holds the B
// operands of the next product: 6 token rows (24 KB), the encoder output (24 KB), one hidden row / the input rows (16 KB), the LayerNorm partial sums (4 KB).
// The per-lane window length L enters as predicates in per-lane scalar work only: which window rows are read, the pos row an action token adds, the key count
// 1 + L of the cross-attention softmax.  Padded state tokens run through the products on zero rows (causal attention never shows them to a valid token).  The
// chain and layer loops are runtime loops.  Every branch in front of a barrier or shuffle depends on kernel arguments or the workgroup-wide vote only.
//
// Random numbers: Philox4x32-10, key = seed, counter = (lo32, hi32 of env_offset + n, step word, DDPM_ACT_TAG | k << 8 | t << 1 | q), k = T for the first iterate
// and i for reverse step i (0 is never drawn), t the action token, component 4 q + m; Box-Muller of policy_common.h.  The head output sits on wave 0, lane (g, j)
// = components 4 g .. 4 g + 3 of environment j: that lane draws call q = g and does the x0 / posterior arithmetic.
//
// No atomics, no workspace, vector stores only, no inline assembly beyond the empty register barrier of the bit test.  NaN / Inf (-ffinite-math-only: bit tests): a
// due environment with one in a valid window row, a head output or an iterate gets 0x7FC00000 in its whole chunk and emitted action and bad[n] = 1; padding rows
// and the window of an environment that is not due are not read; no other environment changes.
#pragma once
#include "policy_common.h"
#include "policy_act.h"

namespace d3il {

constexpr unsigned DDPM_ACT_TAG = 0x44410000u;      // fourth counter word = TAG | k << 8 | t << 1 | q: never 0, never a word of the other five tags
constexpr int DA_SMAX = 5, DA_TAMAX = 4, DA_ETOK = 6, DA_TMAX = 255;
// w_in: tok_emb [4][2][64] f4 | action_emb [4][1][64] f4
constexpr int DA_WIN_ACT = 512;
// tab: pos [8][64] | encoder ln | decoder ln | tok_emb bias | action_emb bias | head bias [16] | temb [T][64] | sched [T][5]
constexpr int DA_TAB_LNE = 512, DA_TAB_LND = 576, DA_TAB_TOKB = 640, DA_TAB_ACTB = 704, DA_TAB_HB = 768, DA_TAB_TEMB = 784;

struct DdpmActArgs {
  const float* win; const long long* len; const float* w_in; const float* tab; const float* enc_w; const float* enc_v; const float* dec_w; const float* dec_v;
  const float* head_w; const float* lo; const float* hi; const float* scale; const float* shift; const unsigned* t_dev; const float* noise_in; const float* x_in;
  int* counter; float* chunk; float* actions; int* bad; float* x_out; float* noise_out;
  unsigned long long seed, env_offset;
  long n_env;
  int obs, A, S, Ta, n_enc, n_dec, T, k_start, k_stop;
};

// the four normals of (environment n, chain index k, action token t) a lane (g, .) of wave 0 holds: components 4 g + r, zero beyond A
__device__ __forceinline__ act_f4 da_noise(const DdpmActArgs& a, long n, unsigned long long ge, unsigned t_word, int k, int t, int g) {
  act_f4 z = act_f4{0.f, 0.f, 0.f, 0.f};
  const long row = ((n * (a.T + 1) + k) * a.Ta + t) * a.A;
  if (a.noise_in) {
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (4 * g + r < a.A) z[r] = a.noise_in[row + 4 * g + r];
  } else if (g < 2) {
    unsigned rr[4];
    philox4x32_10((unsigned)a.seed, (unsigned)(a.seed >> 32), (unsigned)ge, (unsigned)(ge >> 32), t_word, DDPM_ACT_TAG | ((unsigned)k << 8) | ((unsigned)t << 1) | (unsigned)g, rr);
    float n0, n1, n2, n3;
    policy_box_muller(rr[0], rr[1], n0, n1);
    policy_box_muller(rr[2], rr[3], n2, n3);
    z = act_f4{n0, n1, n2, n3};
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (4 * g + r >= a.A) z[r] = 0.f;
  }
  if (a.noise_out) {
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (4 * g + r < a.A) a.noise_out[row + 4 * g + r] = z[r];
  }
  return z;
}

// causal self-attention of the wave's head over the n_tok LayerNorm rows in hbuf (query key value = matrices 0 1 2 of W, biases at V + 128 / 192 / 256): yy[tq]
template <int MAXT>
__device__ __forceinline__ void da_self_attn(const act_f4* __restrict__ W, const float* __restrict__ V, const act_f4* hbuf, int n_tok, act_f4* yy, int w, int lane, int fo) {
  act_f4 kk[MAXT], vv[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; t++) {
    kk[t] = vv[t] = yy[t] = act_f4{0.f, 0.f, 0.f, 0.f};
    if (t < n_tok) {
      kk[t] = act_lin<4>(W + 1024, w, hbuf + t * 256, act_ld4(V + 192 + fo), lane);
      vv[t] = act_lin<4>(W + 2048, w, hbuf + t * 256, act_ld4(V + 256 + fo), lane);
    }
  }
#pragma unroll
  for (int tq = 0; tq < MAXT; tq++)
    if (tq < n_tok) {
      const act_f4 q = act_lin<4>(W, w, hbuf + tq * 256, act_ld4(V + 128 + fo), lane);
      float s[MAXT];
      float m = 0.f, sum = 0.f;
#pragma unroll
      for (int i = 0; i <= tq; i++) { s[i] = act_dot(q, kk[i]); m = i == 0 ? s[i] : fmaxf(m, s[i]); }
#pragma unroll
      for (int i = 0; i <= tq; i++) { s[i] = expf(s[i] - m); sum += s[i]; }
      act_f4 y = act_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i <= tq; i++) y += vv[i] * (s[i] / sum);
      yy[tq] = y;
    }
}

__global__ __launch_bounds__(256) void k_ddpm_act_chunk(DdpmActArgs a) {
  __shared__ act_f4 hb[DA_ETOK * 256];       // up to 6 token rows [t][tile][lane]: LayerNorm output, then the attention output in its place
  __shared__ act_f4 eo[DA_ETOK * 256];       // the encoder output of the current chain step (1 + S rows), read by every decoder layer
  __shared__ act_f4 hid[16 * 64];            // one token's hidden row of the MLP; first the window rows (two input tiles each), per step the iterate (one tile per token)
  __shared__ float ps[2][ACT_TMAX * 64];     // LayerNorm partial sums [token][wave][environment]
  __shared__ int sbad[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const int A = a.A, Ta = a.Ta, OBS = a.obs, S = a.S, T = a.T;
  const long n = (long)blockIdx.x * 16 + j;
  const bool valid = n < a.n_env;      // (a last tile with fewer than 16 environments: its other columns compute on zeros and store nothing)
  const int cnt = valid ? a.counter[n] : 0;
  const bool due = valid && (cnt < 0 || cnt >= Ta);
  const int fo = 16 * w + 4 * g;      // the lane's first feature
  unsigned out0[4] = {0u, 0u, 0u, 0u};      // token 0 of a new chunk (wave 0)
  int badf = 0;

  if (__syncthreads_or(due ? 1 : 0)) {
    if (tid < 16) sbad[tid] = 0;
    int L = 1;      // the lane's window length: 1 .. S (a lane that is not due runs on one zero row)
    if (due) {
      const long long l = a.len[n];
      L = l < 1 ? 1 : (l > S ? S : (int)l);
    }
    int badl = 0;
    const int n_tok = 1 + S;
    // ---- 1. the window rows as B operands (wave 0 loads), the state tokens
    if (w == 0) {
#pragma unroll
      for (int s = 0; s < DA_SMAX; s++)
        if (s < S) {
#pragma unroll
          for (int t = 0; t < 2; t++) {
            act_f4 v = act_f4{0.f, 0.f, 0.f, 0.f};
            if (due && s < L) {
#pragma unroll
              for (int r = 0; r < 4; r++) {
                const int f = 16 * t + 4 * g + r;
                const float x = f < OBS ? a.win[(n * S + s) * OBS + f] : 0.f;
                badl |= policy_nonfinite(x) ? 1 : 0;
                v[r] = x;
              }
            }
            hid[(2 * s + t) * 64 + lane] = v;
          }
        }
    }
    __syncthreads();
    act_f4 se[DA_SMAX];
#pragma unroll
    for (int s = 0; s < DA_SMAX; s++) {
      se[s] = act_f4{0.f, 0.f, 0.f, 0.f};
      if (s < S) se[s] = act_lin<2>((const act_f4*)a.w_in, w, hid + s * 128, act_ld4(a.tab + DA_TAB_TOKB + fo), lane) + act_ld4(a.tab + s * 64 + fo);
    }
    __syncthreads();
    // ---- 2. the first iterate (wave 0: lane (g, j), register r = component 4 g + r of environment j)
    const unsigned t_word = *a.t_dev;
    const unsigned long long ge = a.env_offset + (unsigned long long)n;
    const bool hook = a.x_in != nullptr;
    const int k_hi = a.k_start, k_lo = a.k_stop;      // (the entry point fills in T - 1 .. 0 unless the caller asks for a part of the chain)
    act_f4 xx[DA_TAMAX];
    float lo[4], hi[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int c = 4 * g + r;
      lo[r] = c < A ? a.lo[c] : 0.f;
      hi[r] = c < A ? a.hi[c] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < DA_TAMAX; t++) {
      xx[t] = act_f4{0.f, 0.f, 0.f, 0.f};
      if (w == 0 && due && t < Ta) {
        if (hook) {
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (4 * g + r < A) xx[t][r] = a.x_in[(n * Ta + t) * A + 4 * g + r];
        } else {
          xx[t] = da_noise(a, n, ge, t_word, T, t, g);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) badl |= policy_nonfinite(xx[t][r]) ? 1 : 0;
      }
    }
    // ---- 3. the chain
#pragma clang loop unroll(disable)
    for (int i = k_hi; i >= k_lo; i--) {
      // -- the encoder on [time token, state tokens]
      {
        act_f4 xe[DA_ETOK];
        xe[0] = act_ld4(a.tab + DA_TAB_TEMB + i * 64 + fo);
#pragma unroll
        for (int s = 0; s < DA_SMAX; s++) xe[1 + s] = se[s];
#pragma clang loop unroll(disable)
        for (int l = 0; l < a.n_enc; l++) {
          const act_f4* const W = (const act_f4*)(a.enc_w + (long)l * ACT_ENC_W);
          const float* const V = a.enc_v + l * ACT_ENC_V;
          act_ln<DA_ETOK>(xe, n_tok, V, hb, ps, w, lane, g, j);
          act_f4 yy[DA_ETOK];
          da_self_attn<DA_ETOK>(W, V, hb, n_tok, yy, w, lane, fo);
          __syncthreads();
#pragma unroll
          for (int t = 0; t < DA_ETOK; t++)
            if (t < n_tok) hb[t * 256 + w * 64 + lane] = yy[t];
          __syncthreads();
#pragma unroll
          for (int t = 0; t < DA_ETOK; t++)
            if (t < n_tok) xe[t] += act_lin<4>(W + 3072, w, hb + t * 256, act_ld4(V + 320 + fo), lane);
          act_ln<DA_ETOK>(xe, n_tok, V + 64, hb, ps, w, lane, g, j);
#pragma unroll
          for (int t = 0; t < DA_ETOK; t++)
            if (t < n_tok) xe[t] += act_mlp(W + 4096, W + 8192, V + 384, V + 640, hb + t * 256, hid, w, lane, g);
        }
        act_ln<DA_ETOK>(xe, n_tok, a.tab + DA_TAB_LNE, eo, ps, w, lane, g, j);
      }
      // -- the action tokens of the iterate
      if (w == 0) {
#pragma unroll
        for (int t = 0; t < DA_TAMAX; t++)
          if (t < Ta) hid[t * 64 + lane] = xx[t];
      }
      __syncthreads();
      act_f4 xd[DA_TAMAX];
#pragma unroll
      for (int t = 0; t < DA_TAMAX; t++) {
        xd[t] = act_f4{0.f, 0.f, 0.f, 0.f};
        if (t < Ta) xd[t] = act_lin<1>((const act_f4*)a.w_in + DA_WIN_ACT, w, hid + t * 64, act_ld4(a.tab + DA_TAB_ACTB + fo), lane) + act_ld4(a.tab + (L - 1 + t) * 64 + fo);
      }
      // -- the decoder
#pragma clang loop unroll(disable)
      for (int l = 0; l < a.n_dec; l++) {
        const act_f4* const W = (const act_f4*)(a.dec_w + (long)l * ACT_DEC_W);
        const float* const V = a.dec_v + l * ACT_DEC_V;
        act_ln<DA_TAMAX>(xd, Ta, V, hb, ps, w, lane, g, j);
        act_f4 yy[DA_TAMAX];
        da_self_attn<DA_TAMAX>(W, V, hb, Ta, yy, w, lane, fo);
        act_f4 ck[DA_ETOK], cv[DA_ETOK];
#pragma unroll
        for (int e = 0; e < DA_ETOK; e++) {
          ck[e] = cv[e] = act_f4{0.f, 0.f, 0.f, 0.f};
          if (e < n_tok) {
            ck[e] = act_lin<4>(W + 4096, w, eo + e * 256, act_ld4(V + 384 + fo), lane);
            cv[e] = act_lin<4>(W + 5120, w, eo + e * 256, act_ld4(V + 448 + fo), lane);
          }
        }
#pragma unroll
        for (int tq = 0; tq < DA_TAMAX; tq++)
          if (tq < Ta) {
            const act_f4 cq = act_lin<4>(W + 3072, w, hb + tq * 256, act_ld4(V + 320 + fo), lane);
            float s[DA_ETOK];
#pragma unroll
            for (int e = 0; e < DA_ETOK; e++) s[e] = e < n_tok ? act_dot(cq, ck[e]) : 0.f;
            float m = s[0], sum = 0.f;      // the lane's keys: the time token and its L state tokens
#pragma unroll
            for (int e = 1; e < DA_ETOK; e++) m = e <= L ? fmaxf(m, s[e]) : m;
#pragma unroll
            for (int e = 0; e < DA_ETOK; e++) { s[e] = e <= L ? expf(s[e] - m) : 0.f; sum += s[e]; }
            act_f4 y = act_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < DA_ETOK; e++)
              if (e <= L) y += cv[e] * (s[e] / sum);
            yy[tq] += y;
          }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < DA_TAMAX; t++)
          if (t < Ta) hb[t * 256 + w * 64 + lane] = yy[t];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < DA_TAMAX; t++)
          if (t < Ta) xd[t] += act_lin<4>(W + 6144, w, hb + t * 256, act_ld4(V + 512 + fo), lane);
        act_ln<DA_TAMAX>(xd, Ta, V + 64, hb, ps, w, lane, g, j);
#pragma unroll
        for (int t = 0; t < DA_TAMAX; t++)
          if (t < Ta) xd[t] += act_mlp(W + 7168, W + 11264, V + 576, V + 832, hb + t * 256, hid, w, lane, g);
      }
      act_ln<DA_TAMAX>(xd, Ta, a.tab + DA_TAB_LND, hb, ps, w, lane, g, j);
      // -- head, clipped x0, posterior mean, noise: on the lanes that hold the head output
      if (w == 0) {
        const float* const sc = a.tab + DA_TAB_TEMB + T * 64 + i * 5;
        const float s0 = sc[0], s1 = sc[1], s2 = sc[2], s3 = sc[3], s4 = sc[4];
#pragma unroll
        for (int t = 0; t < DA_TAMAX; t++)
          if (t < Ta) {
            const act_f4 eps = act_lin<4>((const act_f4*)a.head_w, 0, hb + t * 256, act_ld4(a.tab + DA_TAB_HB + 4 * g), lane);
            if (due) {
              act_f4 nz = act_f4{0.f, 0.f, 0.f, 0.f};
              if (i > 0) nz = da_noise(a, n, ge, t_word, i, t, g);
#pragma unroll
              for (int r = 0; r < 4; r++) {
#pragma clang fp contract(off)
                const float pa = s0 * xx[t][r], pb = s1 * eps[r];
                const float x0 = fminf(fmaxf(pa - pb, lo[r]), hi[r]);
                const float ma = s2 * x0, mb = s3 * xx[t][r];
                const float mean = ma + mb;
                const float pn = s4 * nz[r];
                const float xn = i > 0 ? mean + pn : mean;
                const bool in = 4 * g + r < A;
                badl |= (in && (policy_nonfinite(eps[r]) || policy_nonfinite(xn))) ? 1 : 0;
                xx[t][r] = in ? xn : 0.f;
              }
            }
          }
      }
    }
    // ---- 4. final clamp, inverse scaling, the chunk
    if (w == 0 && due) {
      if (badl) sbad[j] = 1;
      if (a.x_out) {
#pragma unroll
        for (int t = 0; t < DA_TAMAX; t++)
          if (t < Ta) {
#pragma unroll
            for (int r = 0; r < 4; r++)
              if (4 * g + r < A) a.x_out[(n * Ta + t) * A + 4 * g + r] = xx[t][r];
          }
      }
    }
    __syncthreads();
    if (w == 0 && due) {
      badf = sbad[j];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int c = 4 * g + r;
        if (c < A) {
          const float sc = a.scale[c], sh = a.shift[c];
#pragma unroll
          for (int t = 0; t < DA_TAMAX; t++)
            if (t < Ta) {
#pragma clang fp contract(off)
              const float cl = fminf(fmaxf(xx[t][r], lo[r]), hi[r]);
              const float pr = cl * sc;
              const unsigned bits = badf ? 0x7FC00000u : __float_as_uint(pr + sh);
              ((unsigned*)a.chunk)[(n * Ta + t) * A + c] = bits;
              if (t == 0) out0[r] = bits;
            }
        }
      }
    }
  }
  // ---- every environment emits chunk[counter] and counts on
  if (w == 0 && valid) {
    const int at = due ? 0 : cnt;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int c = 4 * g + r;
      if (c < A) ((unsigned*)a.actions)[n * A + c] = due ? out0[r] : ((const unsigned*)a.chunk)[(n * Ta + at) * A + c];
    }
    if (g == 0) {
      a.counter[n] = at + 1;
      if (a.bad) a.bad[n] = badf;
    }
  }
}

}  // namespace d3il
