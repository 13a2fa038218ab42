// policy_act.h - the chunk pass and the per-lane chunk bookkeeping of the batched VAE-ACT policy (policies.ACTPolicy; agents/act_agent.py:207-239 around
// agents/models/act/act_vae.py:389-445 ActVAE.forward without actions) as ONE kernel (included by rollout.hip).
//
// Per environment n (persistent device state: counter[n], chunk[n][T][A], the chunk already clamped and inverse-scaled):
//   due = counter[n] == T (or outside 0 .. T).  A due environment computes a new chunk:
//   1. z = latent_in[n] or 32 uniforms, component 4 q + m = 24 bits of word m of philox4x32_10(seed, (env_offset + n, step word, ACT_TAG | q)), q < 8
//   2. encoder input [W_s state + pos[0], W_z z + pos[1]] (no bias; pos: the host-prepared [2][64] table - for T = 1 both rows are pos_emb[0], as the
//      reference's slice broadcasts); n_enc blocks x + proj(attn(ln1 x)), x + fc2(gelu(fc1(ln2 x))) with the reference's causal mask on the two tokens
//      (mask sliced from a T x T triangle: for T = 1 it is a single one and masks nothing), LayerNorm with weight only, exact GELU; a final LayerNorm
//   3. decoder on the T query embeddings: x + proj(causal self-attention(ln1 x) + cross-attention(ln1 x, encoder output)) - both attention outputs are added in
//      front of ONE projection, the cross keys and values come from the raw encoder output, unmasked over its two tokens, both scale by 1 / 4 -, then
//      x + fc2(gelu(fc1(ln2 x))); a final LayerNorm and the action head
//   4. chunk[n][t][a] = clamp(head, lo_a, hi_a) scale_a + shift_a (two f32 operations), counter[n] = 0
//   Every environment then emits actions[n] = chunk[n][counter[n]] and stores counter[n] + 1.
//
// Tiling.  A workgroup of four waves owns 16 environments.  A 16-row matrix-core tile is the 16 environments at one token; wave w owns output tile w of the
// four of width 64 - features 16 w .. 16 w + 15, which are exactly head w - and tiles 4 w .. 4 w + 3 of the MLP's hidden 256.  v_mfma_f32_16x16x4_f32 throughout (exact f32
// products), the weights stream from L2 in fragment order ([To][t][lane (g, i)][r] = W[16 To + i][16 t + 4 g + r], policies.pack_act_weights).  Lane (g, j) of
// wave w holds features 16 w + 4 g + r of environment j: the residual streams (2 encoder, up to 8 decoder tokens), keys, values and attention outputs of head w
// stay in REGISTERS, a head's dot product is four products per lane and two xor shuffles over g.  LDS holds what the next product reads as its B operand:
// the normalised / attention rows (8 tokens x 4 KB), the encoder output (8 KB), one token's hidden row (16 KB) and the LayerNorm partial sums (4 KB): 60 KB.
// A workgroup without a due environment skips 1 - 4 (__syncthreads_or: workgroup-uniform).  Environments that are not due run through the network on a zero
// state row (their columns of every product are their own: no other column reads them) and store nothing but their action and counter.
//
// No atomics, no workspace, vector stores only, no inline assembly beyond the empty register barrier of the bit test, every branch in front of a barrier or
// shuffle depends on kernel arguments or the workgroup-wide vote only.  NaN / Inf: built with -ffinite-math-only, so the state row and the head outputs of a
// due environment are tested on their bit pattern; a hit gives 0x7FC00000 in the whole chunk and the emitted action, and changes no other environment.
#pragma once

namespace d3il {

constexpr unsigned ACT_TAG = 0x41430000u;      // fourth counter word = TAG | q (q < 8): never 0, never BET_TAG, never a DDPM_GPT_TAG or IBC_TAG word
constexpr int ACT_C = 64, ACT_NH = 4, ACT_LAT = 32, ACT_OBSMAX = 32, ACT_TMAX = 8, ACT_AMAX = 8, ACT_MAXENC = 4, ACT_MAXDEC = 8;
// packed layer arrays (policies.pack_act_weights), in floats: matrices [q k v proj fc1 fc2] / [q k v cq ck cv proj fc1 fc2], vectors [ln1 ln2 b.. b1 b2]
constexpr int ACT_ENC_W = 4 * 4096 + 2 * 16384, ACT_ENC_V = 704, ACT_DEC_W = 7 * 4096 + 2 * 16384, ACT_DEC_V = 896;
// tab: pos [2][64] | query_embed [8][64] | encoder ln | decoder ln | head bias [16]
constexpr int ACT_TAB_QE = 128, ACT_TAB_LNE = 640, ACT_TAB_LND = 704, ACT_TAB_HB = 768, ACT_TAB = 784;
typedef float act_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ act_f4 act_ld4(const float* p) { return *(const act_f4*)p; }
// output tile To of a packed layer with NT input tiles on one token's 16 rows (xin: LDS, B-operand order), added to init
template <int NT>
__device__ __forceinline__ act_f4 act_lin(const act_f4* __restrict__ wl, int To, const act_f4* xin, act_f4 init, int lane) {
  const act_f4* const wt = wl + (long)To * (NT * 64) + lane;
  act_f4 acc[4] = {init, act_f4{0.f, 0.f, 0.f, 0.f}, act_f4{0.f, 0.f, 0.f, 0.f}, act_f4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const act_f4 m = xin[t * 64 + lane], a = wt[t * 64];
#pragma unroll
    for (int r = 0; r < 4; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], m[r], acc[r], 0, 0, 0);
  }
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}
// q . k of the wave's head for the lane's environment, scaled by 1 / sqrt(16): the lane's four features, then the four lanes (g) of the environment
__device__ __forceinline__ float act_dot(act_f4 q, act_f4 k) {
  float p = (q[0] * k[0] + q[1] * k[1]) + (q[2] * k[2] + q[3] * k[3]);
  p += __shfl_xor(p, 16);
  p += __shfl_xor(p, 32);
  return p * 0.25f;
}
// softmax over two keys
__device__ __forceinline__ act_f4 act_mix2(float sa, float sb, act_f4 va, act_f4 vb) {
  const float m = fmaxf(sa, sb), pa = expf(sa - m), pb = expf(sb - m), sum = pa + pb;
  return va * (pa / sum) + vb * (pb / sum);
}
__device__ __forceinline__ act_f4 act_gelu4(act_f4 x) {
  act_f4 y;
#pragma unroll
  for (int r = 0; r < 4; r++) y[r] = 0.5f * x[r] * (1.f + erff(x[r] * 0.70710678118654752440f));
  return y;
}
// LayerNorm (weight only, eps 1e-5, two passes) of the n_tok register rows x into LDS rows out[t][..] in B-operand order.  Three barriers, all unconditional.
template <int MAXT>
__device__ __forceinline__ void act_ln(const act_f4* x, int n_tok, const float* __restrict__ wln, act_f4* out, float (*ps)[ACT_TMAX * 64], int w, int lane, int g, int j) {
  float mean[MAXT], rstd[MAXT];
#pragma unroll
  for (int t = 0; t < MAXT; t++)
    if (t < n_tok) {
      float s = (x[t][0] + x[t][1]) + (x[t][2] + x[t][3]);
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (g == 0) ps[0][(t * 4 + w) * 16 + j] = s;
    }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < MAXT; t++)
    if (t < n_tok) {
      const float* p = ps[0] + t * 64 + j;
      mean[t] = ((p[0] + p[16]) + (p[32] + p[48])) * (1.f / 64.f);
      const act_f4 d = x[t] - mean[t];
      float s = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      if (g == 0) ps[1][(t * 4 + w) * 16 + j] = s;
    }
  __syncthreads();
  const act_f4 wv = act_ld4(wln + 16 * w + 4 * g);
#pragma unroll
  for (int t = 0; t < MAXT; t++)
    if (t < n_tok) {
      const float* p = ps[1] + t * 64 + j;
      rstd[t] = 1.f / sqrtf(((p[0] + p[16]) + (p[32] + p[48])) * (1.f / 64.f) + 1e-5f);
      out[t * 256 + w * 64 + lane] = (x[t] - mean[t]) * rstd[t] * wv;
    }
  __syncthreads();
}
// fc2(gelu(fc1(row))) of one token: the wave's four hidden tiles into LDS, then its output tile.  Two barriers.
__device__ __forceinline__ act_f4 act_mlp(const act_f4* __restrict__ w1, const act_f4* __restrict__ w2, const float* __restrict__ b1, const float* __restrict__ b2,
                                          const act_f4* xin, act_f4* hid, int w, int lane, int g) {
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int To = 4 * w + q;
    hid[To * 64 + lane] = act_gelu4(act_lin<4>(w1, To, xin, act_ld4(b1 + 16 * To + 4 * g), lane));
  }
  __syncthreads();
  const act_f4 y = act_lin<16>(w2, w, hid, act_ld4(b2 + 16 * w + 4 * g), lane);
  __syncthreads();
  return y;
}

struct ActArgs {
  const float* state; const float* w_in; const float* tab; const float* enc_w; const float* enc_v; const float* dec_w; const float* dec_v; const float* head_w;
  const float* lo; const float* hi; const float* scale; const float* shift; const unsigned* t_dev; const float* latent_in;
  int* counter; float* chunk; float* actions; float* latent_out;
  unsigned long long seed, env_offset;
  long n_env;
  int obs, A, T, n_enc, n_dec;
};

__global__ __launch_bounds__(256) void k_act_chunk(ActArgs a) {
  __shared__ act_f4 hb[ACT_TMAX * 256];      // up to 8 token rows [t][tile][lane]: LayerNorm output, then the attention output in its place
  __shared__ act_f4 eo[2 * 256];             // the encoder output (two tokens), read by every decoder layer
  __shared__ act_f4 hid[16 * 64];            // one token's hidden row of the MLP; first the state and latent rows (two input tiles each)
  __shared__ float ps[2][ACT_TMAX * 64];     // LayerNorm partial sums [token][wave][environment]
  __shared__ int sbad[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const int A = a.A, T = a.T, OBS = a.obs;
  const long n = (long)blockIdx.x * 16 + j;
  const bool valid = n < a.n_env;      // (a last tile with fewer than 16 environments: its other columns compute on zeros and store nothing)
  int cnt = valid ? a.counter[n] : 0;
  const bool due = valid && (cnt < 0 || cnt >= T);
  const int fo = 16 * w + 4 * g;      // the lane's first feature
  unsigned out0[4] = {0u, 0u, 0u, 0u};      // token 0 of a new chunk (wave 0)

  if (__syncthreads_or(due ? 1 : 0)) {
    // ---- 1. state row and latent as B operands (wave 0 loads and draws)
    if (tid < 16) sbad[tid] = 0;
    int badl = 0;
    if (w == 0) {
      const unsigned t_word = *a.t_dev;
      const unsigned long long ge = a.env_offset + (unsigned long long)n;
#pragma unroll
      for (int t = 0; t < 2; t++) {
        act_f4 s = act_f4{0.f, 0.f, 0.f, 0.f}, z = act_f4{0.f, 0.f, 0.f, 0.f};
        if (due) {
          unsigned rr[4] = {0u, 0u, 0u, 0u};
          if (!a.latent_in) philox4x32_10((unsigned)a.seed, (unsigned)(a.seed >> 32), (unsigned)ge, (unsigned)(ge >> 32), t_word, ACT_TAG | (unsigned)(4 * t + g), rr);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int f = 16 * t + 4 * g + r;
            const float v = f < OBS ? a.state[n * OBS + f] : 0.f;
            badl |= policy_nonfinite(v) ? 1 : 0;
            s[r] = v;
            z[r] = a.latent_in ? a.latent_in[n * ACT_LAT + f] : policy_uniform24(rr[r]);
            if (a.latent_out) a.latent_out[n * ACT_LAT + f] = z[r];
          }
        }
        hid[t * 64 + lane] = s;
        hid[128 + t * 64 + lane] = z;
      }
    }
    __syncthreads();
    if (badl) sbad[j] = 1;
    // ---- 2. the encoder on [state token, latent token]
    act_f4 xe[2];
    xe[0] = act_lin<2>((const act_f4*)a.w_in, w, hid, act_ld4(a.tab + fo), lane);
    xe[1] = act_lin<2>((const act_f4*)a.w_in + 512, w, hid + 128, act_ld4(a.tab + 64 + fo), lane);
    const bool causal = T >= 2;      // the reference slices its mask from a T x T triangle
#pragma clang loop unroll(disable)
    for (int l = 0; l < a.n_enc; l++) {
      const act_f4* const W = (const act_f4*)(a.enc_w + (long)l * ACT_ENC_W);
      const float* const V = a.enc_v + l * ACT_ENC_V;
      act_ln<2>(xe, 2, V, hb, ps, w, lane, g, j);
      const act_f4 q0 = act_lin<4>(W, w, hb, act_ld4(V + 128 + fo), lane), q1 = act_lin<4>(W, w, hb + 256, act_ld4(V + 128 + fo), lane);
      const act_f4 k0 = act_lin<4>(W + 1024, w, hb, act_ld4(V + 192 + fo), lane), k1 = act_lin<4>(W + 1024, w, hb + 256, act_ld4(V + 192 + fo), lane);
      const act_f4 v0 = act_lin<4>(W + 2048, w, hb, act_ld4(V + 256 + fo), lane), v1 = act_lin<4>(W + 2048, w, hb + 256, act_ld4(V + 256 + fo), lane);
      const act_f4 y0m = act_mix2(act_dot(q0, k0), act_dot(q0, k1), v0, v1);
      const act_f4 y0 = causal ? v0 : y0m;      // the state token sees only itself
      const act_f4 y1 = act_mix2(act_dot(q1, k0), act_dot(q1, k1), v0, v1);
      __syncthreads();
      hb[w * 64 + lane] = y0;
      hb[256 + w * 64 + lane] = y1;
      __syncthreads();
      xe[0] += act_lin<4>(W + 3072, w, hb, act_ld4(V + 320 + fo), lane);
      xe[1] += act_lin<4>(W + 3072, w, hb + 256, act_ld4(V + 320 + fo), lane);
      act_ln<2>(xe, 2, V + 64, hb, ps, w, lane, g, j);
#pragma unroll
      for (int t = 0; t < 2; t++) xe[t] += act_mlp(W + 4096, W + 8192, V + 384, V + 640, hb + t * 256, hid, w, lane, g);
    }
    act_ln<2>(xe, 2, a.tab + ACT_TAB_LNE, eo, ps, w, lane, g, j);
    // ---- 3. the decoder on the T query embeddings
    act_f4 xd[ACT_TMAX];
#pragma unroll
    for (int t = 0; t < ACT_TMAX; t++) xd[t] = t < T ? act_ld4(a.tab + ACT_TAB_QE + t * 64 + fo) : act_f4{0.f, 0.f, 0.f, 0.f};
#pragma clang loop unroll(disable)
    for (int l = 0; l < a.n_dec; l++) {
      const act_f4* const W = (const act_f4*)(a.dec_w + (long)l * ACT_DEC_W);
      const float* const V = a.dec_v + l * ACT_DEC_V;
      act_ln<ACT_TMAX>(xd, T, V, hb, ps, w, lane, g, j);
      const act_f4 ck0 = act_lin<4>(W + 4096, w, eo, act_ld4(V + 384 + fo), lane), ck1 = act_lin<4>(W + 4096, w, eo + 256, act_ld4(V + 384 + fo), lane);
      const act_f4 cv0 = act_lin<4>(W + 5120, w, eo, act_ld4(V + 448 + fo), lane), cv1 = act_lin<4>(W + 5120, w, eo + 256, act_ld4(V + 448 + fo), lane);
      act_f4 kk[ACT_TMAX], vv[ACT_TMAX], yy[ACT_TMAX];
#pragma unroll
      for (int t = 0; t < ACT_TMAX; t++) {
        kk[t] = vv[t] = yy[t] = act_f4{0.f, 0.f, 0.f, 0.f};
        if (t < T) {
          kk[t] = act_lin<4>(W + 1024, w, hb + t * 256, act_ld4(V + 192 + fo), lane);
          vv[t] = act_lin<4>(W + 2048, w, hb + t * 256, act_ld4(V + 256 + fo), lane);
        }
      }
#pragma unroll
      for (int tq = 0; tq < ACT_TMAX; tq++)
        if (tq < T) {
          const act_f4 q = act_lin<4>(W, w, hb + tq * 256, act_ld4(V + 128 + fo), lane), cq = act_lin<4>(W + 3072, w, hb + tq * 256, act_ld4(V + 320 + fo), lane);
          float s[ACT_TMAX];
          float m = 0.f, sum = 0.f;
#pragma unroll
          for (int i = 0; i <= tq; i++) { s[i] = act_dot(q, kk[i]); m = i == 0 ? s[i] : fmaxf(m, s[i]); }
#pragma unroll
          for (int i = 0; i <= tq; i++) { s[i] = expf(s[i] - m); sum += s[i]; }
          act_f4 y = act_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int i = 0; i <= tq; i++) y += vv[i] * (s[i] / sum);
          yy[tq] = y + act_mix2(act_dot(cq, ck0), act_dot(cq, ck1), cv0, cv1);
        }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < ACT_TMAX; t++)
        if (t < T) hb[t * 256 + w * 64 + lane] = yy[t];
      __syncthreads();
#pragma unroll
      for (int t = 0; t < ACT_TMAX; t++)
        if (t < T) xd[t] += act_lin<4>(W + 6144, w, hb + t * 256, act_ld4(V + 512 + fo), lane);
      act_ln<ACT_TMAX>(xd, T, V + 64, hb, ps, w, lane, g, j);
#pragma unroll
      for (int t = 0; t < ACT_TMAX; t++)
        if (t < T) xd[t] += act_mlp(W + 7168, W + 11264, V + 576, V + 832, hb + t * 256, hid, w, lane, g);
    }
    act_ln<ACT_TMAX>(xd, T, a.tab + ACT_TAB_LND, hb, ps, w, lane, g, j);
    // ---- 4. head (wave 0: lane (g, j), register r = component 4 g + r of environment j), clamp, inverse scaling, the chunk
    act_f4 oo[ACT_TMAX];
    if (w == 0) {
      int badh = 0;
#pragma unroll
      for (int t = 0; t < ACT_TMAX; t++) {
        oo[t] = act_f4{0.f, 0.f, 0.f, 0.f};
        if (t < T) {
          oo[t] = act_lin<4>((const act_f4*)a.head_w, 0, hb + t * 256, act_ld4(a.tab + ACT_TAB_HB + 4 * g), lane);
#pragma unroll
          for (int r = 0; r < 4; r++) badh |= (4 * g + r < A && policy_nonfinite(oo[t][r])) ? 1 : 0;
        }
      }
      if (badh && due) sbad[j] = 1;
    }
    __syncthreads();
    if (w == 0 && due) {
      const int bad = sbad[j];
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int c = 4 * g + r;
        if (c < A) {
          const float lo = a.lo[c], hi = a.hi[c], sc = a.scale[c], sh = a.shift[c];
#pragma unroll
          for (int t = 0; t < ACT_TMAX; t++)
            if (t < T) {
#pragma clang fp contract(off)
              const float cl = fminf(fmaxf(oo[t][r], lo), hi);
              const float pr = cl * sc;
              const unsigned bits = bad ? 0x7FC00000u : __float_as_uint(pr + sh);
              ((unsigned*)a.chunk)[(n * T + t) * A + c] = bits;
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
      if (c < A) ((unsigned*)a.actions)[n * A + c] = due ? out0[r] : ((const unsigned*)a.chunk)[(n * T + at) * A + c];
    }
    if (g == 0) a.counter[n] = at + 1;
  }
}

}  // namespace d3il
