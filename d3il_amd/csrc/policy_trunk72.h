// policy_trunk72.h - the whole block chain of a 72-wide transformer trunk (n_embd 72, 4 heads of 18, hidden 288: the Avoiding / Aligning / Pushing / Sorting-2
// configs; score_gpts.py:83-115 Block, n_layer times) as ONE kernel (included by rollout.hip after policy_f16x3.h, whose split-f16 helpers it uses):
//     for l in 0 .. n_layer - 1:
//         x = x + proj_l(causal_attention_4heads(LN1_l(x) Wqkv_l' + bqkv_l)) + bproj_l
//         x = x + W2_l GELU(W1_l LN2_l(x) + b1_l) + b2_l
// A row's attention reads rows of its own sequence only, so a wave that owns WHOLE sequences never needs another wave's rows: one wave owns one 16-row
// matrix-core tile = floor(16 / T) sequences of T <= 16 tokens (16 at T = 1, 5 at T = 3, 3 at T = 5, 1 from T = 9 on; the remaining rows of the tile are padding
// that re-reads a live row and stores nothing), and the residual stream of those rows stays in the wave's registers (D-tile order: lane (g, j) holds the features
// 16 t + 4 g + r of row j) for all layers.  HBM sees x once on the way in and the result once on the way out.
// Arithmetic: the split-f16 products of policy_f16x3.h (hx_split / hx_split2 / hx_erf2, v_mfma_f32_16x16x32_f16, hh and cross terms accumulated apart and combined
// once per output, the 2^-22 term dropped).  K = 72 is three K steps of 32, the last zero padded; fc2's K = 288 is nine steps; output widths 216 / 72 / 288 are
// 14 / 5 / 18 tiles.
// Per layer the wave's 16 x 216 LDS rows serve four purposes in turn: the residual rows on their way from the D-tile order into the B-operand order of the
// LayerNorm (both LayerNorms), the q | k | v rows, and the attention output (written over q).  The attention is the arithmetic of k_attention_causal_f32 in its
// order (online softmax, key 0 peeled) with one lane per (token row, head): 16 rows x 4 heads = 64; D = 18 is no multiple of 4 and a head starts every 72 bytes,
// hence 8-byte LDS accesses there.
// WEIGHT STREAM: T72_LAYER_ST = 28 stages of T72_STAGE_V = 768 16-byte vectors per layer (policies.py pack_trunk72_weights), all the same size so that one
// double-buffered LDS stage and one prefetch serve the whole launch, across layer boundaries too; lane = 16 g + i, p = 0 the high half, p = 1 the low half
// times 2^11, zero beyond the matrices:
//   stages  0 ..  6  (q | k | v, two output tiles each):  vector ((u * 3 + s) * 2 + p) * 64 + lane = Wqkv_p[16 (2 st + u) + i][32 s + 8 g + e]
//   stages  7 ..  9  (projection, the sixth tile zero):   the same form with Wproj
//   stages 10 + 2 k  (fc1 of hidden pair k = 0 .. 8):      vector ((tile * 3 + s) * 2 + p) * 64 + lane = W1_p[32 k + 16 tile + i][32 s + 8 g + e]
//   stages 11 + 2 k  (fc2, K step k; the sixth tile zero): vector (t * 2 + p) * 64 + lane = W2_p[16 t + i][32 k + 16 (e >> 2) + 4 g + (e & 3)]
// (the second product sums the 32 hidden units of a pair in the order the two D tiles of the first hold them, as in k_mlp_gelu_residual_f16x3).  The padding costs
// 10 % over the 312 KB of the bare tiles: 344 KB per layer, 1.35 MB for four layers - L2 resident.
// VECTORS: T72_VEC = 936 floats per layer, ln1.w | ln1.b | b_qkv (216) | b_proj | ln2.w | ln2.b | b1 (288) | b2, copied to LDS at the head of the layer.
// GUARD (d3il_f16x3_set_guard): four split sites per layer - the LN1 row, the attention output row, the LN2 row, the GELU outputs.  The lane's running key
// maximum / minimum live for the whole launch and are counted ONCE at its end: a row at most once per counter and launch.  A non-finite operand makes the B operands
// of its row NaN from there on (the minimum is sticky), so the row is NaN in every column; the next layer's attention makes the later tokens of its sequence NaN
// through their keys and values; rows of other sequences - of the same tile too - never read it (lane (g, j) holds data of row j only, the key loop stays inside
// the lane's sequence).
// No workspace, vector stores only, no inline assembly of its own; every branch in front of a barrier or shuffle depends on kernel arguments only.
#pragma once

namespace d3il {

constexpr int T72_C = 72, T72_H = 288, T72_NH = 4, T72_D = 18, T72_RS = 3 * T72_C;
constexpr int T72_STAGE_V = 768, T72_QKV_ST = 7, T72_PROJ_ST = 3, T72_PAIRS = T72_H / 32, T72_LAYER_ST = T72_QKV_ST + T72_PROJ_ST + 2 * T72_PAIRS;
constexpr int T72_LN1W = 0, T72_LN1B = 72, T72_BQKV = 144, T72_BPROJ = 360, T72_LN2W = 432, T72_LN2B = 504, T72_B1 = 576, T72_B2 = 864, T72_VEC = 936;
constexpr int T72_MAX_LAYERS = 8;
constexpr long T72_WIDE_TILES = 2048;      // from this many tiles on a launch uses workgroups of eight waves (256 CUs x 8), four below
static_assert(T72_LAYER_ST == 28 && T72_VEC % 4 == 0, "policies.py pack_trunk72_weights");

// Row `row` (72 floats in LDS, 16-byte aligned) in the B-operand order of v_mfma_f32_16x16x32_f16 - lane (g, j) holds, for K step s, the elements 32 s + 8 g + e of
// row j, zero beyond 72 (step 2: lane group 0 only) -, layer-normalised first if ln_w (biased variance; the four lane groups of a row hold 24 / 16 / 16 / 16 of
// its elements), split into the f16 halves: the 72-wide sibling of hx_load_row.  GUARD: the operands are a split site.
template <bool GUARD>
__device__ __forceinline__ void t72_load_row(const float* row, int g, const float* ln_w, const float* ln_b, float eps, hx_h8* hh, hx_h8* hl, unsigned& khi, unsigned& klo) {
  float v[24];
#pragma unroll
  for (int s = 0; s < 3; s++) {
    const int k0 = 32 * s + 8 * g;
    if (k0 < T72_C) {
      const hx_f4 a = *(const hx_f4*)(row + k0), b = *(const hx_f4*)(row + k0 + 4);
#pragma unroll
      for (int e = 0; e < 4; e++) { v[8 * s + e] = a[e]; v[8 * s + 4 + e] = b[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) v[8 * s + e] = 0.f;
    }
  }
  if (ln_w) {
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 24; k++) sum += v[k];
    sum += __shfl_xor(sum, 16); sum += __shfl_xor(sum, 32);
    const float mean = sum * (1.0f / T72_C);
    float var = 0.f;
#pragma unroll
    for (int s = 0; s < 3; s++) if (32 * s + 8 * g < T72_C) {
#pragma unroll
      for (int e = 0; e < 8; e++) { const float d = v[8 * s + e] - mean; var += d * d; }
    }
    var += __shfl_xor(var, 16); var += __shfl_xor(var, 32);
    const float rstd = 1.0f / sqrtf(var * (1.0f / T72_C) + eps);
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const int k0 = 32 * s + 8 * g;
      if (k0 < T72_C) {
        const hx_f4 w0 = *(const hx_f4*)(ln_w + k0), w1 = *(const hx_f4*)(ln_w + k0 + 4), b0 = *(const hx_f4*)(ln_b + k0), b1 = *(const hx_f4*)(ln_b + k0 + 4);
#pragma unroll
        for (int e = 0; e < 4; e++) {
          v[8 * s + e] = (v[8 * s + e] - mean) * rstd * w0[e] + b0[e];
          v[8 * s + 4 + e] = (v[8 * s + 4 + e] - mean) * rstd * w1[e] + b1[e];
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 3; s++)
#pragma unroll
    for (int e = 0; e < 8; e++) { _Float16 a, b; hx_split(v[8 * s + e], a, b); hh[s][e] = a; hl[s][e] = b; }
  if constexpr (GUARD) {
#pragma unroll
    for (int k = 0; k < 24; k++) hx_track(v[k], khi, klo);
    const bool bad = klo < HXG_BIAS;
#pragma unroll
    for (int s = 0; s < 3; s++) { hh[s] = hx_poison(hh[s], bad); hl[s] = hx_poison(hl[s], bad); }
  }
}

template <int NW, bool GUARD = false>      // waves (tiles of 16 rows) per workgroup: they share one pass over the weight stream
__global__ __launch_bounds__(64 * NW) void k_gpt_trunk72_f16x3(const float* __restrict__ x, const hx_h8* __restrict__ wp, const float* __restrict__ vec, float eps,
                                                              float* __restrict__ out, long n_seq, int T, int n_layer, long long* counts = nullptr) {
  constexpr int C = T72_C, D = T72_D, RS = T72_RS;
  __shared__ __attribute__((aligned(16))) hx_h8 sw[2][T72_STAGE_V];
  __shared__ __attribute__((aligned(16))) float svec[T72_VEC];
  __shared__ __attribute__((aligned(16))) float qs[NW][16][RS];
  static_assert(sizeof(hx_h8) * 2 * T72_STAGE_V + sizeof(float) * T72_VEC + sizeof(float) * NW * 16 * RS <= 160 * 1024, "LDS of a gfx950 CU");
  static_assert((RS * sizeof(float)) % 16 == 0 && (D * sizeof(float)) % 8 == 0 && (C * sizeof(float)) % 16 == 0, "vector accesses of the LDS rows");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  constexpr int NT = 64 * NW, VPT = (T72_STAGE_V + NT - 1) / NT;
  const int rows_tile = (16 / T) * T;      // live rows of a full tile: whole sequences only
  const long M = n_seq * T, row = ((long)blockIdx.x * NW + wave) * rows_tile + j;
  const bool live = j < rows_tile && row < M;
  const long rr = live ? row : M - 1;
  // this lane's place in the attention: the first row of its sequence in the tile and its own position (a padding row is a sequence of its own)
  const int js = j < rows_tile ? (j / T) * T : j, pos = j - js;
  float (*const my)[RS] = qs[wave];
  const int total = T72_LAYER_ST * n_layer;
  int gs = 0, cur = 0;      // the stage of the whole launch the products work on, and its LDS buffer
  hx_h8 pre[VPT];
  auto stage_begin = [&]() {
    if (gs + 1 < total) {
#pragma unroll
      for (int q = 0; q < VPT; q++) if (tid + NT * q < T72_STAGE_V) pre[q] = wp[(long)(gs + 1) * T72_STAGE_V + tid + NT * q];
    }
  };
  auto stage_end = [&]() {
    if (gs + 1 < total) {
#pragma unroll
      for (int q = 0; q < VPT; q++) if (tid + NT * q < T72_STAGE_V) sw[cur ^ 1][tid + NT * q] = pre[q];
    }
    __syncthreads();
    cur ^= 1; gs++;
  };
  hx_h8 hh[3], hl[3];
  unsigned khi = 0u, klo = ~0u;      // the guard's running key maximum / minimum of this lane (GUARD only), for the whole launch
  // one output tile of a 72-deep product from the current stage: hh terms and cross terms apart
  auto tile3 = [&](int base, hx_f4& ah, hx_f4& ax) {
    hx_f4 a = hx_f4{0.f, 0.f, 0.f, 0.f}, x1 = a, x2 = a;
#pragma unroll
    for (int s = 0; s < 3; s++) {
      const hx_h8 wh = sw[cur][base + (s * 2) * 64 + lane], wl = sw[cur][base + (s * 2 + 1) * 64 + lane];
      a = HX_MFMA(wh, hh[s], a);
      x1 = HX_MFMA(wh, hl[s], x1);
      x2 = HX_MFMA(wl, hh[s], x2);
    }
    ah = a; ax = x1 + x2;
  };
  // the residual rows, D-tile order: xr[t][r] = x[row j][16 t + 4 g + r] (tile 4: lane groups 0 and 1 only)
  hx_f4 xr[5];
#pragma unroll
  for (int t = 0; t < 5; t++) {
    const int col = 16 * t + 4 * g;
    xr[t] = col < C ? *(const hx_f4*)(x + rr * C + col) : hx_f4{0.f, 0.f, 0.f, 0.f};
  }
  auto rows_to_lds = [&]() {
#pragma unroll
    for (int t = 0; t < 5; t++) {
      const int col = 16 * t + 4 * g;
      if (col < C) *(hx_f4*)(&my[j][col]) = xr[t];
    }
  };
#pragma unroll
  for (int q = 0; q < VPT; q++) if (tid + NT * q < T72_STAGE_V) sw[0][tid + NT * q] = wp[tid + NT * q];

  for (int l = 0; l < n_layer; l++) {
    // ---- the layer's vectors; the residual rows into the B-operand order through the wave's LDS rows; LN1
    // (every lane has passed the barrier that ended the previous layer's last stage: nobody reads svec or the rows any more)
    for (int q = tid; q < T72_VEC / 4; q += NT) ((hx_f4*)svec)[q] = ((const hx_f4*)(vec + (long)l * T72_VEC))[q];
    rows_to_lds();
    __syncthreads();
    t72_load_row<GUARD>(my[j], g, svec + T72_LN1W, svec + T72_LN1B, eps, hh, hl, khi, klo);
    __syncthreads();
    // ---- q | k | v rows into LDS
    for (int st = 0; st < T72_QKV_ST; st++) {
      stage_begin();
#pragma unroll
      for (int u = 0; u < 2; u++) {
        hx_f4 ah, ax;
        tile3(384 * u, ah, ax);
        const int col = 16 * (2 * st + u) + 4 * g;
        if (col < 3 * C) *(hx_f4*)(&my[j][col]) = ah + ax * HX_ILO + *(const hx_f4*)(svec + T72_BQKV + col);
      }
      stage_end();
    }
    // ---- causal attention: lane (g, j) serves row j and head g, keys js .. js + pos of its own sequence (as k_attention_causal_f32: online softmax, key 0 peeled)
    {
      const float scale = 1.0f / sqrtf((float)D);
      auto ld = [&](const float* ptr, float* r) {
#pragma unroll
        for (int c = 0; c < D / 2; c++) { const hx_f2 t2 = *(const hx_f2*)(ptr + 2 * c); r[2 * c] = t2[0]; r[2 * c + 1] = t2[1]; }
      };
      float q[D], acc[D], kk[D], vv[D];
      ld(&my[j][g * D], q);
#pragma unroll
      for (int d = 0; d < D; d++) q[d] *= scale;
      ld(&my[js][C + g * D], kk); ld(&my[js][2 * C + g * D], acc);
      float m = 0.0f, lsum = 1.0f;
#pragma unroll
      for (int d = 0; d < D; d++) m += q[d] * kk[d];
      for (int jj = 1; jj <= pos; jj++) {
        ld(&my[js + jj][C + g * D], kk); ld(&my[js + jj][2 * C + g * D], vv);
        float sc = 0.0f;
#pragma unroll
        for (int d = 0; d < D; d++) sc += q[d] * kk[d];
        const float mn = fmaxf(m, sc), corr = __expf(m - mn), pj = __expf(sc - mn);
        lsum = lsum * corr + pj;
#pragma unroll
        for (int d = 0; d < D; d++) acc[d] = acc[d] * corr + pj * vv[d];
        m = mn;
      }
      const float inv = 1.0f / lsum;
#pragma unroll
      for (int c = 0; c < D / 2; c++) *(hx_f2*)(&my[j][g * D + 2 * c]) = hx_f2{acc[2 * c] * inv, acc[2 * c + 1] * inv};
    }
    __syncthreads();
    // ---- the attention output of row j as the B operand of the projection (a split site)
    t72_load_row<GUARD>(my[j], g, nullptr, nullptr, 0.f, hh, hl, khi, klo);
    // ---- x1 = x + proj(y) + bproj
#pragma unroll
    for (int st = 0; st < T72_PROJ_ST; st++) {
      stage_begin();
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int t = 2 * st + u;
        if (t < 5) {
          hx_f4 ah, ax;
          tile3(384 * u, ah, ax);
          const int col = 16 * t + 4 * g;
          const hx_f4 bb = col < C ? *(const hx_f4*)(svec + T72_BPROJ + col) : hx_f4{0.f, 0.f, 0.f, 0.f};
          xr[t] = ah + ax * HX_ILO + bb + xr[t];
        }
      }
      stage_end();
    }
    // ---- LN2 of x1 (the projection's stages have ended with barriers: the attention output rows are free)
    rows_to_lds();
    __syncthreads();
    t72_load_row<GUARD>(my[j], g, svec + T72_LN2W, svec + T72_LN2B, eps, hh, hl, khi, klo);
    // ---- x = x1 + b2 + W2 GELU(W1 LN2(x1) + b1), hidden pair by hidden pair
    hx_f4 acc2h[5], acc2x[5];
#pragma unroll
    for (int t = 0; t < 5; t++) { acc2h[t] = hx_f4{0.f, 0.f, 0.f, 0.f}; acc2x[t] = acc2h[t]; }
    for (int k = 0; k < T72_PAIRS; k++) {
      stage_begin();
      hx_h8 gh, gl;
#pragma unroll
      for (int tile = 0; tile < 2; tile++) {
        hx_f4 ch, cx;
        tile3(384 * tile, ch, cx);
        const hx_f4 v4 = ch + cx * HX_ILO + *(const hx_f4*)(svec + T72_B1 + 32 * k + 16 * tile + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          const hx_f2 v = hx_f2{v4[r], v4[r + 1]};
          const hx_f2 gv = (v * 0.5f) * (hx_erf2(v * 0.70710678118654752440f) + 1.0f);      // nn.GELU() (exact form)
          hx_h2 a2, b2;
          hx_split2(gv, a2, b2);
          gh[4 * tile + r] = a2[0]; gh[4 * tile + r + 1] = a2[1]; gl[4 * tile + r] = b2[0]; gl[4 * tile + r + 1] = b2[1];
          if constexpr (GUARD) { hx_track(gv[0], khi, klo); hx_track(gv[1], khi, klo); }
        }
      }
      if constexpr (GUARD) { const bool bad = klo < HXG_BIAS; gh = hx_poison(gh, bad); gl = hx_poison(gl, bad); }
      stage_end();
      stage_begin();
#pragma unroll
      for (int t = 0; t < 5; t++) {
        const hx_h8 wh = sw[cur][(t * 2) * 64 + lane], wl = sw[cur][(t * 2 + 1) * 64 + lane];
        acc2h[t] = HX_MFMA(wh, gh, acc2h[t]);
        acc2x[t] = HX_MFMA(wh, gl, acc2x[t]);
        acc2x[t] = HX_MFMA(wl, gh, acc2x[t]);
      }
      stage_end();
    }
#pragma unroll
    for (int t = 0; t < 5; t++) {
      const int col = 16 * t + 4 * g;
      const hx_f4 bb = col < C ? *(const hx_f4*)(svec + T72_B2 + col) : hx_f4{0.f, 0.f, 0.f, 0.f};
      xr[t] = xr[t] + bb + acc2h[t] + acc2x[t] * HX_ILO;
    }
    __syncthreads();      // b2 has been read by every wave before the next layer's vectors replace it
  }
  if constexpr (GUARD) hx_guard_count(live, khi, klo, counts);
  if (!live) return;
#pragma unroll
  for (int t = 0; t < 5; t++) {
    const int col = 16 * t + 4 * g;
    if (col < C) *(hx_f4*)(out + row * C + col) = xr[t];
  }
}

}  // namespace d3il
