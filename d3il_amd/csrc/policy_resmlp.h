// policy_resmlp.h - the device code of the reference's ResidualMLPNetwork (agents/models/common/mlp.py:114-182: Linear, n pre-activation residual blocks
// x + l2(mish(l1(mish(x)))), Linear), written once (included by rollout.hip behind policy_f32.h: mlp_f4 and dd_mish are there).  k_resmlp_f32 - the network of the BC
// agent, bc_agent.py:240-271 - is here; k_cvae_decode, k_ddpm_mlp_chain and k_bc_gmm build their trunks from the pieces below (k_bet_mlp uses rm_layer only).
//
// Tiling, the same operand scheme as k_ddpm_mlp_f32: a workgroup of eight waves owns 16 rows; the waves share the HID / 16 output tiles of a layer (wave w: tiles
// TPW w .. TPW (w + 1) - 1, TPW = HID / 128), the weights stream from L2 in the packed operand order (d3il_amd/policies.py pack_resmlp_weights), the activations go
// from layer to layer through LDS in B-operand order - xb[buf][t][lane (g, j)] = features 16 t + 4 g + r of row j, the D registers of one layer are the B operand of
// the next -, one barrier per layer, the block count is a loop bound.  HID = 128 or 256.  The kernel owns ``xb`` (2 x NT x 64 float4: 16 / 32 KB), its tiles ``xo`` of
// the residual stream and the buffer index ``buf``; the pieces take them as arguments.  Every piece is called by all eight waves unless it says otherwise; none has
// a branch in front of its barriers.  Rows never mix: column j of every matrix-core product is row j.
#pragma once

namespace d3il {

// y[q] = (RES ? y[q] : 0) + bias + W m for the wave's output tiles TPW w + q of one packed HID x HID layer (xin: the 16 rows' activations in LDS)
template <int HID, bool RES>
__device__ __forceinline__ void rm_layer(const mlp_f4* __restrict__ wl, const float* __restrict__ bias, const mlp_f4* xin, mlp_f4* y, int w, int lane, int g) {
  constexpr int NT = HID / 16, TPW = NT / 8;
  mlp_f4 m[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) m[t] = xin[t * 64 + lane];
#pragma unroll
  for (int q = 0; q < TPW; q++) {
    const int To = TPW * w + q;
    const mlp_f4* wt = wl + (long)To * (NT * 64) + lane;
    mlp_f4 a[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) a[t] = wt[t * 64];
    mlp_f4 acc[4];
    acc[0] = *(const mlp_f4*)(bias + 16 * To + 4 * g);
    acc[1] = RES ? y[q] : mlp_f4{0.f, 0.f, 0.f, 0.f};
    acc[2] = mlp_f4{0.f, 0.f, 0.f, 0.f}; acc[3] = mlp_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][r], m[t][r], acc[r], 0, 0, 0);
    y[q] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
}
// the wave's tiles into one activation buffer, as they are or through Mish; the caller's barrier makes them the next layer's input
template <int HID, bool MISH>
__device__ __forceinline__ void rm_store(mlp_f4* xbuf, const mlp_f4* y, int w, int lane) {
  constexpr int TPW = HID / 128;
#pragma unroll
  for (int q = 0; q < TPW; q++) xbuf[(TPW * w + q) * 64 + lane] = MISH ? mlp_f4{dd_mish(y[q][0]), dd_mish(y[q][1]), dd_mish(y[q][2]), dd_mish(y[q][3])} : y[q];
}
// the residual blocks on the wave's tiles xo: two layers and two barriers per block.  Behind it xb[buf] is free to be written (its last reader was the layer
// before the last barrier).  The loop runs on copies of xo and buf and its two Mish stores are written out in it, not calls of rm_store: the optimiser simplifies
// this function on its own before it reaches a kernel, and only with the tiles as values of the loop (not memory behind a reference) and dd_mish in the loop's
// own body does it turn dd_mish's early-out into selects, as it does in a kernel that holds this loop as text (profiles/resmlp_trunk/README.md).
template <int HID>
__device__ __forceinline__ void rm_blocks(const float* w_blk, const float* b_blk, int nblk, mlp_f4 (&xb)[2][HID * 4], mlp_f4 (&xo)[HID / 128], int& buf,
                                          int w, int lane, int g) {
  constexpr int NT = HID / 16, TPW = NT / 8, LAYER_F4 = NT * NT * 64;
  mlp_f4 x[TPW];
  int bf = buf;
#pragma unroll
  for (int q = 0; q < TPW; q++) x[q] = xo[q];
#pragma clang loop unroll(disable)
  for (int b = 0; b < nblk; b++) {
    mlp_f4 y[TPW];
#pragma unroll
    for (int q = 0; q < TPW; q++) xb[bf][(TPW * w + q) * 64 + lane] = mlp_f4{dd_mish(x[q][0]), dd_mish(x[q][1]), dd_mish(x[q][2]), dd_mish(x[q][3])};
    __syncthreads();
    rm_layer<HID, false>((const mlp_f4*)w_blk + (long)(2 * b) * LAYER_F4, b_blk + (2 * b) * HID, xb[bf], y, w, lane, g);
    bf ^= 1;
#pragma unroll
    for (int q = 0; q < TPW; q++) xb[bf][(TPW * w + q) * 64 + lane] = mlp_f4{dd_mish(y[q][0]), dd_mish(y[q][1]), dd_mish(y[q][2]), dd_mish(y[q][3])};
    __syncthreads();
    rm_layer<HID, true>((const mlp_f4*)w_blk + (long)(2 * b + 1) * LAYER_F4, b_blk + (2 * b + 1) * HID, xb[bf], x, w, lane, g);      // the residual rides in the accumulator
    bf ^= 1;
  }
#pragma unroll
  for (int q = 0; q < TPW; q++) xo[q] = x[q];
  buf = bf;
}
// the lane's share of a row of at most 28 features: lane (g, j) holds feature 4 s2 + g of row j (rr: the row, clamped to the last live one by the caller)
__device__ __forceinline__ void rm_load_row28(const float* x, long rr, int IN, int g, float* in_k) {
#pragma unroll
  for (int s2 = 0; s2 < 7; s2++) { const int f = 4 * s2 + g; in_k[s2] = f < IN ? x[rr * IN + f] : 0.f; }
}
// the input layer on such a row: xo = b_in + W_in x, 7 matrix-core steps per tile on weights packed to 32 columns (two float4 per lane and tile)
template <int HID>
__device__ __forceinline__ void rm_input28(const float* w_in, const float* b_in, const float* in_k, mlp_f4* xo, int w, int lane, int g) {
  constexpr int TPW = HID / 128;
  const mlp_f4* w_in4 = (const mlp_f4*)w_in;
#pragma unroll
  for (int q = 0; q < TPW; q++) {
    const int To = TPW * w + q;
    mlp_f4 acc = *(const mlp_f4*)(b_in + 16 * To + 4 * g);
    const mlp_f4 a0 = w_in4[(To * 64 + lane) * 2], a1 = w_in4[(To * 64 + lane) * 2 + 1];
#pragma unroll
    for (int s2 = 0; s2 < 7; s2++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s2 < 4 ? a0[s2] : a1[s2 - 4], in_k[s2], acc, 0, 0, 0);
    xo[q] = acc;
  }
}
// the input layer on a row of 64 features (in_k[16]): 16 steps per tile on two accumulators, weights packed to 64 columns (four float4 per lane and tile); the
// first accumulator starts from the bias or, without one (b_in is not read), from zero
template <int HID, bool BIAS>
__device__ __forceinline__ void rm_input64(const float* w_in, const float* b_in, const float* in_k, mlp_f4* xo, int w, int lane, int g) {
  constexpr int TPW = HID / 128;
  const mlp_f4* w_in4 = (const mlp_f4*)w_in;
#pragma unroll
  for (int q = 0; q < TPW; q++) {
    const int To = TPW * w + q;
    mlp_f4 acc = BIAS ? *(const mlp_f4*)(b_in + 16 * To + 4 * g) : mlp_f4{0.f, 0.f, 0.f, 0.f}, acc2 = mlp_f4{0.f, 0.f, 0.f, 0.f};
    mlp_f4 aw[4];
#pragma unroll
    for (int c = 0; c < 4; c++) aw[c] = w_in4[(To * 64 + lane) * 4 + c];
#pragma unroll
    for (int s2 = 0; s2 < 16; s2 += 2) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[s2 >> 2][s2 & 3], in_k[s2], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[(s2 + 1) >> 2][(s2 + 1) & 3], in_k[s2 + 1], acc2, 0, 0, 0);
    }
    xo[q] = acc + acc2;
  }
}
// one 16-row output tile over K = HID on two accumulators: acc0 + W m, W the packed tile at ``wt`` ([t][lane][r]), m the 16 rows' activations in LDS.  Lane (g, j),
// register r of the result = output 4 g + r of row j.  One wave's work.
template <int HID>
__device__ __forceinline__ mlp_f4 rm_tile(const mlp_f4* wt, const mlp_f4* xin, mlp_f4 acc0, int lane) {
  mlp_f4 acc = acc0, acc2 = mlp_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < HID / 16; t++) {
    const mlp_f4 a4 = wt[t * 64 + lane], m4 = xin[t * 64 + lane];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0], m4[0], acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1], m4[1], acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[2], m4[2], acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[3], m4[3], acc2, 0, 0, 0);
  }
  return acc + acc2;
}
// the dot product of the row-major weight row ``wr`` with row jr of the activations in LDS: this lane's float4 chunks sub, sub + 8, ..; the caller sums the eight
// lanes.
template <int HID>
__device__ __forceinline__ float rm_row_part(const float* wr, const mlp_f4* xf, int sub, int jr) {
  float part = 0.f;
#pragma unroll
  for (int jj = 0; jj < HID / 32; jj++) {
    const int q = sub + 8 * jj;      // features 4 q .. 4 q + 3: tile q / 4, lane group q % 4
    const mlp_f4 wv = *(const mlp_f4*)(wr + 4 * q), xv = xf[(q >> 2) * 64 + (q & 3) * 16 + jr];
    part += fmaf(wv[3], xv[3], fmaf(wv[2], xv[2], fmaf(wv[1], xv[1], wv[0] * xv[0])));
  }
  return part;
}
// a row's non-finite verdict: the OR over the four lane groups of column j, which hold its features 4 s + g (or its outputs 4 g + r) between them
__device__ __forceinline__ unsigned rm_row_or(unsigned bad) {
  bad |= (unsigned)__shfl_xor((int)bad, 16); bad |= (unsigned)__shfl_xor((int)bad, 32);
  return bad;
}

// The network in one launch: at most 28 inputs and 16 outputs.  The hot kernel of the BC policy keeps the input layer, the block loop and the output tile as text:
// built from rm_input28 / rm_blocks / rm_tile it ran 1 to 4 % slower (profiles/resmlp_trunk/README.md); as written it compiles to the instructions it had
// before this header existed.  k_bet_mlp (policy_bet_mlp.h) keeps its trunk as text for the same reason (hidden 256: 5 % slower from the pieces).  Keep these
// copies in step with the pieces above.
template <int HID>
__global__ __launch_bounds__(512) void k_resmlp_f32(const float* __restrict__ x, const float* __restrict__ w_in, const float* __restrict__ b_in, const float* __restrict__ w_blk,
                                                     const float* __restrict__ b_blk, const float* __restrict__ w_out, const float* __restrict__ b_out, float* __restrict__ out,
                                                     long n, int IN, int OUT, int nblk) {
  constexpr int NT = HID / 16, TPW = NT / 8, LAYER_F4 = NT * NT * 64;
  __shared__ mlp_f4 xb[2][NT * 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const long row = (long)blockIdx.x * 16 + j;
  const bool live = row < n;
  const long rr = live ? row : (n - 1);
  float in_k[7];
  rm_load_row28(x, rr, IN, g, in_k);
  const mlp_f4* w_in4 = (const mlp_f4*)w_in;
  const mlp_f4* w_out4 = (const mlp_f4*)w_out;
  mlp_f4 xo[TPW];
#pragma unroll
  for (int q = 0; q < TPW; q++) {      // (rm_input28, as text)
    const int To = TPW * w + q;
    mlp_f4 acc = *(const mlp_f4*)(b_in + 16 * To + 4 * g);
    const mlp_f4 a0 = w_in4[(To * 64 + lane) * 2], a1 = w_in4[(To * 64 + lane) * 2 + 1];
#pragma unroll
    for (int s2 = 0; s2 < 7; s2++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s2 < 4 ? a0[s2] : a1[s2 - 4], in_k[s2], acc, 0, 0, 0);
    xo[q] = acc;
  }
  int buf = 0;
#pragma clang loop unroll(disable)
  for (int b = 0; b < nblk; b++) {      // (rm_blocks, as text)
    mlp_f4 y[TPW];
#pragma unroll
    for (int q = 0; q < TPW; q++) xb[buf][(TPW * w + q) * 64 + lane] = mlp_f4{dd_mish(xo[q][0]), dd_mish(xo[q][1]), dd_mish(xo[q][2]), dd_mish(xo[q][3])};
    __syncthreads();
    rm_layer<HID, false>((const mlp_f4*)w_blk + (long)(2 * b) * LAYER_F4, b_blk + (2 * b) * HID, xb[buf], y, w, lane, g);
    buf ^= 1;
#pragma unroll
    for (int q = 0; q < TPW; q++) xb[buf][(TPW * w + q) * 64 + lane] = mlp_f4{dd_mish(y[q][0]), dd_mish(y[q][1]), dd_mish(y[q][2]), dd_mish(y[q][3])};
    __syncthreads();
    rm_layer<HID, true>((const mlp_f4*)w_blk + (long)(2 * b + 1) * LAYER_F4, b_blk + (2 * b + 1) * HID, xb[buf], xo, w, lane, g);
    buf ^= 1;
  }
  rm_store<HID, false>(xb[buf], xo, w, lane);
  __syncthreads();
  if (w != 0) return;      // (after the last barrier) the output tile is one wave's work
  mlp_f4 acc = mlp_f4{0.f, 0.f, 0.f, 0.f}, acc2 = mlp_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < NT; t++) {      // (rm_tile, as text)
    const mlp_f4 a4 = w_out4[t * 64 + lane], m4 = xb[buf][t * 64 + lane];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0], m4[0], acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1], m4[1], acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[2], m4[2], acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[3], m4[3], acc2, 0, 0, 0);
  }
  acc += acc2;
  if (live) {
#pragma unroll
    for (int r = 0; r < 4; r++) if (4 * g + r < OUT) out[row * OUT + 4 * g + r] = acc[r] + b_out[4 * g + r];
  }
}

}  // namespace d3il
