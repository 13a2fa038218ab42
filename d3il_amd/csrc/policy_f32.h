// policy_f32.h - the f32 matrix-core kernels of the batched policies (included by rollout.hip behind policy_common.h): the transformer-block pieces of the
// DiffusionGPT / minGPT trunks at n_embd 120 (k_mlp_gelu_residual_f32, k_linear120_f32, k_layernorm_f32, k_attention_causal_f32) and the fused DDPM-MLP sampling
// chain (k_ddpm_mlp_f32), with mlp_f4 and dd_mish, which the ResidualMLPNetwork trunk of policy_resmlp.h reuses.  The C ABI wrappers (d3il_*_f32) are in rollout.hip.
#pragma once

namespace d3il {

// Causal self-attention for the short token sequences of the BESO policy (DiffusionGPT of BASELINE config 5: T = 11 tokens, 6 heads
// of 20): one lane per (sequence b, head h, query i).  qkv: f32 [B * T][3 C] (query | key | value of a token, C = H * D, as written
// by ONE fused linear layer), out: f32 [B * T][C] in token-major layout (what the output projection reads) - no transposes, no
// [B, H, T, T] score tensor, no batched GEMM of 11 x 20 matrices.  Softmax over the keys j <= i with the 1 / sqrt(D) scaling
// (score_gpts.py:59-76).  D <= 32, T <= 32.
// LayerNorm over the last dimension for the narrow rows of the policy transformer (C = 120): 32 lanes per row, four consecutive
// floats per lane (C <= 128, C a multiple of 4), two rows per wave; mean and variance by xor shuffles inside the half wave; the
// biased variance and eps inside the square root like torch.nn.LayerNorm.  x, y: f32 [rows][C].
// Fused transformer MLP of the batched DiffusionGPT policy (score_gpts.py:83-115: x + fc2(GELU(fc1(ln2(x)))), n_embd 120, hidden 480), f32 on the matrix
// cores: out[M][120] = x + b2 + W2 GELU(W1 h + b1) for the [B * T][120] activations of the BESO policy.  One wave owns 16 rows; per chunk
// of 16 hidden units it runs the TRANSPOSED first product D1[hid][row] = W1c[16 x 120] h^T[120 x 16] with v_mfma_f32_16x16x4_f32 (30 steps), applies bias +
// GELU to its four D registers and feeds them STRAIGHT BACK as the B operand of the second product D2[out][row] += W2c[128 x 16] G[16 x 16] (8 tiles x 4
// steps) - the D layout (lane = row, register r of lane group g = hidden 4 g + r) is already a B layout when step e of the second product sums the hidden
// units {4 g + e}, which only fixes how the W2 chunk is packed - so the hidden activations never leave the registers.  Weights arrive pre-packed per chunk
// in exactly the LDS order (16 blocks of [4 g][16 i][4 e] floats, one float4 per lane: d3il_amd/policies.py pack_mlp_weights), double-buffered in LDS and shared by the four waves of
// a workgroup.  1860 MFMAs per 16 rows; 14.7 MFLOP per 64-row workgroup against 32 KB of weight traffic from L2.
typedef float mlp_f4 __attribute__((ext_vector_type(4)));
constexpr int MLP_C = 120, MLP_H = 480, MLP_CHUNKS = MLP_H / 16, MLP_CHUNK_F = 16 * 256;      // floats per packed chunk
// The row of a lane in the B-operand order of the products below: lane (g, j) holds elements 4 s + g of row j.  With ln_w the row is layer-normalised
// first (nn.LayerNorm over the 120 features, biased variance): the four lane groups of a row each hold 30 of its elements, so the two row sums are
// a 30-term sum per lane and two cross-group exchanges.
__device__ __forceinline__ void mlp_load_row(const float* __restrict__ src, long rr, int g, const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps, float* hk) {
#pragma unroll
  for (int s2 = 0; s2 < MLP_C / 4; s2++) hk[s2] = src[rr * MLP_C + 4 * s2 + g];
  if (ln_w) {
    float sum = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < MLP_C / 4; s2++) sum += hk[s2];
    sum += __shfl_xor(sum, 16); sum += __shfl_xor(sum, 32);
    const float mean = sum * (1.0f / MLP_C);
    float var = 0.f;
#pragma unroll
    for (int s2 = 0; s2 < MLP_C / 4; s2++) { const float d = hk[s2] - mean; var += d * d; }
    var += __shfl_xor(var, 16); var += __shfl_xor(var, 32);
    const float rstd = 1.0f / sqrtf(var * (1.0f / MLP_C) + eps);
#pragma unroll
    for (int s2 = 0; s2 < MLP_C / 4; s2++) hk[s2] = (hk[s2] - mean) * rstd * ln_w[4 * s2 + g] + ln_b[4 * s2 + g];
  }
}
__global__ __launch_bounds__(256) void k_mlp_gelu_residual_f32(const float* __restrict__ h, const float* __restrict__ x, const float* __restrict__ wp,
                                                                const float* __restrict__ b1, const float* __restrict__ b2, float* __restrict__ out, long M,
                                                                const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps) {
  __shared__ mlp_f4 sw[2][MLP_CHUNK_F / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const long row0 = (long)blockIdx.x * 64 + wave * 16, row = row0 + j;
  const bool live = row < M;
  const long rr = live ? row : (M - 1);
  float hk[MLP_C / 4];
  mlp_load_row(h, rr, g, ln_w, ln_b, eps, hk);
  mlp_f4 acc2[8];
#pragma unroll
  for (int t = 0; t < 8; t++) acc2[t] = mlp_f4{0.f, 0.f, 0.f, 0.f};
  const mlp_f4* wp4 = (const mlp_f4*)wp;
  mlp_f4 pre[4];
#pragma unroll
  for (int q = 0; q < 4; q++) sw[0][tid + 256 * q] = wp4[tid + 256 * q];
  __syncthreads();
  for (int c = 0; c < MLP_CHUNKS; c++) {
    const int cur = c & 1;
    if (c + 1 < MLP_CHUNKS) {
#pragma unroll
      for (int q = 0; q < 4; q++) pre[q] = wp4[(long)(c + 1) * (MLP_CHUNK_F / 4) + tid + 256 * q];
    }
    mlp_f4 acc1 = mlp_f4{0.f, 0.f, 0.f, 0.f}, acc1b = mlp_f4{0.f, 0.f, 0.f, 0.f};      // two accumulators: the dependent MFMA chain is half as long
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const mlp_f4 a4 = sw[cur][q * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; e++) if (4 * q + e < MLP_C / 4) {
        if (e & 1) acc1b = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], hk[4 * q + e], acc1b, 0, 0, 0);
        else acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], hk[4 * q + e], acc1, 0, 0, 0);
      }
    }
    acc1 += acc1b;
    float gv[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const float v = acc1[r] + b1[16 * c + 4 * g + r];
      gv[r] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));      // nn.GELU() (exact)
    }
#pragma unroll
    for (int t = 0; t < 8; t++) {
      const mlp_f4 a4 = sw[cur][(8 + t) * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; e++) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], gv[e], acc2[t], 0, 0, 0);
    }
    if (c + 1 < MLP_CHUNKS) {
#pragma unroll
      for (int q = 0; q < 4; q++) sw[cur ^ 1][tid + 256 * q] = pre[q];
    }
    __syncthreads();
  }
  if (!live) return;
#pragma unroll
  for (int t = 0; t < 8; t++) {
    const int col = 16 * t + 4 * g;
    if (col >= MLP_C) continue;
    const mlp_f4 xr = *(const mlp_f4*)(x + row * MLP_C + col), bb = *(const mlp_f4*)(b2 + col);
    *(mlp_f4*)(out + row * MLP_C + col) = xr + bb + acc2[t];
  }
}
// out[M][N] = (LayerNorm)(xin)[M][120] W^T + bias (+ resid): the linear layers of the DiffusionGPT block with 120 input features (query | key | value in
// one product, the attention output projection with the residual) on the f32 matrix cores.  Same operand scheme as the first product of the MLP kernel:
// D[n][row] per tile of 16 outputs (30 MFMA steps), the lane's four D registers are four consecutive outputs of its row - one float4 store.
__global__ __launch_bounds__(256) void k_linear120_f32(const float* __restrict__ xin, const float* __restrict__ wp, const float* __restrict__ bias, const float* __restrict__ resid,
                                                        float* __restrict__ out, long M, int N, const float* __restrict__ ln_w, const float* __restrict__ ln_b, float eps) {
  __shared__ mlp_f4 sw[2][8 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, g = lane >> 4;
  const long row = (long)blockIdx.x * 64 + wave * 16 + j;
  const bool live = row < M;
  const long rr = live ? row : (M - 1);
  float hk[MLP_C / 4];
  mlp_load_row(xin, rr, g, ln_w, ln_b, eps, hk);
  const int ntiles = (N + 15) / 16;
  const mlp_f4* wp4 = (const mlp_f4*)wp;
  mlp_f4 pre[2];
#pragma unroll
  for (int q = 0; q < 2; q++) sw[0][tid + 256 * q] = wp4[tid + 256 * q];
  __syncthreads();
  for (int t = 0; t < ntiles; t++) {
    const int cur = t & 1;
    if (t + 1 < ntiles) {
#pragma unroll
      for (int q = 0; q < 2; q++) pre[q] = wp4[(long)(t + 1) * 512 + tid + 256 * q];
    }
    mlp_f4 acc = mlp_f4{0.f, 0.f, 0.f, 0.f}, acc_b = mlp_f4{0.f, 0.f, 0.f, 0.f};      // two accumulators: the dependent MFMA chain is half as long
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const mlp_f4 a4 = sw[cur][q * 64 + lane];
#pragma unroll
      for (int e = 0; e < 4; e++) if (4 * q + e < MLP_C / 4) {
        if (e & 1) acc_b = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], hk[4 * q + e], acc_b, 0, 0, 0);
        else acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], hk[4 * q + e], acc, 0, 0, 0);
      }
    }
    const int col = 16 * t + 4 * g;
    if (live && col < N) {
      mlp_f4 v = acc + acc_b + *(const mlp_f4*)(bias + col);
      if (resid) v += *(const mlp_f4*)(resid + row * (long)N + col);
      *(mlp_f4*)(out + row * (long)N + col) = v;
    }
    if (t + 1 < ntiles) {
#pragma unroll
      for (int q = 0; q < 2; q++) sw[cur ^ 1][tid + 256 * q] = pre[q];
    }
    __syncthreads();
  }
}
// The whole sampling chain of the reference's DDPM policy (agents/models/diffusion/gc_diffusion.py:101-216 over diffusion_models.py:20-118 and
// common/mlp.py:9-46,114-182 as configs/agents/ddpm_agent.yaml + scripts/sorting_4/ddpm_benchmark.sh configure them: DiffusionMLP, hidden 256, 8 hidden layers =
// 4 pre-activation residual blocks, Mish, t_dim 8, window 1) in ONE kernel, f32 on the matrix cores.  Rows are independent: a workgroup owns 16 rows for all T
// denoising steps and all layers, its DD_NW waves each own DD_TPW of the 16 output tiles of every layer (wave w: outputs 16 DD_TPW w .. 16 DD_TPW (w + 1) - 1).
// D of v_mfma_f32_16x16x4_f32 (lane (g, j): outputs 4 g + r of row j) is a B operand of the next layer when step (t, r) sums the features {16 t + 4 g + r}, which only
// fixes how the next weight matrix is packed (d3il_amd/policies.py pack_ddpm_weights): [T_out][t][lane (g, i)][r] = W[16 T_out + i][16 t + 4 g + r].  So a layer is: every
// wave reads the 16 rows' 256 activations (16 float4 per lane) from LDS, runs DD_TPW x 64 MFMAs with its own share of the weights streamed from L2 (16 KB per tile,
// no sharing needed), applies bias / residual / Mish to its D registers and writes them to the other LDS buffer: one barrier per layer.
// The first layer (x | time embedding | state = 26 -> 28 inputs, 7 steps per tile) and the output layer (2 of 16 outputs; every wave computes it for the DDPM
// update of its copy of x) read their small packed matrices from L2.  The time embedding of step i is the same for every row (temb [T][8], evaluated once by the
// caller); the noise of all T + 1 draws comes as one tensor.
// Non-finite operands: the clip of the x0 prediction and the final clamp are fminf(fmaxf(..)), which return their bound for a NaN - a NaN observation would come out
// as a finite in-bounds action where the torch chain (torch.clamp) gives NaN.  So the row's state, its T + 1 noise draws and its final x are tested on their bit
// patterns (policy_nonfinite, policy_common.h) and a hit row gets 0x7FC00000 in both components by an integer select; the row's
// arithmetic still runs, rows are independent, no other row changes and finite rows come out bit for bit as without the test.
constexpr int DD_H = 256, DD_TILE_F4 = 16 * 64, DD_LAYER_F4 = 16 * DD_TILE_F4;      // float4 per packed output tile (16 KB), per packed layer
constexpr int DD_NW = 8, DD_TPW = 16 / DD_NW;      // waves per workgroup (16 rows), output tiles per wave: eight waves of two tiles - two waves per SIMD hide each other's weight loads
__device__ __forceinline__ float dd_mish(float x) {      // x tanh(softplus(x)), softplus with torch's threshold 20; tanh(log(1 + n)) = (n^2 + 2 n) / (n^2 + 2 n + 2), n = e^x
  if (x > 20.f) return x;
  const float n = expf(x), p = n * (n + 2.f);
  return x * (p / (p + 2.f));
}
// y[q] = (RES ? y[q] : 0) + bias + W m for the wave's four output tiles 4 w + q of one packed 256 x 256 layer (xin: the 16 rows' activations in LDS, B-operand order)
template <bool RES>
__device__ __forceinline__ void dd_layer4(const mlp_f4* __restrict__ wl, const float* __restrict__ bias, const mlp_f4* xin, mlp_f4* y, int w, int lane, int g) {
  mlp_f4 m[16], a[2][16];      // the weights of tile q + 1 are on their way from L2 while tile q is multiplied
  const mlp_f4* wt = wl + (long)(DD_TPW * w) * DD_TILE_F4 + lane;
#pragma unroll
  for (int t = 0; t < 16; t++) a[0][t] = wt[t * 64];
#pragma unroll
  for (int t = 0; t < 16; t++) m[t] = xin[t * 64 + lane];
#pragma unroll
  for (int q = 0; q < DD_TPW; q++) {
    const int To = DD_TPW * w + q;
    if (q + 1 < DD_TPW) {
#pragma unroll
      for (int t = 0; t < 16; t++) a[(q + 1) & 1][t] = wt[(q + 1) * DD_TILE_F4 + t * 64];
    }
    mlp_f4 acc[4];      // four accumulators: no MFMA waits for the one before it
    acc[0] = *(const mlp_f4*)(bias + 16 * To + 4 * g);
    acc[1] = RES ? y[q] : mlp_f4{0.f, 0.f, 0.f, 0.f};
    acc[2] = mlp_f4{0.f, 0.f, 0.f, 0.f}; acc[3] = mlp_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 16; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[q & 1][t][r], m[t][r], acc[r], 0, 0, 0);
    y[q] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
}
__global__ __launch_bounds__(64 * DD_NW) void k_ddpm_mlp_f32(const float* __restrict__ state, const float* __restrict__ noise, const float* __restrict__ temb, const float* __restrict__ w_in,
                                                       const float* __restrict__ b_in, const float* __restrict__ w_blk, const float* __restrict__ b_blk, const float* __restrict__ w_out,
                                                       const float* __restrict__ b_out, const float* __restrict__ sched, const float* __restrict__ bounds, float* __restrict__ out,
                                                       long n, int SD, int T, int nblk) {
  __shared__ mlp_f4 xb[2][DD_TILE_F4];      // the 16 rows' 256 activations, [t][lane] float4 = features 16 t + 4 g + r of row j: written by the layer that produces them, read by the next
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 15, g = lane >> 4;
  const long row = (long)blockIdx.x * 16 + j;
  const bool live = row < n;
  const long rr = live ? row : (n - 1);
  float st_k[7];      // the lane's share of the input row: feature 4 s + g of [x (2) | time embedding (8) | state (SD)]
#pragma unroll
  for (int s2 = 0; s2 < 7; s2++) { const int f = 4 * s2 + g; st_k[s2] = (f >= 10 && f < 10 + SD) ? state[rr * SD + f - 10] : 0.f; }
  const float lo0 = bounds[0], lo1 = bounds[1], hi0 = bounds[2], hi1 = bounds[3];
  float x0 = noise[rr * 2], x1 = noise[rr * 2 + 1];
  unsigned bad = (unsigned)policy_nonfinite(x0) | (unsigned)policy_nonfinite(x1);
#pragma unroll
  for (int s2 = 0; s2 < 7; s2++) bad |= (unsigned)policy_nonfinite(st_k[s2]);
  bad |= (unsigned)__shfl_xor((int)bad, 16); bad |= (unsigned)__shfl_xor((int)bad, 32);      // the four lane groups of row j hold its features 4 s + g
  const mlp_f4* w_in4 = (const mlp_f4*)w_in;
  const mlp_f4* w_out4 = (const mlp_f4*)w_out;
  int buf = 0;
#pragma clang loop unroll(disable)
  for (int step = 0; step < T; step++) {
    const int i = T - 1 - step;
    float in_k[7];
#pragma unroll
    for (int s2 = 0; s2 < 7; s2++) { const int f = 4 * s2 + g; in_k[s2] = f == 0 ? x0 : (f == 1 ? x1 : (f < 10 ? temb[i * 8 + f - 2] : st_k[s2])); }
    mlp_f4 xo[DD_TPW];      // the wave's tiles of the residual stream
#pragma unroll
    for (int q = 0; q < DD_TPW; q++) {
      const int To = DD_TPW * w + q;
      mlp_f4 acc = *(const mlp_f4*)(b_in + 16 * To + 4 * g);
      const mlp_f4 a0 = w_in4[(To * 64 + lane) * 2], a1 = w_in4[(To * 64 + lane) * 2 + 1];
#pragma unroll
      for (int s2 = 0; s2 < 7; s2++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(s2 < 4 ? a0[s2] : a1[s2 - 4], in_k[s2], acc, 0, 0, 0);
      xo[q] = acc;
    }
#pragma clang loop unroll(disable)
    for (int b = 0; b < nblk; b++) {      // x + l2(mish(l1(mish(x))))
      mlp_f4 y[DD_TPW];
#pragma unroll
      for (int q = 0; q < DD_TPW; q++) xb[buf][(DD_TPW * w + q) * 64 + lane] = mlp_f4{dd_mish(xo[q][0]), dd_mish(xo[q][1]), dd_mish(xo[q][2]), dd_mish(xo[q][3])};
      __syncthreads();
      dd_layer4<false>((const mlp_f4*)w_blk + (long)(2 * b) * DD_LAYER_F4, b_blk + (2 * b) * DD_H, xb[buf], y, w, lane, g);
      buf ^= 1;
#pragma unroll
      for (int q = 0; q < DD_TPW; q++) xb[buf][(DD_TPW * w + q) * 64 + lane] = mlp_f4{dd_mish(y[q][0]), dd_mish(y[q][1]), dd_mish(y[q][2]), dd_mish(y[q][3])};
      __syncthreads();
      dd_layer4<true>((const mlp_f4*)w_blk + (long)(2 * b + 1) * DD_LAYER_F4, b_blk + (2 * b + 1) * DD_H, xb[buf], xo, w, lane, g);      // the residual rides in the accumulator
      buf ^= 1;
    }
#pragma unroll
    for (int q = 0; q < DD_TPW; q++) xb[buf][(DD_TPW * w + q) * 64 + lane] = xo[q];
    __syncthreads();
    mlp_f4 acc = mlp_f4{0.f, 0.f, 0.f, 0.f}, acc2 = mlp_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const mlp_f4 a4 = w_out4[t * 64 + lane], m4 = xb[buf][t * 64 + lane];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0], m4[0], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1], m4[1], acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[2], m4[2], acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[3], m4[3], acc2, 0, 0, 0);
    }
    buf ^= 1;
    acc += acc2;
    // epsilon of row j sits in lane (0, j), registers 0 and 1: every lane group of every wave takes it and does the same update on its copy of x
    const float e0 = __shfl(acc[0], j) + b_out[0], e1 = __shfl(acc[1], j) + b_out[1];
    const float sra = sched[i * 5], srm1 = sched[i * 5 + 1], c1 = sched[i * 5 + 2], c2 = sched[i * 5 + 3], sig = sched[i * 5 + 4];
    const float p0 = fminf(fmaxf(sra * x0 - srm1 * e0, lo0), hi0), p1 = fminf(fmaxf(sra * x1 - srm1 * e1, lo1), hi1);      // clipped x0 prediction
    const float z0 = noise[((long)(step + 1) * n + rr) * 2], z1 = noise[((long)(step + 1) * n + rr) * 2 + 1];
    bad |= (unsigned)policy_nonfinite(z0) | (unsigned)policy_nonfinite(z1);
    x0 = (c1 * p0 + c2 * x0) + sig * z0;
    x1 = (c1 * p1 + c2 * x1) + sig * z1;
  }
  if (live && w == 0 && g == 0) {
    bad |= (unsigned)policy_nonfinite(x0) | (unsigned)policy_nonfinite(x1);
    const unsigned y0 = __float_as_uint(fminf(fmaxf(x0, lo0), hi0)), y1 = __float_as_uint(fminf(fmaxf(x1, lo1), hi1));
    ((unsigned*)out)[row * 2] = bad ? 0x7FC00000u : y0;
    ((unsigned*)out)[row * 2 + 1] = bad ? 0x7FC00000u : y1;
  }
}
__global__ __launch_bounds__(256) void k_layernorm_f32(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ y,
                                                       long rows, int C, float eps) {
  const long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 5;
  const int sub = threadIdx.x & 31;
  const bool live = row < rows && 4 * sub < C;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) v = reinterpret_cast<const float4*>(x + row * C)[sub];
  float s = v.x + v.y + v.z + v.w;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  const float mean = s / (float)C;
  const float dx = live ? v.x - mean : 0.f, dy = live ? v.y - mean : 0.f, dz = live ? v.z - mean : 0.f, dw = live ? v.w - mean : 0.f;
  float q = dx * dx + dy * dy + dz * dz + dw * dw;
#pragma unroll
  for (int m = 16; m >= 1; m >>= 1) q += __shfl_xor(q, m);
  const float inv = rsqrtf(q / (float)C + eps);
  if (live) {
    const float4 ww = reinterpret_cast<const float4*>(w)[sub], bb = reinterpret_cast<const float4*>(b)[sub];
    reinterpret_cast<float4*>(y + row * C)[sub] = make_float4(dx * inv * ww.x + bb.x, dy * inv * ww.y + bb.y, dz * inv * ww.z + bb.z, dw * inv * ww.w + bb.w);
  }
}

template <int D4>      // D4 = D / 4 float4 chunks per head row (D a multiple of 4: 16-byte loads), or 0: scalar loads for any D <= 32
__global__ __launch_bounds__(256) void k_attention_causal_f32(const float* __restrict__ qkv, float* __restrict__ out, int B, int T, int H, int D) {
  // One lane serves TWO queries of a (sequence, head): i and T - 1 - i.  Query i attends to i + 1 keys, so the pair costs T + 1 key steps whatever i is:
  // the lanes of a wave run the same number of steps (one query per lane leaves half of the lane-steps idle under the causal mask).
  const int TP = (T + 1) / 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;     // ((b * H) + h) * TP + p: the query pairs of one (b, h) sit in adjacent lanes
  const long total = (long)B * H * TP;
  if (idx >= total) return;
  const int p = (int)(idx % TP), h = (int)((idx / TP) % H);
  const long b = idx / ((long)TP * H);
  const int C = H * D;
  const float* base = qkv + (b * T) * (long)(3 * C) + h * D;
  constexpr int DR = D4 > 0 ? 4 * D4 : 32;
  const float scale = 1.0f / sqrtf((float)D);
  auto load = [&](const float* ptr, float* r) {
    if constexpr (D4 > 0) {
#pragma unroll
      for (int c = 0; c < D4; c++) { const float4 t = reinterpret_cast<const float4*>(ptr)[c]; r[4 * c] = t.x; r[4 * c + 1] = t.y; r[4 * c + 2] = t.z; r[4 * c + 3] = t.w; }
    } else {
#pragma unroll
      for (int d = 0; d < 32; d++) r[d] = d < D ? ptr[d] : 0.0f;
    }
  };
  for (int half = 0; half < 2; half++) {
    const int i = half == 0 ? p : T - 1 - p;
    if (half == 1 && i == p) break;      // the middle query of an odd T
    float q[DR], acc[DR], kk[DR], vv[DR];
    load(base + (long)i * 3 * C, q);
#pragma unroll
    for (int d = 0; d < DR; d++) q[d] *= scale;
    // online softmax; key 0 is peeled (m = score_0, l = 1, acc = v_0) so that no infinity is ever formed: the device pass is built
    // with -ffinite-math-only, under which arithmetic on infinities is undefined
    load(base + C, kk); load(base + 2 * C, acc);
    float m = 0.0f, l = 1.0f;
#pragma unroll
    for (int d = 0; d < DR; d++) m += q[d] * kk[d];
    for (int j = 1; j <= i; j++) {
      const float* kj = base + (long)j * 3 * C + C;
      load(kj, kk); load(kj + C, vv);
      float sc = 0.0f;
#pragma unroll
      for (int d = 0; d < DR; d++) sc += q[d] * kk[d];
      const float mn = fmaxf(m, sc), corr = __expf(m - mn), pj = __expf(sc - mn);
      l = l * corr + pj;
#pragma unroll
      for (int d = 0; d < DR; d++) acc[d] = acc[d] * corr + pj * vv[d];
      m = mn;
    }
    float* o = out + (b * T + i) * (long)C + h * D;
    const float inv = 1.0f / l;
    if constexpr (D4 > 0) {
#pragma unroll
      for (int c = 0; c < D4; c++) reinterpret_cast<float4*>(o)[c] = make_float4(acc[4 * c] * inv, acc[4 * c + 1] * inv, acc[4 * c + 2] * inv, acc[4 * c + 3] * inv);
    } else {
#pragma unroll
      for (int d = 0; d < 32; d++) if (d < D) o[d] = acc[d] * inv;
    }
  }
  // A NaN / Inf score of a later key makes l NaN by itself (exp of NaN, of Inf - Inf).  Query 0 has one key and never exponentiates its score: a non-finite
  // score 0 hands out v_0 above, where the masked softmax of that single score is NaN.  Its lane (pair 0) forms that score once more, tests the bits and
  // writes NaN over the row - behind the loop and apart from it, so that the arithmetic above compiles as it did (the f32 sums of finite rows keep their bits)
  if (p == 0) {
    float s0 = 0.0f;
    for (int d = 0; d < D; d++) s0 += (base[d] * scale) * base[C + d];
    if (policy_nonfinite(s0)) {
      float* o = out + (b * T) * (long)C + h * D;      // (float stores, as the ones above: stores of another type could be ordered before them)
      const float qnan = __uint_as_float(0x7FC00000u);
      for (int d = 0; d < D; d++) o[d] = qnan;
    }
  }
}

}  // namespace d3il
