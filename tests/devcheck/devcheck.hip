// devcheck.hip - TEST-ONLY device build of leaf math of the kernels (d3il_amd/csrc/panda_step.h), one problem per lane.
// Lets the GPU suite (tests/test_gpu_ik_solve6.py) call ik_solve6, rcpd / rsqrtd, trig_advance and ik_update by themselves, compiled with the product's
// flags (d3il_amd.build.HIPCC_FLAGS), against the references of tests/ik_solve6_cases.py.  It is NOT part of the product: d3il_amd/ never loads it and
// libd3il_rollout.so does not contain it.  Laid out so that other leaf routines (the contact solvers) can follow: one kernel + one dc_ entry per routine.
//
// Conventions: arrays are problem-major ([n][21], [n][6], ...; sequences [T][n][..]); every entry takes device pointers and the caller's stream, launches
// ceil(n / 64) workgroups of one wave, and returns 0, DC_EINVAL (n <= 0 or a required pointer NULL: nothing is launched) or the HIP error of the launch.
#include <hip/hip_runtime.h>
#include "../../d3il_amd/csrc/panda_step.h"
#include "../../d3il_amd/csrc/gen/avoiding_consts.inc"

using namespace d3il;

namespace {
constexpr int LANES = 64;
constexpr int DC_EINVAL = -1;

template <bool FAST, bool WARM>
__global__ __launch_bounds__(LANES) void k_solve6(const double* __restrict__ A, const double* __restrict__ b, double lo, double hi, double* __restrict__ x,
                                                  double* __restrict__ vwarm, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  double a[21], r[6], o[6], vw[7];
#pragma unroll
  for (int i = 0; i < 21; i++) a[i] = A[(size_t)e * 21 + i];
#pragma unroll
  for (int i = 0; i < 6; i++) r[i] = b[(size_t)e * 6 + i];
  if (WARM) {
#pragma unroll
    for (int i = 0; i < 7; i++) vw[i] = vwarm[(size_t)e * 7 + i];
  }
  ik_solve6<FAST>(a, r, lo, hi, o, WARM ? vw : nullptr);
#pragma unroll
  for (int i = 0; i < 6; i++) x[(size_t)e * 6 + i] = o[i];
  if (WARM) {
#pragma unroll
    for (int i = 0; i < 7; i++) vwarm[(size_t)e * 7 + i] = vw[i];
  }
}

// T solves per lane in sequence, the vector carried in registers from one to the next as the step kernels carry it (cold before the first).
// mark: a valid vector enters every solve with [6] = 2.0 instead of 1.0 (as valid: any non-zero), so that sent[t][e] = [6] after solve t tells the path:
// 2.0 path 1 (vector untouched), 1.0 deflation accepted, 0.0 Jacobi (or path 1 without a vector).
template <bool FAST>
__global__ __launch_bounds__(LANES) void k_solve6_chain(const double* __restrict__ A, const double* __restrict__ b, double lo, double hi, double* __restrict__ x,
                                                        double* __restrict__ sent, int mark, int T, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  double vw[7];
#pragma unroll
  for (int i = 0; i < 7; i++) vw[i] = 0.0;
#pragma clang loop unroll(disable)
  for (int t = 0; t < T; t++) {
    const size_t p = (size_t)t * n + e;
    double a[21], r[6], o[6];
#pragma unroll
    for (int i = 0; i < 21; i++) a[i] = A[p * 21 + i];
#pragma unroll
    for (int i = 0; i < 6; i++) r[i] = b[p * 6 + i];
    if (mark && vw[6] != 0.0) vw[6] = 2.0;
    ik_solve6<FAST>(a, r, lo, hi, o, vw);
#pragma unroll
    for (int i = 0; i < 6; i++) x[p * 6 + i] = o[i];
    sent[p] = vw[6];
  }
}

__global__ __launch_bounds__(LANES) void k_scalar(const double* __restrict__ in, double* __restrict__ rcp, double* __restrict__ rsq, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  const double v = in[e];
  rcp[e] = rcpd(v);
  rsq[e] = v > 0.0 ? rsqrtd(v) : 0.0;
}

__global__ __launch_bounds__(LANES) void k_trig_chain(const double* __restrict__ dl, double* __restrict__ sn, double* __restrict__ cs, int K, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  double s = sn[e], c = cs[e];
#pragma clang loop unroll(disable)
  for (int k = 0; k < K; k++) trig_advance(dl[(size_t)k * n + e], s, c);
  sn[e] = s; cs[e] = c;
}

// len[e] controller calls of lane e on the Avoiding constants: des [K][n][7] = position + UNIT quaternion, jpos / jvel [K][n][7]; out ikq / tau [K][n][7].
// VW / TR: pass vwarm / trig as the kernels do; period > 0: both start afresh every `period` calls (one launch of the step kernel).
template <bool FAST, bool VW, bool TR>
__global__ __launch_bounds__(LANES) void k_ik_update(const double* __restrict__ des, const double* __restrict__ jpos, const double* __restrict__ jvel,
                                                     const int* __restrict__ len, double* __restrict__ ikq_out, double* __restrict__ tau_out, int period, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  const PandaConsts& c = kAvoidingConsts;
  double ikq[NARM], ikqd[NARM], vw[7], trig[2 * NARM + 1];
#pragma unroll
  for (int i = 0; i < NARM; i++) { ikq[i] = 0.0; ikqd[i] = 0.0; }
#pragma unroll
  for (int i = 0; i < 7; i++) vw[i] = 0.0;
#pragma unroll
  for (int i = 0; i <= 2 * NARM; i++) trig[i] = 0.0;
  unsigned fl = 0;
  const int K = len[e];
#pragma clang loop unroll(disable)
  for (int k = 0; k < K; k++) {
    const size_t p = ((size_t)k * n + e) * 7;
    double d[7], q0[NARM], v0[NARM];
#pragma unroll
    for (int i = 0; i < 7; i++) { d[i] = des[p + i]; q0[i] = jpos[p + i]; v0[i] = jvel[p + i]; }
    if (period > 0 && k % period == 0) { vw[6] = 0.0; trig[2 * NARM] = 0.0; }
    ik_update<FAST>(c, d, d + 3, q0, fl, ikq, ikqd, VW ? vw : nullptr, TR ? trig : nullptr);
#pragma unroll
    for (int i = 0; i < NARM; i++) { ikq_out[p + i] = ikq[i]; tau_out[p + i] = c.pd_p[i] * (ikq[i] - q0[i]) + c.pd_d[i] * (ikqd[i] - v0[i]); }
  }
}

int launched() { return (int)hipGetLastError(); }
dim3 grid(int n) { return dim3((unsigned)((n + LANES - 1) / LANES)); }
}  // namespace

extern "C" {
int dc_lanes() { return LANES; }

int dc_solve6(const double* A, const double* b, double lo, double hi, double* x, double* vwarm, int fast, int n, void* stream) {
  if (n <= 0 || !A || !b || !x) return DC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (vwarm) {
    if (fast) hipLaunchKernelGGL((k_solve6<true, true>), grid(n), dim3(LANES), 0, s, A, b, lo, hi, x, vwarm, n);
    else hipLaunchKernelGGL((k_solve6<false, true>), grid(n), dim3(LANES), 0, s, A, b, lo, hi, x, vwarm, n);
  } else {
    if (fast) hipLaunchKernelGGL((k_solve6<true, false>), grid(n), dim3(LANES), 0, s, A, b, lo, hi, x, vwarm, n);
    else hipLaunchKernelGGL((k_solve6<false, false>), grid(n), dim3(LANES), 0, s, A, b, lo, hi, x, vwarm, n);
  }
  return launched();
}

int dc_solve6_chain(const double* A, const double* b, double lo, double hi, double* x, double* sent, int fast, int mark, int T, int n, void* stream) {
  if (n <= 0 || T <= 0 || !A || !b || !x || !sent) return DC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (fast) hipLaunchKernelGGL((k_solve6_chain<true>), grid(n), dim3(LANES), 0, s, A, b, lo, hi, x, sent, mark, T, n);
  else hipLaunchKernelGGL((k_solve6_chain<false>), grid(n), dim3(LANES), 0, s, A, b, lo, hi, x, sent, mark, T, n);
  return launched();
}

int dc_scalar(const double* in, double* rcp, double* rsq, int n, void* stream) {
  if (n <= 0 || !in || !rcp || !rsq) return DC_EINVAL;
  hipLaunchKernelGGL(k_scalar, grid(n), dim3(LANES), 0, (hipStream_t)stream, in, rcp, rsq, n);
  return launched();
}

int dc_trig_chain(const double* dl, double* sn, double* cs, int K, int n, void* stream) {
  if (n <= 0 || K <= 0 || !dl || !sn || !cs) return DC_EINVAL;
  hipLaunchKernelGGL(k_trig_chain, grid(n), dim3(LANES), 0, (hipStream_t)stream, dl, sn, cs, K, n);
  return launched();
}

int dc_ik_update(const double* des, const double* jpos, const double* jvel, const int* len, double* ikq_out, double* tau_out, int use_vwarm, int use_trig, int period,
                 int fast, int n, void* stream) {
  if (n <= 0 || period < 0 || !des || !jpos || !jvel || !len || !ikq_out || !tau_out) return DC_EINVAL;
  if (!fast && (use_vwarm || use_trig)) return DC_EINVAL;      // FAST = false is built in the plain calling form only
  hipStream_t s = (hipStream_t)stream;
#define DC_IK(F, V, T) hipLaunchKernelGGL((k_ik_update<F, V, T>), grid(n), dim3(LANES), 0, s, des, jpos, jvel, len, ikq_out, tau_out, period, n)
  if (!fast) DC_IK(false, false, false);
  else if (use_vwarm && use_trig) DC_IK(true, true, true);
  else if (use_vwarm) DC_IK(true, true, false);
  else if (use_trig) DC_IK(true, false, true);
  else DC_IK(true, false, false);
#undef DC_IK
  return launched();
}
}
