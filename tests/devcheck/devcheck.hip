// devcheck.hip - TEST-ONLY device build of leaf math of the kernels (d3il_amd/csrc/panda_step.h, rigid_common.h, gen_tree.h), one problem per lane.
// Lets the GPU suite (tests/test_gpu_ik_solve6.py) call ik_solve6, rcpd / rsqrtd, trig_advance and ik_update by themselves, compiled with the product's
// flags (d3il_amd.build.HIPCC_FLAGS), against the references of tests/ik_solve6_cases.py; and (tests/test_gpu_contact_leaf.py) the leaf routines of the contact
// engines - box_box_emit, cyl_box, cone_eval / gt_cone_eval, ldl_n / gt_ldl_n with their solves, cube_integrate, push_tan_yaw, quat2mat - against the
// references of tests/contact_leaf_cases.py.  gen_step.h is included whole, as tests/hostcheck/hostcheck.cpp includes it (gen_tree.h cannot stand without its
// slot constants); that brings the generic engine's __constant__ block into this library, unused and colliding with nothing.  It is NOT part of the product: d3il_amd/ never loads it and
// libd3il_rollout.so does not contain it.  Laid out so that other leaf routines (the contact solvers) can follow: one kernel + one dc_ entry per routine.
//
// Conventions: arrays are problem-major ([n][21], [n][6], ...; sequences [T][n][..]); every entry takes device pointers and the caller's stream, launches
// ceil(n / 64) workgroups of one wave, and returns 0, DC_EINVAL (n <= 0 or a required pointer NULL: nothing is launched) or the HIP error of the launch.
#include <hip/hip_runtime.h>
#include "../../d3il_amd/csrc/gen_step.h"
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

// ---------------------------------------------------------------- leaf routines of the contact engines (rigid_common.h, gen_tree.h)
// box_box_emit with a callback that writes the lane's own rows, as gen_phase2 / gen_phase3 do: rec [n][8][7] = dist, pos3, normal3 (the caller pre-fills it with
// NaN: rows >= count[e] stay untouched), count [n].  R row-major.  Either geom order is the caller's choice of which box comes first.
__global__ __launch_bounds__(LANES) void k_box_box(const double* __restrict__ p1, const double* __restrict__ R1, const double* __restrict__ s1,
                                                   const double* __restrict__ p2, const double* __restrict__ R2, const double* __restrict__ s2,
                                                   const double* __restrict__ margin, int cap, int* __restrict__ count, double* __restrict__ rec, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  double a[3], b[3], sa[3], sb[3], Ra[9], Rb[9];
#pragma unroll
  for (int k = 0; k < 3; k++) { a[k] = p1[(size_t)e * 3 + k]; b[k] = p2[(size_t)e * 3 + k]; sa[k] = s1[(size_t)e * 3 + k]; sb[k] = s2[(size_t)e * 3 + k]; }
#pragma unroll
  for (int k = 0; k < 9; k++) { Ra[k] = R1[(size_t)e * 9 + k]; Rb[k] = R2[(size_t)e * 9 + k]; }
  double* row = rec + (size_t)e * 56;
  int cnt = 0;
  const int lim = cap < 8 ? (cap < 0 ? 0 : cap) : 8;      // the rows of a lane end at 8 whatever the caller asks for
  box_box_emit(a, Ra, sa, b, Rb, sb, margin[e], lim, [&](double dist, const double* pos, const double* nrm) {
    if (cnt < 8) {
      double* r = row + 7 * cnt;
      r[0] = dist; r[1] = pos[0]; r[2] = pos[1]; r[3] = pos[2]; r[4] = nrm[0]; r[5] = nrm[1]; r[6] = nrm[2];
    }
    cnt++;
  });
  count[e] = cnt;
}

// out [n][7] (pre-filled with NaN by the caller, written on a hit only), hit [n]; par [n][3] = rad, half, margin
__global__ __launch_bounds__(LANES) void k_cyl_box(const double* __restrict__ pc, const double* __restrict__ axis, const double* __restrict__ par,
                                                   const double* __restrict__ pb, const double* __restrict__ Rb, const double* __restrict__ sb,
                                                   int* __restrict__ hit, double* __restrict__ out, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  double c[3], u[3], b[3], s[3], R[9], o[7];
#pragma unroll
  for (int k = 0; k < 3; k++) { c[k] = pc[(size_t)e * 3 + k]; u[k] = axis[(size_t)e * 3 + k]; b[k] = pb[(size_t)e * 3 + k]; s[k] = sb[(size_t)e * 3 + k]; }
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = Rb[(size_t)e * 9 + k];
  const bool h = cyl_box(c, u, par[(size_t)e * 3], par[(size_t)e * 3 + 1], b, R, s, par[(size_t)e * 3 + 2], o);
  hit[e] = h ? 1 : 0;
  if (h) {
#pragma unroll
    for (int k = 0; k < 7; k++) out[(size_t)e * 7 + k] = o[k];
  }
}

// both twins in one launch: par [n][4] = Dn, Dt, mu, fric; out [n][2][13] = cost, force3, Hc9 of cone_eval ([0]) and gt_cone_eval ([1])
__global__ __launch_bounds__(LANES) void k_cone_eval(const double* __restrict__ jar, const double* __restrict__ par, double* __restrict__ out, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  const double j[3] = {jar[(size_t)e * 3], jar[(size_t)e * 3 + 1], jar[(size_t)e * 3 + 2]};
  const double Dn = par[(size_t)e * 4], Dt = par[(size_t)e * 4 + 1], mu = par[(size_t)e * 4 + 2], fric = par[(size_t)e * 4 + 3];
  double f[3], H[9];
  double* o = out + (size_t)e * 26;
  o[0] = cone_eval(j, Dn, Dt, mu, fric, f, H);
#pragma unroll
  for (int k = 0; k < 3; k++) o[1 + k] = f[k];
#pragma unroll
  for (int k = 0; k < 9; k++) o[4 + k] = H[k];
  o[13] = gt_cone_eval(j, Dn, Dt, mu, fric, f, H);
#pragma unroll
  for (int k = 0; k < 3; k++) o[14 + k] = f[k];
#pragma unroll
  for (int k = 0; k < 9; k++) o[17 + k] = H[k];
}

// A [n][N (N + 1) / 2] packed lower triangle, b [n][N] -> L (same packing: diagonal as given, strict lower part = L), d, x [n][N], ok [n]
template <int N, bool TWIN>
__global__ __launch_bounds__(LANES) void k_ldl(const double* __restrict__ A, const double* __restrict__ b, double* __restrict__ L, double* __restrict__ d,
                                               double* __restrict__ x, int* __restrict__ ok, int n) {
  constexpr int P = N * (N + 1) / 2;
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  double a[P], dd[N], id[N], r[N];
#pragma unroll
  for (int i = 0; i < P; i++) a[i] = A[(size_t)e * P + i];
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = b[(size_t)e * N + i];
  bool good;
  if (TWIN) { good = gt_ldl_n<N>(a, dd, id); gt_ldl_solve_n<N>(a, id, r); }
  else { good = ldl_n<N>(a, dd, id); ldl_solve_n<N>(a, id, r); }
#pragma unroll
  for (int i = 0; i < P; i++) L[(size_t)e * P + i] = a[i];
#pragma unroll
  for (int i = 0; i < N; i++) { d[(size_t)e * N + i] = dd[i]; x[(size_t)e * N + i] = r[i]; }
  ok[e] = good ? 1 : 0;
}

// K calls of cube_integrate per lane, the state (pos3 quat4 vel6) carried in registers; state [n][13] in/out, acc [n][6], h [n];
// qhist (may be NULL) [K][n][4]: the quaternion after every call
__global__ __launch_bounds__(LANES) void k_cube_chain(double* __restrict__ state, const double* __restrict__ acc, const double* __restrict__ h, int K,
                                                      double* __restrict__ qhist, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  BoxState bx; double a[6];
#pragma unroll
  for (int k = 0; k < 3; k++) bx.pos[k] = state[(size_t)e * 13 + k];
#pragma unroll
  for (int k = 0; k < 4; k++) bx.quat[k] = state[(size_t)e * 13 + 3 + k];
#pragma unroll
  for (int k = 0; k < 6; k++) { bx.vel[k] = state[(size_t)e * 13 + 7 + k]; a[k] = acc[(size_t)e * 6 + k]; }
  const double hh = h[e];
#pragma clang loop unroll(disable)
  for (int c = 0; c < K; c++) {
    cube_integrate(bx, a, hh);
    if (qhist) {
#pragma unroll
      for (int k = 0; k < 4; k++) qhist[((size_t)c * n + e) * 4 + k] = bx.quat[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) state[(size_t)e * 13 + k] = bx.pos[k];
#pragma unroll
  for (int k = 0; k < 4; k++) state[(size_t)e * 13 + 3 + k] = bx.quat[k];
#pragma unroll
  for (int k = 0; k < 6; k++) state[(size_t)e * 13 + 7 + k] = bx.vel[k];
}

__global__ __launch_bounds__(LANES) void k_tan_yaw(const double* __restrict__ q, double* __restrict__ out, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  const double v[4] = {q[(size_t)e * 4], q[(size_t)e * 4 + 1], q[(size_t)e * 4 + 2], q[(size_t)e * 4 + 3]};
  out[e] = push_tan_yaw(v);
}

__global__ __launch_bounds__(LANES) void k_quat2mat(const double* __restrict__ q, double* __restrict__ R, int n) {
  const int e = blockIdx.x * LANES + threadIdx.x;
  if (e >= n) return;
  const double v[4] = {q[(size_t)e * 4], q[(size_t)e * 4 + 1], q[(size_t)e * 4 + 2], q[(size_t)e * 4 + 3]};
  double r[9];
  quat2mat(v, r);
#pragma unroll
  for (int k = 0; k < 9; k++) R[(size_t)e * 9 + k] = r[k];
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

int dc_box_box(const double* p1, const double* R1, const double* s1, const double* p2, const double* R2, const double* s2, const double* margin, int cap,
               int* count, double* rec, int n, void* stream) {
  if (n <= 0 || !p1 || !R1 || !s1 || !p2 || !R2 || !s2 || !margin || !count || !rec) return DC_EINVAL;
  hipLaunchKernelGGL(k_box_box, grid(n), dim3(LANES), 0, (hipStream_t)stream, p1, R1, s1, p2, R2, s2, margin, cap, count, rec, n);
  return launched();
}

int dc_cyl_box(const double* pc, const double* axis, const double* par, const double* pb, const double* Rb, const double* sb, int* hit, double* out, int n, void* stream) {
  if (n <= 0 || !pc || !axis || !par || !pb || !Rb || !sb || !hit || !out) return DC_EINVAL;
  hipLaunchKernelGGL(k_cyl_box, grid(n), dim3(LANES), 0, (hipStream_t)stream, pc, axis, par, pb, Rb, sb, hit, out, n);
  return launched();
}

int dc_cone_eval(const double* jar, const double* par, double* out, int n, void* stream) {
  if (n <= 0 || !jar || !par || !out) return DC_EINVAL;
  hipLaunchKernelGGL(k_cone_eval, grid(n), dim3(LANES), 0, (hipStream_t)stream, jar, par, out, n);
  return launched();
}

// order 5 or 6; twin: gt_ldl_n / gt_ldl_solve_n (the product instantiates ldl_n<5> and gt_ldl_n<6>; the other two are here for the twin comparison)
int dc_ldl(int order, int twin, const double* A, const double* b, double* L, double* d, double* x, int* ok, int n, void* stream) {
  if (n <= 0 || (order != 5 && order != 6) || !A || !b || !L || !d || !x || !ok) return DC_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (order == 5 && !twin) hipLaunchKernelGGL((k_ldl<5, false>), grid(n), dim3(LANES), 0, s, A, b, L, d, x, ok, n);
  else if (order == 5) hipLaunchKernelGGL((k_ldl<5, true>), grid(n), dim3(LANES), 0, s, A, b, L, d, x, ok, n);
  else if (!twin) hipLaunchKernelGGL((k_ldl<6, false>), grid(n), dim3(LANES), 0, s, A, b, L, d, x, ok, n);
  else hipLaunchKernelGGL((k_ldl<6, true>), grid(n), dim3(LANES), 0, s, A, b, L, d, x, ok, n);
  return launched();
}

int dc_cube_chain(double* state, const double* acc, const double* h, int K, double* qhist, int n, void* stream) {
  if (n <= 0 || K <= 0 || !state || !acc || !h) return DC_EINVAL;
  hipLaunchKernelGGL(k_cube_chain, grid(n), dim3(LANES), 0, (hipStream_t)stream, state, acc, h, K, qhist, n);
  return launched();
}

int dc_tan_yaw(const double* q, double* out, int n, void* stream) {
  if (n <= 0 || !q || !out) return DC_EINVAL;
  hipLaunchKernelGGL(k_tan_yaw, grid(n), dim3(LANES), 0, (hipStream_t)stream, q, out, n);
  return launched();
}

int dc_quat2mat(const double* q, double* R, int n, void* stream) {
  if (n <= 0 || !q || !R) return DC_EINVAL;
  hipLaunchKernelGGL(k_quat2mat, grid(n), dim3(LANES), 0, (hipStream_t)stream, q, R, n);
  return launched();
}
}
