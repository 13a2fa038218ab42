// link_guard.h - the link-near guard of the generic engine (Pushing, Sorting, Inserting; included by rollout.hip).
//
// The generic engine collides ONE part of the robot with the scene: the rod.  The model gives every Panda link a collision hull
// (link0 .. link7, hand, both fingers with their tip boxes) that MuJoCo collides with the cubes, the walls, the platform and the
// table; those pairs are absent here.  The guard does not add them - it says when one of them WOULD matter:
// once per env step, after the physics, bounding capsules of the hulls are tested against the environment's cubes and static
// boxes, and D3IL_PFLAG_LINK_NEAR (sticky for the episode, cleared by the resets like the other per-episode bits) is raised when
// a pair is closer than `margin`.  The physics is not touched; the step kernels are not edited.
//
// Pairs:  every capsule x every cube;  the capsules marked `statics` (the distal bodies: link5, link6, link7, hand, both
// fingers) x every static box (all ns, frame beams included).  LEFT OUT ON PURPOSE: the proximal links (link0 .. link4) x static
// boxes - they sit at the mount with cm-scale clearance to the table and the frame in every configuration, a 2 cm guard there
// would fire constantly and say nothing.
//
// Sampling: the test runs at env-step boundaries (every n_substeps physics sub-steps).  An approach shorter than one env step can
// be missed; a contact that persists - the kind that changes an outcome - cannot.
//
// Distance capsule <-> box = distance(segment, oriented box) - r.  In the box frame the squared distance g(t) from the segment
// point a + t d to the box is convex in t, so the sign of g'(t) = 2 e(t) . d (e = the point minus its clamp into the box)
// brackets a minimiser: LG_BISECT = 12 halvings leave an interval of |d| / 4096, and because the distance is 1-Lipschitz in the
// point, f(mid) - |d| / 8192 is a LOWER BOUND of the true distance (no false negatives) that lies at most
//     LG_MAXLEN / 8192 = 1.22e-4 m  <=  LG_SLACK = 1.25e-4 m
// below it (segments longer than LG_MAXLEN = 1 m are refused by d3il_set_link_guard; the Panda capsules are < 0.2 m: 2.5e-5 m).
// In front of it a bounding-sphere cull: distance(segment mid point, box) - |d| / 2 is a lower bound too; beyond r + margin the
// pair is skipped.
//
// One environment is worked on by LG_LPE = 4 neighbouring lanes (16 environments per wave, 4096 environments = one wave per CU):
// each lane runs the forward kinematics of the body chain (qpos rows 0 .. 8; the chain constants are the arm dynamics' own,
// PandaConsts::P / Q / f_axis), puts the world end points of ITS capsules (every fourth) and its share of the cubes' frames into
// LDS, then tests its capsules against all boxes - the box index is uniform over the wave, so the static boxes come in by scalar
// loads.  No scratch, no atomics except the episode counter.  The host build (tests/hostcheck) runs the same functions with one
// "lane" per environment.
#pragma once
#include "gen_step.h"

namespace d3il {

constexpr int LG_MAXCAP = 16;              // capsules per handle
constexpr int LG_BISECT = 12;
constexpr double LG_MAXLEN = 1.0;          // longest capsule segment accepted
constexpr double LG_SLACK = 1.25e-4;         // how far the distance used may lie below the true one (tests, d3il_rollout.h)
static_assert(LG_MAXLEN / (double)(2 << LG_BISECT) <= LG_SLACK, "the bisection's interval bounds the slack");
constexpr int LG_LPE = 4;                  // lanes per environment (device)
constexpr int LG_ENVS = GEN_WAVE / LG_LPE; // environments per workgroup (one wave)
constexpr int LG_CAPW = 7;                 // LDS words per capsule: world p0, p1, r
constexpr int LG_BOXW = 12;                // per cube: centre, world <- cube rotation
constexpr int LG_WORK = LG_MAXCAP * LG_CAPW + GEN_MAXNB * LG_BOXW;
constexpr unsigned LG_FLAG = 1u << 20;     // D3IL_PFLAG_LINK_NEAR

struct LinkGuardConsts {
  int n, pad;
  double margin;
  int link[LG_MAXCAP];       // 0: fixed to the world (link0);  k = 1 .. 7: the frame behind arm joint k
  int finger[LG_MAXCAP];     // -1, or the finger slide (0 / 1) that carries the capsule (link == 7)
  int statics[LG_MAXCAP];    // 1: also tested against the static boxes
  double p0[LG_MAXCAP][3], p1[LG_MAXCAP][3], r[LG_MAXCAP];   // in the frame of `link` (fingers: at slide position 0)
};

// true when the lower bound of distance(segment a b, box) described above is below `reach`; lb (optional) = that bound (of the cull when the cull decided)
template <class TC, class TR, class TH>
D3IL_HD bool lg_seg_box_near(const double* a, const double* b, TC c, TR R, TH h, double reach, double* lb) {
  double A[3], d[3], M[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double xa = (a[0] - c[0]) * R[i] + (a[1] - c[1]) * R[3 + i] + (a[2] - c[2]) * R[6 + i];
    const double xb = (b[0] - c[0]) * R[i] + (b[1] - c[1]) * R[3 + i] + (b[2] - c[2]) * R[6 + i];
    A[i] = xa; d[i] = xb - xa; M[i] = 0.5 * (xa + xb);
  }
  const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  double g = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) { const double e = fabs(M[i]) - h[i]; if (e > 0) g += e * e; }
  const double cull = sqrt(g) - 0.5 * len;
  if (cull >= reach) { if (lb) *lb = cull; return false; }
  double lo = 0.0, hi = 1.0;
#pragma unroll
  for (int it = 0; it < LG_BISECT; it++) {
    const double t = 0.5 * (lo + hi);
    double s = 0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double x = A[i] + t * d[i];
      const double e = x > h[i] ? x - h[i] : (x < -h[i] ? x + h[i] : 0.0);
      s += e * d[i];
    }
    if (s > 0) hi = t; else lo = t;
  }
  const double t = 0.5 * (lo + hi);
  g = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) { const double e = fabs(A[i] + t * d[i]) - h[i]; if (e > 0) g += e * e; }
  const double bound = sqrt(g) - len * (0.5 / (double)(1 << LG_BISECT));
  if (lb) *lb = bound;
  return bound < reach;
}

// Forward kinematics of the body chain and the world end points of the capsules c = sub, sub + lpe, ... -> w[LG_CAPW c ..];
// the frames of the cubes b = sub, sub + lpe, ... -> w[LG_MAXCAP LG_CAPW + LG_BOXW b ..].  q: 7 hinges + 2 finger slides;
// box(b, k): word k (pos 3, quat 4) of cube b.
template <class PC, class BOX>
D3IL_HD void lg_place(const PC& c, const LinkGuardConsts& lg, int nb, const double* q, BOX box, double* w, int sub, int lpe) {
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, p[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k <= NARM; k++) {
    if (k > 0) {      // the frame behind joint k (world_chain of panda_step.h, one link at a time)
      const int i = k - 1;
      double t[3], E[9], Rn[9], sn, cs;
      mulE(R, c.P[i], t);
      p[0] += t[0]; p[1] += t[1]; p[2] += t[2];
      sincos(q[i], &sn, &cs);
      joint_rot(c.Q[i], sn, cs, E);
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int cc = 0; cc < 3; cc++) Rn[3 * r + cc] = R[3 * r] * E[cc] + R[3 * r + 1] * E[3 + cc] + R[3 * r + 2] * E[6 + cc];
#pragma unroll
      for (int j = 0; j < 9; j++) R[j] = Rn[j];
    }
    for (int cap = sub; cap < lg.n; cap += lpe) {
      if (lg.link[cap] != k) continue;
      double a[3] = {lg.p0[cap][0], lg.p0[cap][1], lg.p0[cap][2]}, b[3] = {lg.p1[cap][0], lg.p1[cap][1], lg.p1[cap][2]}, t[3];
      const int f = lg.finger[cap];
      if (f >= 0) {
        const double qf = f == 0 ? q[NARM] : q[NARM + 1];      // (selects, not indexed: q lives in registers)
#pragma unroll
        for (int j = 0; j < 3; j++) { const double ax = f == 0 ? c.f_axis[0][j] : c.f_axis[1][j]; a[j] += ax * qf; b[j] += ax * qf; }
      }
      double* o = w + LG_CAPW * cap;
      mulE(R, a, t); o[0] = p[0] + t[0]; o[1] = p[1] + t[1]; o[2] = p[2] + t[2];
      mulE(R, b, t); o[3] = p[0] + t[0]; o[4] = p[1] + t[1]; o[5] = p[2] + t[2];
      o[6] = lg.r[cap];
    }
  }
  for (int b = sub; b < nb; b += lpe) {
    double* o = w + LG_MAXCAP * LG_CAPW + LG_BOXW * b;
    double qt[4] = {box(b, 3), box(b, 4), box(b, 5), box(b, 6)};
    const double nrm = 1.0 / sqrt(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3]);
#pragma unroll
    for (int j = 0; j < 4; j++) qt[j] *= nrm;
    o[0] = box(b, 0); o[1] = box(b, 1); o[2] = box(b, 2);
    quat2mat(qt, o + 3);
  }
}

// The pairs of the capsules c = sub, sub + lpe, ...: true when one of them is below the margin.  dmin (optional): the smallest bound seen.
D3IL_HD bool lg_test(const GenConsts& gc0, const LinkGuardConsts& lg, const double* w, int sub, int lpe, double* dmin) {
  D3IL_GEN_CONSTS(gc0, gc);
  bool near = false;
  for (int cap = sub; cap < lg.n; cap += lpe) {
    const double* o = w + LG_CAPW * cap;
    const double a[3] = {o[0], o[1], o[2]}, b[3] = {o[3], o[4], o[5]}, r = o[6];
    const double reach = r + lg.margin;
    for (int k = 0; k < gc.nb; k++) {
      const double* bx = w + LG_MAXCAP * LG_CAPW + LG_BOXW * k;
      double lb;
      near = lg_seg_box_near(a, b, bx, bx + 3, gc.box_half, reach, &lb) || near;
      if (dmin && lb - r < *dmin) *dmin = lb - r;
    }
    if (!lg.statics[cap]) continue;
    for (int s = 0; s < gc.ns; s++) {
      double lb;
      near = lg_seg_box_near(a, b, gc.st_c[s], gc.st_R[s], gc.st_h[s], reach, &lb) || near;
      if (dmin && lb - r < *dmin) *dmin = lb - r;
    }
  }
  return near;
}

// Host side of d3il_set_link_guard: capsules [n][9] = body id in the blob's body list, 1 = also against the static boxes, p0[3], p1[3]
// (body frame), r  ->  the frame the kernel places them in.  A body welded to an arm link (link8, hand) goes into that link's frame,
// a finger (or its tip body) into link 7's with its slide, link0 - welded to the world on the way to joint 1 - into the world.
// Returns 0, or a negative code with *err set: a body outside the chain, r <= 0, margin < 0, n above LG_MAXCAP, a segment above LG_MAXLEN.
inline int build_link_guard(const d3il_model_blob& m, const double* caps, int n, double margin, LinkGuardConsts& lg, const char** err) {
  using namespace hostmath;
  std::memset(&lg, 0, sizeof lg);
  if (n < 0 || n > LG_MAXCAP) { *err = "link guard: n must be in 0 .. 16"; return -1; }
  if (!(margin >= 0) || !(margin < 1e300)) { *err = "link guard: margin must be >= 0"; return -1; }
  if (n > 0 && !caps) { *err = "link guard: null capsule array"; return -1; }
  if (m.nu != NDOF) { *err = "link guard: expected 9 actuators"; return -1; }
  static thread_local Xf X0[D3IL_MAXBODY];
  X0[0] = identity();
  for (int b = 1; b < m.nbody; b++) { Xf l; hostmath::quat2mat(m.body_quat[b], l.R); std::memcpy(l.p, m.body_pos[b], sizeof l.p); X0[b] = compose(X0[m.body_parent[b]], l); }
  auto rel = [&](int a, int b) {  // a <- b at q = 0
    Xf inv; for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) inv.R[3 * i + j] = X0[a].R[3 * j + i];
    double t[3]; mv(inv.R, X0[a].p, t); for (int k = 0; k < 3; k++) inv.p[k] = -t[k];
    return compose(inv, X0[b]);
  };
  auto weld_root = [&](int b) { while (b > 0 && m.body_jntnum[b] == 0) b = m.body_parent[b]; return b; };
  int lbody[NARM], fbody[NFING];
  for (int k = 0; k < NARM; k++) lbody[k] = m.jnt_body[m.act_jnt[k]];
  for (int k = 0; k < NFING; k++) fbody[k] = m.jnt_body[m.act_jnt[NARM + k]];
  lg.n = n; lg.margin = margin;
  for (int i = 0; i < n; i++) {
    const double* cp = caps + 9 * i;
    for (int k = 0; k < 9; k++) if (!(cp[k] > -1e300 && cp[k] < 1e300)) { *err = "link guard: a capsule holds NaN / Inf"; return -1; }
    const int body = (int)cp[0];
    if ((double)body != cp[0] || body < 1 || body >= m.nbody) { *err = "link guard: body id outside the model"; return -1; }
    if (!(cp[8] > 0)) { *err = "link guard: r must be positive"; return -1; }
    const int root = weld_root(body);
    Xf x;
    lg.finger[i] = -1;
    if (root == 0) {      // welded to the world: only the bodies between the world and link 1 (link0) belong to the chain
      bool on_path = false;
      for (int b = m.body_parent[lbody[0]]; b > 0; b = m.body_parent[b]) on_path = on_path || b == body;
      if (!on_path) { *err = "link guard: body id outside the robot's chain"; return -1; }
      lg.link[i] = 0; x = X0[body];
    } else {
      int k = 0;
      while (k < NARM && lbody[k] != root) k++;
      if (k < NARM) { lg.link[i] = k + 1; x = rel(root, body); }
      else {
        int f = 0;
        while (f < NFING && fbody[f] != root) f++;
        if (f == NFING) { *err = "link guard: body id outside the robot's chain"; return -1; }
        lg.link[i] = NARM; lg.finger[i] = f; x = rel(lbody[NARM - 1], body);
      }
    }
    lg.statics[i] = cp[1] != 0.0 ? 1 : 0;
    double t[3];
    mv(x.R, cp + 2, t); for (int k = 0; k < 3; k++) lg.p0[i][k] = t[k] + x.p[k];
    mv(x.R, cp + 5, t); for (int k = 0; k < 3; k++) lg.p1[i][k] = t[k] + x.p[k];
    lg.r[i] = cp[8];
    double L2 = 0;
    for (int k = 0; k < 3; k++) L2 += (cp[5 + k] - cp[2 + k]) * (cp[5 + k] - cp[2 + k]);
    if (!(L2 <= LG_MAXLEN * LG_MAXLEN)) { *err = "link guard: a capsule segment is longer than 1 m"; return -1; }
  }
  return 0;
}

#if defined(__HIPCC__)
// one launch per env step, behind the step kernel on its stream; flagged (may be null): += 1 for every environment whose bit goes 0 -> 1
__global__ __launch_bounds__(GEN_WAVE) void k_gen_link_guard(const LinkGuardConsts* __restrict__ lgp, const double* __restrict__ state, unsigned* __restrict__ flags,
                                                             unsigned long long* __restrict__ flagged, int n, int stride) {
  __shared__ double work[LG_ENVS][LG_WORK];
  const int lane = threadIdx.x, col = lane / LG_LPE, sub = lane & (LG_LPE - 1);
  const int e = blockIdx.x * LG_ENVS + col;
  const bool live = e < n;
  const GenConsts& gc = g_gen_consts;
  const LinkGuardConsts& lg = *lgp;                      // (the arm is the Avoiding arm, as in the step kernel: kAvoidingConsts)
  const double* sp = state + (live ? e : 0);
#if defined(D3IL_POISON)
  // guard build (rigid_common.h): a capsule or cube slot that lg_test reads and lg_place skipped (fewer cubes than GEN_MAXNB) is a NaN
  for (int q = lane; q < LG_ENVS * LG_WORK; q += GEN_WAVE) ((unsigned long long*)&work[0][0])[q] = D3IL_POISON_BITS;
  __syncthreads();
#endif
  if (live) {
    double q[NDOF];
#pragma unroll
    for (int i = 0; i < NDOF; i++) q[i] = sp[(D3IL_STATE_QPOS + i) * (size_t)stride];
    lg_place(kAvoidingConsts, lg, gc.nb, q, [&](int b, int k) { return sp[(size_t)(42 + 13 * b + k) * stride]; }, work[col], sub, LG_LPE);
  }
  __syncthreads();
  int near = 0;
  if (live) near = lg_test(gc, lg, work[col], sub, LG_LPE, nullptr) ? 1 : 0;
#pragma unroll
  for (int m = 1; m < LG_LPE; m <<= 1) near |= __shfl_xor(near, m);
  if (live && sub == 0 && near) {
    const unsigned old = flags[e];
    if (!(old & LG_FLAG)) {
      flags[e] = old | LG_FLAG;
      if (flagged) atomicAdd(flagged, 1ull);
    }
  }
}
#endif

}  // namespace d3il
