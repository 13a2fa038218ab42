// hostcheck.cpp - TEST-ONLY host build of the kernels' per-environment math (d3il_amd/csrc/panda_step.h).
// Lets the CPU test-suite compare the exact device formulation against the oracle without a GPU.
// It is NOT part of the product: libd3il_rollout.so never links or calls this file, and the product
// fails loudly when no HIP device is present.
#define D3IL_HOST_STATS 1
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "../../d3il_amd/csrc/gen_step.h"
#include "../../d3il_amd/csrc/stack_step.h"

using namespace d3il;

static void unpack(const double* s, const int* f, EnvState& st) {
  int k = 0;
  for (int i = 0; i < NDOF; i++) st.q[i] = s[k++];
  for (int i = 0; i < NDOF; i++) st.v[i] = s[k++];
  for (int i = 0; i < NARM; i++) st.bias[i] = s[k++];
  for (int i = 0; i < 3; i++) st.tcp[i] = s[k++];
  for (int i = 0; i < NARM; i++) st.ikq[i] = s[k++];
  for (int i = 0; i < NARM; i++) st.ikqd[i] = s[k++];
  st.flags = (unsigned)f[0]; st.step = f[1];
}
static void pack(const EnvState& st, double* s, int* f) {
  int k = 0;
  for (int i = 0; i < NDOF; i++) s[k++] = st.q[i];
  for (int i = 0; i < NDOF; i++) s[k++] = st.v[i];
  for (int i = 0; i < NARM; i++) s[k++] = st.bias[i];
  for (int i = 0; i < 3; i++) s[k++] = st.tcp[i];
  for (int i = 0; i < NARM; i++) s[k++] = st.ikq[i];
  for (int i = 0; i < NARM; i++) s[k++] = st.ikqd[i];
  f[0] = (int)st.flags; f[1] = st.step;
}

extern "C" {
void* hc_create(const d3il_model_blob* blob, const char** err) {
  PandaConsts* c = (PandaConsts*)std::malloc(sizeof(PandaConsts));
  static const char* e = "";
  int rc = build_panda_consts(*blob, *c, &e);
  if (rc) { *err = e; std::free(c); return nullptr; }
  finish_invweights(*c);
  return c;
}
void hc_destroy(void* c) { std::free(c); }
void hc_stats(long* out, int reset) { out[0] = g_stats.newton_calls; out[1] = g_stats.newton_iters; out[2] = g_stats.ls_iters; out[3] = g_stats.eig_calls; out[4] = g_stats.ik_calls; out[5] = g_stats.contact_calls; if (reset) g_stats = Stats{0, 0, 0, 0, 0, 0}; }
// 0: the production stopping rule of the contact solvers, 1: the oracle's (iterate to round-off) - the device's option solver_strict
void hc_set_solver_strict(int strict) { host_solver_tol() = strict ? SOLVER_TOL_STRICT : SOLVER_TOL_PRODUCTION; }
int hc_sizeof_consts() { return (int)sizeof(PandaConsts); }
void hc_get_consts(const void* c, double* dof_invw, double* rod_invw, double* masses, double* coms) {
  const PandaConsts& p = *(const PandaConsts*)c;
  std::memcpy(dof_invw, p.dof_invweight0, sizeof p.dof_invweight0); *rod_invw = p.rod_invweight0;
  std::memcpy(masses, p.mass, sizeof p.mass); std::memcpy(coms, p.com, sizeof p.com);
}
void hc_dynamics(const void* c, const double* q, const double* v, double* M81, double* bias, double* tcp) {
  const PandaConsts& p = *(const PandaConsts*)c;
  DynOut d; dynamics(p, q, v, d);
  for (int r = 0; r < NDOF; r++) for (int k = 0; k < NDOF; k++) M81[r * NDOF + k] = d.M[r >= k ? tri(r, k) : tri(k, r)];
  std::memcpy(bias, d.bias, sizeof d.bias);
  double t[3]; mulE(d.R7, p.tcp7, t); for (int k = 0; k < 3; k++) tcp[k] = d.p7[k] + t[k];
}
void hc_ik_fk(const void* c, const double* q, double* pos, double* quat, double* J42) {
  const PandaConsts& p = *(const PandaConsts*)c;
  double R[9], ax[NARM][3], og[NARM][3], sq[NARM], cq[NARM];
  for (int k = 0; k < NARM; k++) { sq[k] = std::sin(q[k]); cq[k] = std::cos(q[k]); }
  ik_chain(p, sq, cq, pos, R, ax, og); mat2quat(R, quat);
  for (int k = 0; k < NARM; k++) { double d[3] = {pos[0] - og[k][0], pos[1] - og[k][1], pos[2] - og[k][2]}, cr[3]; cross3(ax[k], d, cr);
    for (int r = 0; r < 3; r++) { J42[r * NARM + k] = cr[r]; J42[(3 + r) * NARM + k] = ax[k][r]; } }
}
// one controller call: returns PD torque (without gravity compensation), updates ikq/ikqd/flags
void hc_ik_control(const void* c, const double* setpoint, const double* cur_q, const double* cur_v, double* ikq, double* ikqd, int* flags, int fast, double* tau) {
  const PandaConsts& p = *(const PandaConsts*)c;
  unsigned f = (unsigned)*flags;
  double n = std::sqrt(setpoint[3] * setpoint[3] + setpoint[4] * setpoint[4] + setpoint[5] * setpoint[5] + setpoint[6] * setpoint[6]);
  double dq[4] = {setpoint[3] / n, setpoint[4] / n, setpoint[5] / n, setpoint[6] / n};
  if (fast) ik_update<true>(p, setpoint, dq, cur_q, f, ikq, ikqd); else ik_update<false>(p, setpoint, dq, cur_q, f, ikq, ikqd);
  for (int k = 0; k < NARM; k++) tau[k] = p.pd_p[k] * (ikq[k] - cur_q[k]) + p.pd_d[k] * (ikqd[k] - cur_v[k]);
  *flags = (int)f;
}
void hc_solve6(const double* A21, const double* b, double lo, double hi, double* x, int fast) { if (fast) ik_solve6<true>(A21, b, lo, hi, x); else ik_solve6<false>(A21, b, lo, hi, x); }
// the solve as the kernels call it: vwarm (7 doubles, in/out, may be NULL) = the eigenvector accepted by the previous solve, [6] != 0 when valid
void hc_solve6_warm(const double* A21, const double* b, double lo, double hi, double* x, int fast, double* vwarm) {
  if (fast) ik_solve6<true>(A21, b, lo, hi, x, vwarm); else ik_solve6<false>(A21, b, lo, hi, x, vwarm);
}
// hc_ik_control in the kernels' calling form: vwarm (7 doubles) and trig (15 doubles: sin[7] cos[7] of ikq, [14] != 0 when valid), each in/out, each may be NULL
void hc_ik_control_form(const void* c, const double* setpoint, const double* cur_q, const double* cur_v, double* ikq, double* ikqd, int* flags, int fast, double* tau,
                        double* vwarm, double* trig) {
  const PandaConsts& p = *(const PandaConsts*)c;
  unsigned f = (unsigned)*flags;
  double n = std::sqrt(setpoint[3] * setpoint[3] + setpoint[4] * setpoint[4] + setpoint[5] * setpoint[5] + setpoint[6] * setpoint[6]);
  double dq[4] = {setpoint[3] / n, setpoint[4] / n, setpoint[5] / n, setpoint[6] / n};
  if (fast) ik_update<true>(p, setpoint, dq, cur_q, f, ikq, ikqd, vwarm, trig); else ik_update<false>(p, setpoint, dq, cur_q, f, ikq, ikqd, vwarm, trig);
  for (int k = 0; k < NARM; k++) tau[k] = p.pd_p[k] * (ikq[k] - cur_q[k]) + p.pd_d[k] * (ikqd[k] - cur_v[k]);
  *flags = (int)f;
}
// the controller's linear system at the virtual joint target q (one iteration of ik_update, before the solve): A (packed lower triangle, 21) and its right-hand side
void hc_ik_system(const void* c, const double* setpoint, const double* q, double* A21, double* rhs) {
  const PandaConsts& p = *(const PandaConsts*)c;
  double n = std::sqrt(setpoint[3] * setpoint[3] + setpoint[4] * setpoint[4] + setpoint[5] * setpoint[5] + setpoint[6] * setpoint[6]);
  double dq[4] = {setpoint[3] / n, setpoint[4] / n, setpoint[5] / n, setpoint[6] / n};
  double pos[3], R[9], ax[NARM][3], og[NARM][3], sq[NARM], cq[NARM], cq4[4], qe[3], target[6], J[6][NARM], qn[NARM];
  for (int k = 0; k < NARM; k++) { sq[k] = std::sin(q[k]); cq[k] = std::cos(q[k]); }
  ik_chain(p, sq, cq, pos, R, ax, og); mat2quat(R, cq4);
  double dm = 0, dp = 0;
  for (int k = 0; k < 4; k++) { dm += (cq4[k] - dq[k]) * (cq4[k] - dq[k]); dp += (cq4[k] + dq[k]) * (cq4[k] + dq[k]); }
  if (dm > dp) for (int k = 0; k < 4; k++) dq[k] = -dq[k];
  quat_error(cq4, dq, qe);
  for (int k = 0; k < 3; k++) { target[k] = p.ik_ppos[k] * clampd(setpoint[k] - pos[k], -0.01, 0.01); target[3 + k] = p.ik_pquat[k] * clampd(qe[k], -0.1, 0.1); }
  for (int k = 0; k < NARM; k++) { double d[3] = {pos[0] - og[k][0], pos[1] - og[k][1], pos[2] - og[k][2]}, cr[3]; cross3(ax[k], d, cr);
    for (int r = 0; r < 3; r++) { J[r][k] = cr[r]; J[3 + r][k] = ax[k][r]; } }
  for (int a = 0; a < 6; a++) for (int b = 0; b <= a; b++) { double s = a == b ? p.ik_Jreg : 0.0; for (int k = 0; k < NARM; k++) s += J[a][k] * J[b][k]; A21[tri(a, b)] = s; }
  for (int k = 0; k < NARM; k++) qn[k] = p.ik_pnull[k] * clampd(p.ik_rest[k] - q[k], -0.2, 0.2);
  for (int a = 0; a < 6; a++) { double s = target[a]; for (int k = 0; k < NARM; k++) s -= J[a][k] * qn[k]; rhs[a] = s; }
}
void hc_ik_params(const void* c, double* out /* ik_minsv, ik_maxsv, ik_Jreg, ik_lr, ik_iters, n_substeps, q_min[7], q_max[7], pd_p[7], pd_d[7], timestep */) {
  const PandaConsts& p = *(const PandaConsts*)c;
  out[0] = p.ik_minsv; out[1] = p.ik_maxsv; out[2] = p.ik_Jreg; out[3] = p.ik_lr; out[4] = p.ik_iters; out[5] = p.n_substeps;
  for (int k = 0; k < NARM; k++) { out[6 + k] = p.q_min[k]; out[6 + NARM + k] = p.q_max[k]; out[6 + 2 * NARM + k] = p.pd_p[k]; out[6 + 3 * NARM + k] = p.pd_d[k]; }
  out[6 + 4 * NARM] = p.timestep;
}
void hc_physics_substep(const void* c, double* s, int* f, const double* tau, const double* ffing) {
  EnvState st; unpack(s, f, st); double warm[6]; warm[5] = 0; physics_substep(*(const PandaConsts*)c, st, tau, ffing, warm); pack(st, s, f);
}
void hc_env_reset(const void* c, const double* init_qpos, double* s, int* f, float* obs) {
  EnvState st; std::memset(&st, 0, sizeof st);
  env_reset(*(const PandaConsts*)c, st, init_qpos, obs); pack(st, s, f);
}
void hc_env_step(const void* c, double* s, int* f, const double* action, float* obs, unsigned char* done, int fast) {
  EnvState st; unpack(s, f, st);
  const PandaConsts& pc = *(const PandaConsts*)c;
  if (fast) env_step<true>(pc, st, action, obs, done, pc.n_substeps, pc.max_steps); else env_step<false>(pc, st, action, obs, done, pc.n_substeps, pc.max_steps);
  pack(st, s, f);
}

// ---------------------------------------------------------------- generic engine / Sorting (gen_step.h)
struct GenHost { PandaConsts c; GenConsts gc; double h[GL_SIZE]; double g[GG_SIZE]; };
void* hc_gen_create(const d3il_model_blob* blob, const char** err) {
  GenHost* p = (GenHost*)std::calloc(1, sizeof(GenHost));
  static const char* e = "";
  if (build_panda_consts(*blob, p->c, &e)) { *err = e; std::free(p); return nullptr; }
  finish_invweights(p->c);
  if (build_gen_consts(*blob, p->c, p->gc, &e)) { *err = e; std::free(p); return nullptr; }
  return p;
}
int hc_gen_info(void* h, int* nb, int* ns, double* statics /* ns x (c3, h3, first) */) {
  GenHost* p = (GenHost*)h; *nb = p->gc.nb; *ns = p->gc.ns;
  for (int s = 0; s < p->gc.ns; s++) { for (int k = 0; k < 3; k++) { statics[7 * s + k] = p->gc.st_c[s][k]; statics[7 * s + 3 + k] = p->gc.st_h[s][k]; } statics[7 * s + 6] = p->gc.st_first[s]; }
  return gen_state_rows(p->gc.nb);
}
// the split of the static list: [0, ns_core) inside the table, the rest = frame beams; and the two workspaces (inner lo / hi, outer lo / hi)
int hc_gen_workspace(void* h, double* ws8) {
  GenHost* p = (GenHost*)h;
  for (int k = 0; k < 2; k++) { ws8[k] = p->gc.in_lo[k]; ws8[2 + k] = p->gc.in_hi[k]; ws8[4 + k] = p->gc.ws_lo[k]; ws8[6 + k] = p->gc.ws_hi[k]; }
  return p->gc.ns_core;
}
// read-before-write detector of the generic engine (like hc_stack_poison): when on, the t area (the device's LDS block) and the record area hold NaN before
// every reset, env step and single sub-step; the warm start is carried in the state rows, nothing else is meant to be carried
static int g_gen_poison = 0;
void hc_gen_poison(int on) { g_gen_poison = on; }
static void gen_poison_fill(GenHost* p) {
  if (!g_gen_poison) return;
  for (int i = 0; i < GL_SIZE; i++) p->h[i] = std::nan("");
  for (int i = 0; i < GG_SIZE; i++) p->g[i] = std::nan("");
}
// what the collision phases of the last sub-step found: out[b] = the info word of cube b (contact count | partner cubes << 5 | rod contact << 9),
// out[GEN_MAXNB] = rod <-> static box contacts (tasks that evaluate those pairs; else 0)
void hc_gen_contact_info(void* h, int* out) {
  GenHost* p = (GenHost*)h;
  for (int b = 0; b < GEN_MAXNB; b++) out[b] = b < p->gc.nb ? (int)(unsigned)p->h[GL_INFO + b] : 0;
  out[GEN_MAXNB] = p->gc.rod_static ? (int)(unsigned)p->h[GL_INFO + 8] : 0;
}
// s: the environment's state column (arm[42] | cubes | warm start | task words), f: flags, step
void hc_gen_reset(void* h, const double* init_qpos, const double* ctx, double* s, int* f, float* obs) {
  GenHost* p = (GenHost*)h; EnvState st; std::memset(&st, 0, sizeof st);
  gen_poison_fill(p);
  PushScratch sc{p->h, p->g, 1, s + 42, 1};
  gen_env_reset(p->c, p->gc, st, sc, init_qpos, ctx, obs); pack(st, s, f);
}
void hc_gen_step(void* h, double* s, int* f, const double* action, float* obs, unsigned char* done, int* mode_code, int fast) {
  GenHost* p = (GenHost*)h; EnvState st; unpack(s, f, st);
  gen_poison_fill(p);
  PushScratch sc{p->h, p->g, 1, s + 42, 1};
  if (fast) gen_env_step<true>(p->c, p->gc, st, sc, action, obs, done, mode_code, p->c.n_substeps, p->c.max_steps);
  else gen_env_step<false>(p->c, p->gc, st, sc, action, obs, done, mode_code, p->c.n_substeps, p->c.max_steps);
  pack(st, s, f);
}
void hc_gen_island_hist(long* out, int reset) { for (int k = 0; k < 80; k++) { out[k] = g_isl_hist[k]; if (reset) g_isl_hist[k] = 0; } }
void hc_gen_substep(void* h, double* s, int* f, const double* tau, const double* ffing) {
  GenHost* p = (GenHost*)h; EnvState st; unpack(s, f, st);
  gen_poison_fill(p);
  PushScratch sc{p->h, p->g, 1, s + 42, 1};
  gen_physics_substep(p->c, p->gc, st, sc, tau, ffing); pack(st, s, f);
}
// the control law of a sub-step on its own (joint PD towards q_des / qd_des + finger PD, as gen_control_and_physics applies it): torques for hc_gen_substep
void hc_gen_control(void* h, const double* s, const int* f, const double* q_des, const double* qd_des, double* tau, double* ffing) {
  GenHost* p = (GenHost*)h; EnvState st; unpack(s, f, st);
  push_control(p->c, st, q_des, qd_des, 0.04, false, tau, ffing);
}
// ---------------------------------------------------------------- Stacking (stack_step.h)
struct StackHost { PandaConsts c; StackConsts kc; double t[ST_SIZE]; double g[SG_SIZE]; };
static void stack_unpack(const double* s, const int* f, StackState& ss) {
  int k = 0;
  for (int i = 0; i < NDOF; i++) ss.arm.q[i] = s[k++];
  for (int i = 0; i < NDOF; i++) ss.arm.v[i] = s[k++];
  for (int i = 0; i < NARM; i++) ss.arm.bias[i] = s[k++];
  for (int i = 0; i < 3; i++) ss.arm.tcp[i] = s[k++];
  for (int b = 0; b < SK_NB; b++) { for (int i = 0; i < 3; i++) ss.box[b].pos[i] = s[k++]; for (int i = 0; i < 4; i++) ss.box[b].quat[i] = s[k++]; for (int i = 0; i < 6; i++) ss.box[b].vel[i] = s[k++]; }
  for (int i = 0; i < SK_NV; i++) ss.warm[i] = s[k++];
  ss.arm.flags = (unsigned)f[0]; ss.arm.step = f[1];
}
static void stack_pack(const StackState& ss, double* s, int* f) {
  int k = 0;
  for (int i = 0; i < NDOF; i++) s[k++] = ss.arm.q[i];
  for (int i = 0; i < NDOF; i++) s[k++] = ss.arm.v[i];
  for (int i = 0; i < NARM; i++) s[k++] = ss.arm.bias[i];
  for (int i = 0; i < 3; i++) s[k++] = ss.arm.tcp[i];
  for (int b = 0; b < SK_NB; b++) { for (int i = 0; i < 3; i++) s[k++] = ss.box[b].pos[i]; for (int i = 0; i < 4; i++) s[k++] = ss.box[b].quat[i]; for (int i = 0; i < 6; i++) s[k++] = ss.box[b].vel[i]; }
  for (int i = 0; i < SK_NV; i++) s[k++] = ss.warm[i];
  f[0] = (int)ss.arm.flags; f[1] = ss.arm.step;
}
void* hc_stack_create(const d3il_model_blob* blob, const char** err) {
  StackHost* p = (StackHost*)std::calloc(1, sizeof(StackHost));
  static const char* e = "";
  if (build_panda_consts(*blob, p->c, &e)) { *err = e; std::free(p); return nullptr; }
  finish_invweights(p->c);
  if (build_stack_consts(*blob, p->c, p->kc, &e)) { *err = e; std::free(p); return nullptr; }
  return p;
}
int hc_stack_state_size() { return SK_STATE_F64; }
void hc_stack_reset(void* h, const double* init_qpos, const double* ctx, double* s, int* f, float* obs) {
  StackHost* p = (StackHost*)h; StackState ss; std::memset(&ss, 0, sizeof ss);
  StackScratch sc{p->t, p->g};
  stack_env_reset(p->c, p->kc, ss, sc, init_qpos, ctx, obs); stack_pack(ss, s, f);
}
static int g_stack_poison = 0;
void hc_stack_poison(int on) { g_stack_poison = on; }
void hc_stack_step(void* h, double* s, int* f, const double* action, float* obs, unsigned char* done, double* mean_dist) {
  StackHost* p = (StackHost*)h; StackState ss; stack_unpack(s, f, ss);
  if (g_stack_poison) {   // read-before-write detector: the scratch areas hold NaN before every step
    for (int i = 0; i < ST_SIZE; i++) p->t[i] = std::nan("");
    for (int i = 0; i < SG_SIZE; i++) p->g[i] = std::nan("");
  }
  StackScratch sc{p->t, p->g};
  stack_env_step(p->c, p->kc, ss, sc, action, obs, done, mean_dist, p->c.n_substeps, p->c.max_steps);
  stack_pack(ss, s, f);
}
void hc_stack_scratch(void* h, double* out, int count) { StackHost* p = (StackHost*)h; std::memcpy(out, p->g, (size_t)count * sizeof(double)); }
// contacts of the last sub-step: per contact dist, pos3, normal3, bodyA, bodyB, set
int hc_stack_contacts(void* h, double* out) {
  StackHost* p = (StackHost*)h; int n = 0;
  for (int ci = 0; ci < SK_MAXCON; ci++) {
    const double* r = p->g + ci * SREC;
    if (r[3] == 0 && r[4] == 0 && r[5] == 0) break;
    out[10 * n] = r[12]; for (int k = 0; k < 3; k++) { out[10 * n + 1 + k] = r[k]; out[10 * n + 4 + k] = r[3 + k]; }
    out[10 * n + 7] = r[13]; out[10 * n + 8] = r[14]; out[10 * n + 9] = r[15]; n++;
  }
  return n;
}
// collision routines of push_step.h on their own (quaternions in, same record layout as the oracle's test hooks)
int hc_cyl_box(const double* pc, const double* qc, double rad, double half, const double* pb, const double* qb, const double* sb, double margin, double* out) {
  double Rc[9], Rb[9]; quat2mat(qc, Rc); quat2mat(qb, Rb);
  double axis[3] = {Rc[2], Rc[5], Rc[8]};
  return cyl_box(pc, axis, rad, half, pb, Rb, sb, margin, out) ? 1 : 0;
}
int hc_box_box(const double* p1, const double* q1, const double* s1, const double* p2, const double* q2, const double* s2, double margin, double* out) {
  double R1[9], R2[9], rec[16][7]; quat2mat(q1, R1); quat2mat(q2, R2);
  int n = box_box(p1, R1, s1, p2, R2, s2, margin, rec, 16);
  std::memcpy(out, rec, n * 7 * sizeof(double));
  return n;
}
// ---------------------------------------------------------------- leaf routines of the contact engines by themselves (tests/contact_leaf_cases.py)
// box_box as the device check calls it: row-major R, the caller's cap, out [8][7] (rows >= the count are left as they were)
int hc_box_box_R(const double* p1, const double* R1, const double* s1, const double* p2, const double* R2, const double* s2, double margin, int cap, double* out) {
  return box_box(p1, R1, s1, p2, R2, s2, margin, (double (*)[7])out, cap);
}
int hc_cyl_box_axis(const double* pc, const double* axis, double rad, double half, const double* pb, const double* Rb, const double* sb, double margin, double* out) {
  return cyl_box(pc, axis, rad, half, pb, Rb, sb, margin, out) ? 1 : 0;
}
// twin: gt_cone_eval (gen_tree.h)
double hc_cone_eval(const double* jar, double Dn, double Dt, double mu, double fric, double* force, double* Hc, int twin) {
  return twin ? gt_cone_eval(jar, Dn, Dt, mu, fric, force, Hc) : cone_eval(jar, Dn, Dt, mu, fric, force, Hc);
}
// A: packed lower triangle (n (n + 1) / 2), IN PLACE - its strict lower part becomes L; b -> x; d: the pivots.  Returns ok (1 / 0), -1 for another order.
int hc_ldl(int n, double* A, const double* b, double* x, double* d, int twin) {
  double id[6]; bool ok;
  if (n != 5 && n != 6) return -1;
  for (int i = 0; i < n; i++) x[i] = b[i];
  if (n == 5) { if (twin) { ok = gt_ldl_n<5>(A, d, id); gt_ldl_solve_n<5>(A, id, x); } else { ok = ldl_n<5>(A, d, id); ldl_solve_n<5>(A, id, x); } }
  else { if (twin) { ok = gt_ldl_n<6>(A, d, id); gt_ldl_solve_n<6>(A, id, x); } else { ok = ldl_n<6>(A, d, id); ldl_solve_n<6>(A, id, x); } }
  return ok ? 1 : 0;
}
// state13 = pos3 quat4 vel6, in place; K calls
void hc_cube_integrate(double* s, const double* acc, double h, int K) {
  BoxState bx;
  for (int k = 0; k < 3; k++) bx.pos[k] = s[k];
  for (int k = 0; k < 4; k++) bx.quat[k] = s[3 + k];
  for (int k = 0; k < 6; k++) bx.vel[k] = s[7 + k];
  for (int c = 0; c < K; c++) cube_integrate(bx, acc, h);
  for (int k = 0; k < 3; k++) s[k] = bx.pos[k];
  for (int k = 0; k < 4; k++) s[3 + k] = bx.quat[k];
  for (int k = 0; k < 6; k++) s[7 + k] = bx.vel[k];
}
double hc_tan_yaw(const double* q) { return push_tan_yaw(q); }
void hc_quat2mat(const double* q, double* R) { quat2mat(q, R); }
}
