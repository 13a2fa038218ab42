// TEST-ONLY host build of the link-near guard (d3il_amd/csrc/link_guard.h): the functions the kernel k_gen_link_guard runs, compiled for the CPU with one
// "lane" per environment, so that the forward kinematics, the capsule placement and the segment <-> box distance are checked without a GPU
// (tests/test_link_guard_host.py).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "../../d3il_amd/csrc/link_guard.h"

using namespace d3il;

struct GuardHost { PandaConsts c; GenConsts gc; LinkGuardConsts lg; d3il_model_blob blob; };

extern "C" {
void* lgc_create(const d3il_model_blob* blob, const char** err) {
  GuardHost* p = (GuardHost*)std::calloc(1, sizeof(GuardHost));
  static const char* e = "";
  if (build_panda_consts(*blob, p->c, &e)) { *err = e; std::free(p); return nullptr; }
  finish_invweights(p->c);
  if (build_gen_consts(*blob, p->c, p->gc, &e)) { *err = e; std::free(p); return nullptr; }
  p->blob = *blob;
  return p;
}
void lgc_destroy(void* h) { std::free(h); }
// as d3il_set_link_guard: 0, or -1 with *err set
int lgc_set(void* h, const double* caps, int n, double margin, const char** err) {
  GuardHost* p = (GuardHost*)h;
  static const char* e = "";
  int rc = build_link_guard(p->blob, caps, n, margin, p->lg, &e);
  *err = e;
  return rc;
}
double lgc_slack(void) { return LG_SLACK; }
// the lower bound of distance(segment a b, box) without the cull (reach = infinity)
double lgc_seg_box(const double* a, const double* b, const double* c, const double* R9, const double* h) {
  double lb = 0;
  lg_seg_box_near(a, b, c, R9, h, 1e300, &lb);
  return lb;
}
int lgc_info(void* h, int* nb, int* ns, double* statics /* ns x (c3, h3, R9) */, double* box_half) {
  GuardHost* p = (GuardHost*)h; *nb = p->gc.nb; *ns = p->gc.ns;
  for (int s = 0; s < p->gc.ns; s++) {
    for (int k = 0; k < 3; k++) { statics[15 * s + k] = p->gc.st_c[s][k]; statics[15 * s + 3 + k] = p->gc.st_h[s][k]; }
    for (int k = 0; k < 9; k++) statics[15 * s + 6 + k] = p->gc.st_R[s][k];
  }
  for (int k = 0; k < 3; k++) box_half[k] = p->gc.box_half[k];
  return p->lg.n;
}
// the verdict of one environment: q[9], cubes [nb][7] (pos, quat); world_caps (optional) [n][7] = the capsules as placed; dmin (optional) = smallest bound seen
int lgc_eval(void* h, const double* q, const double* cubes, double* world_caps, double* dmin) {
  GuardHost* p = (GuardHost*)h;
  double w[LG_WORK];
  std::memset(w, 0, sizeof w);
  lg_place(p->c, p->lg, p->gc.nb, q, [&](int b, int k) { return cubes[7 * b + k]; }, w, 0, 1);
  if (world_caps) std::memcpy(world_caps, w, sizeof(double) * LG_CAPW * p->lg.n);
  double dm = 1e300;
  const bool near = lg_test(p->gc, p->lg, w, 0, 1, &dm);
  if (dmin) *dmin = dm;
  return near ? 1 : 0;
}
}
