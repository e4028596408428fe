// dem_laws.h -- the soft-disc contact laws as device functions: the drifted state of a grain (main.c:1748-1753), the two
// grain-grain laws (force_grains, main.c:739-774; the inline film law, main.c:1365-1395) and the four wall laws
// (force_WallB/T/L/R, main.c:809-951). ONE copy for everybody who evaluates a contact: the sub-step kernels
// (dem_kernels.hip) and the contact network export (lbm_contacts.hip), which re-derives a sub-step's contacts from the state
// that sub-step started from and has to arrive at the same bits.
#pragma once

#include "lbmdem_internal.h"

namespace {

// fn, ft, branch vector, vt: for the diagnostics; dn, xn, yn (the law's gap and normal, main.c:742, 752-753): for the contact
// network export -- the sub-step kernels never read them, so they cost those kernels nothing
struct Force3 { real f1, f2, f3, fn, ft, xij, yij, vt, dn, xn, yn; };

__device__ __forceinline__ real maxt(real x, real y) { return (x < y) ? 0. : y; }  // main.c:211-216

struct GrainState { real x1, x2, v1, v2, v3, r; };

// drifted + half-kicked state of grain j from the previous sub-step's state: main.c:1748-1753
__device__ __forceinline__ GrainState advance(const Kin& K, const real* __restrict__ r, int j,
                                              const DemParams& P) {
  GrainState s;
  const real a1 = K.a1[j], a2 = K.a2[j], a3 = K.a3[j];
  const real v1 = K.v1[j], v2 = K.v2[j], v3 = K.v3[j];
  s.x1 = K.x1[j] + P.dt * v1 + P.dt2 * a1 / 2.;
  s.x2 = K.x2[j] + P.dt * v2 + P.dt2 * a2 / 2.;
  s.v1 = v1 + P.dt * a1 / 2.;
  s.v2 = v2 + P.dt * a2 / 2.;
  s.v3 = v3 + P.dt * a3 / 2.;
  s.r = r[j];
  return s;
}

// contact force on grain A (lower index) from grain B (higher index).
// FILM = false: force_grains, main.c:739-774. FILM = true: the inline law of main.c:1365-1395.
template <bool FILM>
__device__ __forceinline__ Force3 contact(const GrainState& A, const GrainState& B, const DemParams& P,
                                          bool& touched) {
  Force3 F = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  const real xij = A.x1 - B.x1;
  const real yij = A.x2 - B.x2;
  const real dist = (real)sqrt((double)(xij * xij + yij * yij));   // <math.h>'s double sqrt, rounded to real (main.c:742)
  const real dn = dist - A.r - B.r;
  touched = !(dn >= 0);
  if (dn >= 0) return F;
  const real vx = A.v1 - B.v1;
  const real vy = A.v2 - B.v2;
  const real xn = xij / dist;
  const real yn = yij / dist;
  const real vn = vx * xn + vy * yn;
  const real vt = -vx * yn + vy * xn - A.v3 * A.r - B.v3 * B.r;
  if (!FILM) {
    // force_grains declares `double fn, ft` (main.c:736) whatever `real` is: f1, f2 and the arguments of Maxt are formed
    // in double and rounded to real once (fn and ft themselves always hold real values)
    double fn = -P.kg * dn - P.nug * vn;
    if (fn < 0) fn = 0.0;
    double ft = -P.kt * vt * P.dt;
    const real ftest = P.mu * fn;
    if (fabs(ft) > ftest) ft = (ft < 0.0) ? ftest : -ftest;
    F.f3 = -maxt((real)(ft * A.r), (real)(fn * P.murf * A.r * B.r));
    F.f1 = fn * xn - ft * yn;
    F.f2 = fn * yn + ft * xn;
    F.fn = fn;
    F.ft = ft;
  } else {
    // the inline film law uses acceleration_grains' own `real fn, ft` (main.c:1340)
    real fn = -P.kg * dn - P.nug * vn;
    if (fn < 0) fn = 0.0;
    real ft = P.kt * vt * P.dt;
    const real ftest = P.mu * ft;  // sic, main.c:1385
    if (fabs((double)ft) > ftest) ft = (ft > 0.0) ? ftest : -ftest;
    F.f3 = -ft * A.r * P.murf;
    F.f1 = fn * xn - ft * yn;
    F.f2 = fn * yn + ft * xn;
    F.fn = fn;
    F.ft = ft;
  }
  F.xij = xij;
  F.yij = yij;
  F.vt = vt;
  F.dn = dn;
  F.xn = xn;
  F.yn = yn;
  return F;
}

// One wall law applied to one grain: the law's gap dn, the reference's variables fn and ft of that wall's function as they
// stand when it returns, and the force f1, f2, f3 it hands back (all zero unless dn < 0: the reference does not call the law
// then, main.c:1457, 1474, 1485, 1502).
struct WallForce { real dn, fn, ft, f1, f2, f3; };

__device__ __forceinline__ WallForce wall_bottom(const GrainState& me, const DemParams& P) {   // force_WallB, main.c:809-828
  WallForce W = {me.x2 - me.r - P.Mby, 0., 0., 0., 0., 0.};
  if (W.dn < 0) {
    const real vn = me.v2, vt = me.v1;
    real fn = -P.km * W.dn - P.num * vn;
    if (fn < 0) fn = 0.;
    real ft = P.ktm * vt;
    const real ftest = P.mumb * fn;
    if (fabs((double)ft) > ftest) ft = (ft < 0.0) ? ftest : -ftest;
    W.fn = fn; W.ft = ft;
    W.f1 = ft; W.f2 = fn; W.f3 = -(ft * me.r * P.murf);
  }
  return W;
}

__device__ __forceinline__ WallForce wall_top(const GrainState& me, const DemParams& P) {   // force_WallT, main.c:846-871
  WallForce W = {-me.x2 - me.r + P.Mhy, 0., 0., 0., 0., 0.};
  if (W.dn < 0) {
    const real vn = me.v2;
    real fn = P.km * W.dn - P.num * vn;
    if (fn > 0.) fn = 0.;
    const real vt = me.v1 + me.v3 * me.r - P.wallT_vel;   // wallT_vel = amp * freq * cos(freq * t) is a double (main.c:855)
    real ft = fabs((double)(P.ktm * vt));
    real ftmax;
    if (vt >= 0) ftmax = P.mumb * fn - P.nugt * vt; else ftmax = P.mumb * fn + P.nugt * vt;
    if (ft > ftmax) ft = ftmax;
    if (vt > 0) ft = -ft;
    W.fn = fn; W.ft = ft;
    W.f1 = ft; W.f2 = fn; W.f3 = ft * me.r * P.murf;
  }
  return W;
}

__device__ __forceinline__ WallForce wall_left(const GrainState& me, const DemParams& P) {   // force_WallL, main.c:888-904
  WallForce W = {me.x1 - me.r - P.Mgx, 0., 0., 0., 0., 0.};
  if (W.dn < 0) {
    const real vn = me.v1;
    real fn = -P.km * W.dn + P.num * vn;
    if (fn < 0.) fn = 0.;
    const real vt = me.v2;
    real ft = P.mum * fn;
    if (vt > 0) ft = -ft;
    W.fn = fn; W.ft = ft;
    W.f1 = fn; W.f2 = ft; W.f3 = ft * me.r * P.murf;
  }
  return W;
}

__device__ __forceinline__ WallForce wall_right(const GrainState& me, const DemParams& P) {   // force_WallR, main.c:923-936
  WallForce W = {-me.x1 - me.r + P.Mdx, 0., 0., 0., 0., 0.};
  if (W.dn < 0) {
    const real vn = me.v1;
    real fn = P.km * W.dn - P.num * vn;
    const real vt = me.v2;
    real ft = P.mum * fn;   // (ft from the unclamped fn)
    if (vt > 0) ft = -ft;
    if (fn > 0.) fn = 0.;
    W.fn = fn; W.ft = ft;
    W.f1 = fn; W.f2 = -ft; W.f3 = ft * me.r * P.murf;
  }
  return W;
}

}  // namespace
