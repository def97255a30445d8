// The Solo12 leg model and its forward kinematics, shared by the kernels that run one lane per leg (wbc_kernel.hip: the
// whole-body controller; estimator_kernel.hip: the state estimator).  Small 3-vector / 3x3 helpers, the model constants of one
// leg (mirror images of the FL leg of include/qrw_solo12_model.h, proved at compile time) and leg_kinematics: joint origins,
// axes, link rotations, foot position and the three columns of the foot Jacobian in the base frame.
// Everything sits in an unnamed namespace: each translation unit that includes this gets its own, fully inlined copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/qrw_solo12_model.h"

namespace qrw {

namespace {

struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 mk(double x, double y, double z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return mk(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
struct M3 {
  V3 r0, r1, r2;  // rows
};
__device__ __forceinline__ V3 mul(const M3& m, V3 v) { return mk(dot(m.r0, v), dot(m.r1, v), dot(m.r2, v)); }
__device__ __forceinline__ V3 mulT(const M3& m, V3 v) {
  return mk(m.r0.x * v.x + m.r1.x * v.y + m.r2.x * v.z, m.r0.y * v.x + m.r1.y * v.y + m.r2.y * v.z,
            m.r0.z * v.x + m.r1.z * v.y + m.r2.z * v.z);
}
__device__ __forceinline__ V3 rotx(double c, double s, V3 v) { return mk(v.x, c * v.y - s * v.z, s * v.y + c * v.z); }
__device__ __forceinline__ V3 roty(double c, double s, V3 v) { return mk(c * v.x + s * v.z, v.y, -s * v.x + c * v.z); }

// Model constants of one leg.  The numbers come from include/qrw_solo12_model.h (the ONE data file):
// the kernel takes the FL leg of a compile-time copy of that initialiser as immediates and applies the mirror signs of
// the leg it works on; a static_assert proves that the other three legs of the data file ARE those mirror images, so
// a model file that breaks the symmetry cannot be compiled into a kernel that silently ignores it.
struct LegC {
  V3 haa, hfe, kfe, foot;
  double m[4];
  V3 com[4];
  double I[4][6];
};
constexpr qrw_solo12_model kModel = QRW_SOLO12_MODEL_INIT;
// sign of entry e of (com | inertia) of link `link` (0 shoulder, 1 upper, 2 lower, 3 foot) for mirror signs (sx, sy)
constexpr double mirror_sign(int link, bool inertia, int e, double sx, double sy) {
  if (!inertia) return (e == 0 && link == 0) ? sx : (e == 1 && link != 3) ? sy : 1.0;
  if (link == 0) return e == 1 ? sx * sy : 1.0;            // shoulder: ixy
  if (link == 1 || link == 2) return e == 4 ? sy : 1.0;    // upper / lower leg: iyz
  return 1.0;
}
constexpr bool same(double a, double b) { return a == b; }
constexpr bool link_is_mirror(const qrw_link_inertial& a, const qrw_link_inertial& fl, int link, double sx, double sy) {
  bool ok = same(a.mass, fl.mass);
  for (int e = 0; e < 3; e++) ok = ok && same(a.com[e], mirror_sign(link, false, e, sx, sy) * fl.com[e]);
  for (int e = 0; e < 6; e++) ok = ok && same(a.inertia[e], mirror_sign(link, true, e, sx, sy) * fl.inertia[e]);
  return ok;
}
constexpr bool leg_is_mirror(const qrw_leg_model& a, const qrw_leg_model& fl, double sx, double sy) {
  bool ok = same(a.haa_xyz[0], sx * fl.haa_xyz[0]) && same(a.haa_xyz[1], sy * fl.haa_xyz[1]) && same(a.haa_xyz[2], fl.haa_xyz[2]);
  const double* o[3] = {a.hfe_xyz, a.kfe_xyz, a.foot_xyz};
  const double* f[3] = {fl.hfe_xyz, fl.kfe_xyz, fl.foot_xyz};
  for (int i = 0; i < 3; i++) ok = ok && same(o[i][0], f[i][0]) && same(o[i][1], sy * f[i][1]) && same(o[i][2], f[i][2]);
  return ok && link_is_mirror(a.shoulder, fl.shoulder, 0, sx, sy) && link_is_mirror(a.upper, fl.upper, 1, sx, sy) &&
         link_is_mirror(a.lower, fl.lower, 2, sx, sy) && link_is_mirror(a.foot, fl.foot, 3, sx, sy);
}
static_assert(leg_is_mirror(kModel.leg[0], kModel.leg[0], 1.0, 1.0) && leg_is_mirror(kModel.leg[1], kModel.leg[0], 1.0, -1.0) &&
                  leg_is_mirror(kModel.leg[2], kModel.leg[0], -1.0, 1.0) && leg_is_mirror(kModel.leg[3], kModel.leg[0], -1.0, -1.0),
              "include/qrw_solo12_model.h: legs FR/HL/HR are not the mirror images of FL that the one-lane-per-leg kernels assume");

__device__ __forceinline__ LegC leg_consts(int j) {
  LegC L;
  const double sx = (j < 2) ? 1.0 : -1.0, sy = (j & 1) ? -1.0 : 1.0;
  constexpr qrw_leg_model FL = kModel.leg[0];
  L.haa = mk(sx * FL.haa_xyz[0], sy * FL.haa_xyz[1], FL.haa_xyz[2]);
  L.hfe = mk(FL.hfe_xyz[0], sy * FL.hfe_xyz[1], FL.hfe_xyz[2]);
  L.kfe = mk(FL.kfe_xyz[0], sy * FL.kfe_xyz[1], FL.kfe_xyz[2]);
  L.foot = mk(FL.foot_xyz[0], sy * FL.foot_xyz[1], FL.foot_xyz[2]);
  constexpr qrw_link_inertial LK[4] = {FL.shoulder, FL.upper, FL.lower, FL.foot};
#pragma unroll
  for (int l = 0; l < 4; l++) {
    L.m[l] = LK[l].mass;
    L.com[l] = mk(mirror_sign(l, false, 0, sx, sy) * LK[l].com[0], mirror_sign(l, false, 1, sx, sy) * LK[l].com[1], LK[l].com[2]);
#pragma unroll
    for (int e = 0; e < 6; e++) L.I[l][e] = mirror_sign(l, true, e, sx, sy) * LK[l].inertia[e];
  }
  return L;
}

struct LegKin {
  V3 p0, p1, p2, pf;  // joint origins and foot, base frame
  V3 a0, a1;          // joint axes (a2 = a1)
  M3 R0, R1, R2;      // link rotations (base <- link)
  V3 J0, J1, J2;      // columns of the foot Jacobian (base frame)
};

__device__ __forceinline__ LegKin leg_kinematics(const LegC& C, const double q[3]) {
  LegKin K;
  const double c0 = cos(q[0]), s0 = sin(q[0]);
  const double c1 = cos(q[1]), s1 = sin(q[1]);
  const double c12 = cos(q[1] + q[2]), s12 = sin(q[1] + q[2]);
  // R0 = Rx(q0); R1 = R0 Ry(q1); R2 = R0 Ry(q1 + q2)
  K.R0.r0 = mk(1, 0, 0); K.R0.r1 = mk(0, c0, -s0); K.R0.r2 = mk(0, s0, c0);
  K.R1.r0 = mk(c1, 0, s1); K.R1.r1 = mk(s0 * s1, c0, -s0 * c1); K.R1.r2 = mk(-c0 * s1, s0, c0 * c1);
  K.R2.r0 = mk(c12, 0, s12); K.R2.r1 = mk(s0 * s12, c0, -s0 * c12); K.R2.r2 = mk(-c0 * s12, s0, c0 * c12);
  K.p0 = C.haa;
  K.p1 = K.p0 + mul(K.R0, C.hfe);
  K.p2 = K.p1 + mul(K.R1, C.kfe);
  K.pf = K.p2 + mul(K.R2, C.foot);
  K.a0 = mk(1, 0, 0);
  K.a1 = mk(0, c0, s0);
  K.J0 = cross(K.a0, K.pf - K.p0);
  K.J1 = cross(K.a1, K.pf - K.p1);
  K.J2 = cross(K.a1, K.pf - K.p2);
  return K;
}

}  // namespace

}  // namespace qrw
