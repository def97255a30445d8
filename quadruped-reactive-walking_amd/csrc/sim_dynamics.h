// Forward dynamics of one Solo12 with penalty contact, one lane per leg (sim_kernel.hip).
//
// Everything is written in ONE coordinate system, the base frame with the base origin as the reference point of every
// spatial quantity (Featherstone's spatial algebra holds in any frame, a moving one too), so no transform between link
// frames is needed: a body's inertia is (mass, first moment, rotational inertia about the base origin), a joint's motion
// subspace is (p x a, a) for the axis a through the point p.  Conventions are the oracle's (oracle/rbd_oracle.c, Pinocchio's):
// motions (linear, angular), forces (force, moment), the free-flyer's velocity and acceleration in the base frame,
// gravity as the base's spatial acceleration R'(0, 0, +g).
//
// M(q) of this tree is [Mbb F; F' H] with H block diagonal (one 3x3 block per leg), so the 18x18 solve is, per leg, its
// block's inverse and a Schur complement onto the base's 6x6; the four legs' contributions are summed by the caller
// (DPP quad sums on the device).
#pragma once
#include "sim_terrain.h"
#include "solo12_leg.h"

namespace qrw {

namespace {

struct SV {  // spatial motion (lin, ang) or force (force, moment)
  V3 l, a;
};
__device__ __forceinline__ SV operator+(SV x, SV y) { SV r; r.l = x.l + y.l; r.a = x.a + y.a; return r; }
__device__ __forceinline__ SV operator*(double s, SV x) { SV r; r.l = s * x.l; r.a = s * x.a; return r; }
__device__ __forceinline__ double sdot(SV m, SV f) { return dot(m.l, f.l) + dot(m.a, f.a); }
// v x m (motion with motion) and v x* f (motion with force), oracle/rbd_oracle.c motion_cross / force_cross
__device__ __forceinline__ SV mcross(SV v, SV m) { SV r; r.a = cross(v.a, m.a); r.l = cross(v.a, m.l) + cross(v.l, m.a); return r; }
__device__ __forceinline__ SV fcross(SV v, SV f) { SV r; r.l = cross(v.a, f.l); r.a = cross(v.a, f.a) + cross(v.l, f.l); return r; }

// rigid-body inertia about the base origin, base axes: mass, first moment m c, rotational inertia (xx xy xz yy yz zz)
struct RB {
  double m;
  V3 h;
  double I[6];
};
__device__ __forceinline__ RB operator+(const RB& x, const RB& y) {
  RB r;
  r.m = x.m + y.m;
  r.h = x.h + y.h;
#pragma unroll
  for (int e = 0; e < 6; e++) r.I[e] = x.I[e] + y.I[e];
  return r;
}
// a link's inertial (mass, CoM `com` and inertia I about it, both in link axes) carried by the link frame (R, p)
__device__ __forceinline__ RB rb_of(double m, V3 com, const double I[6], const M3& R, V3 p) {
  RB b;
  const V3 c = p + mul(R, com);
  b.m = m;
  b.h = m * c;
  // R I R': rows of A = R I, then A R'
  const V3 i0 = mk(I[0], I[1], I[2]), i1 = mk(I[1], I[3], I[4]), i2 = mk(I[2], I[4], I[5]);
  const V3 A0 = mk(dot(R.r0, i0), dot(R.r0, i1), dot(R.r0, i2));
  const V3 A1 = mk(dot(R.r1, i0), dot(R.r1, i1), dot(R.r1, i2));
  const V3 A2 = mk(dot(R.r2, i0), dot(R.r2, i1), dot(R.r2, i2));
  const double n2 = dot(c, c);
  b.I[0] = dot(A0, R.r0) + m * (n2 - c.x * c.x);
  b.I[1] = dot(A0, R.r1) - m * c.x * c.y;
  b.I[2] = dot(A0, R.r2) - m * c.x * c.z;
  b.I[3] = dot(A1, R.r1) + m * (n2 - c.y * c.y);
  b.I[4] = dot(A1, R.r2) - m * c.y * c.z;
  b.I[5] = dot(A2, R.r2) + m * (n2 - c.z * c.z);
  return b;
}
// force = m v + w x h, moment = I w + h x v
__device__ __forceinline__ SV rb_apply(const RB& b, SV v) {
  SV f;
  f.l = b.m * v.l + cross(v.a, b.h);
  f.a = mk(b.I[0] * v.a.x + b.I[1] * v.a.y + b.I[2] * v.a.z, b.I[1] * v.a.x + b.I[3] * v.a.y + b.I[4] * v.a.z,
           b.I[2] * v.a.x + b.I[4] * v.a.y + b.I[5] * v.a.z) + cross(b.h, v.l);
  return f;
}
// I a + v x* (I v)
__device__ __forceinline__ SV rb_force(const RB& b, SV v, SV a) { return rb_apply(b, a) + fcross(v, rb_apply(b, v)); }

__device__ __forceinline__ M3 sim_quat_to_rot(double x, double y, double z, double w) {  // Eigen's toRotationMatrix, rows
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  M3 R;
  R.r0 = mk(1.0 - (tyy + tzz), txy - twz, txz + twy);
  R.r1 = mk(txy + twz, 1.0 - (txx + tzz), tyz - twx);
  R.r2 = mk(txz - twy, tyz + twx, 1.0 - (txx + tyy));
  return R;
}

struct SimContact {
  double kn, dn, mu, vs, foot_radius;
};

// The ground of the terrain instantiation: one heightfield for the whole batch (sim_terrain.h) and this robot's offset into it
// (the foot at world (x, y) is looked up at (x + ox, y + oy); zero when the caller gave no origins).
struct SimGround {
  terrain::Field T;
  double ox, oy;
};

// Contact of one foot (centre at height z_foot, world velocity v) with the triangle's plane s under it: with the unit normal
// n = (-gx, -gy, 1)/|.|, d = foot_radius - n_z (z_foot - h) is how far the foot's sphere reaches through the plane, the normal
// force kn d - dn (n.v) clipped at 0 while d > 0, regularised Coulomb friction against the tangential velocity v - (n.v) n.
// For a field of zeros this is the plane z = 0's formula term by term (n = (-0, -0, 1)).
__device__ __forceinline__ V3 sim_terrain_force(const terrain::Plane& s, double z_foot, V3 v, const SimContact& cp) {
  const double in = 1.0 / sqrt(s.gx * s.gx + s.gy * s.gy + 1.0);
  const V3 n = mk(-s.gx * in, -s.gy * in, in);
  const double d = cp.foot_radius - n.z * (z_foot - s.h);
  const double vn = dot(n, v);
  double fn = 0.0;
  if (d > 0.0) fn = fmax(0.0, cp.kn * d - cp.dn * vn);
  const V3 vt = v - vn * n;
  const double kt = -cp.mu * fn / sqrt(dot(vt, vt) + cp.vs * cp.vs);
  return fn * n + kt * vt;
}

// What one leg adds to the base's 6x6 system, and what it keeps to recover its own joint accelerations.
struct LegPart {
  double S[21];    // upper triangle (row-major) of: the leg's composite inertia minus F H^-1 F'
  double r[6];     // contact wrench of the foot minus the leg's bias wrench minus F H^-1 (joint right-hand side)
  SV F[3];         // columns of the coupling block
  double Hi[6];    // H^-1 (xx xy xz yy yz zz)
  double rj[3];    // joint right-hand side: tau + J'f - bias
  V3 f_world;      // contact force on the foot, world frame
};

// One leg at (q3, dq3) under the torques tau3, hanging from a base with rotation R (world <- base), height of its origin pz
// and velocity (vb, wb) in the base frame.  kTerrain: the ground is the heightfield g under the base at (px, py) instead of the
// plane z = 0 (px, py and g are not read otherwise).
template <bool kTerrain>
__device__ __forceinline__ LegPart sim_leg_part(int j, const double q3[3], const double dq3[3], const double tau3[3], const M3& R,
                                                double px, double py, double pz, V3 vb, V3 wb, const SimContact& cp, const SimGround& g) {
  LegPart P;
  const LegC C = leg_consts(j);
  const LegKin K = leg_kinematics(C, q3);
  // ---- contact: penalty normal force on the plane z = 0 (or the heightfield), regularised Coulomb friction
  const V3 v_foot_b = vb + cross(wb, K.pf) + dq3[0] * K.J0 + dq3[1] * K.J1 + dq3[2] * K.J2;
  const V3 v_foot = mul(R, v_foot_b);
  const double z_foot = pz + dot(R.r2, K.pf);
  terrain::Axis cu, cv;
  terrain::Corners hc;
  V3 fb;  // the contact force in the base frame
  if constexpr (kTerrain) {
    // the cell under the foot and its four heights (two 16-byte loads): the tick's only new memory traffic, asked for here, as soon
    // as the foot's position is known; the force is formed after the bodies and the bias pass.  (How much of that arithmetic the
    // compiler really leaves between the loads and their wait, at 256 VGPRs, is recorded in DESIGN.md 4.7.)
    cu = terrain::axis_cell(px + dot(R.r0, K.pf) + g.ox, g.T.x0, g.T.dx, g.T.cols);
    cv = terrain::axis_cell(py + dot(R.r1, K.pf) + g.oy, g.T.y0, g.T.dy, g.T.rows);
    hc = terrain::load_corners(g.T, cv.i, cu.i);
    __builtin_amdgcn_sched_barrier(0);  // (keeps the loads here, ahead of what follows; without it: 212 AGPRs and 6 spilled registers)
  } else {
    const double d = cp.foot_radius - z_foot;
    double fn = 0.0;
    if (d > 0.0) fn = fmax(0.0, cp.kn * d - cp.dn * v_foot.z);
    const double kt = -cp.mu * fn / sqrt(v_foot.x * v_foot.x + v_foot.y * v_foot.y + cp.vs * cp.vs);
    P.f_world = mk(kt * v_foot.x, kt * v_foot.y, fn);
    fb = mulT(R, P.f_world);
  }
  // ---- bodies and joints
  const RB b0 = rb_of(C.m[0], C.com[0], C.I[0], K.R0, K.p0);
  const RB b1 = rb_of(C.m[1], C.com[1], C.I[1], K.R1, K.p1);
  const RB b2 = rb_of(C.m[2], C.com[2], C.I[2], K.R2, K.p2) + rb_of(C.m[3], C.foot + C.com[3], C.I[3], K.R2, K.p2);
  SV S0, S1, S2;
  S0.l = cross(K.p0, K.a0); S0.a = K.a0;
  S1.l = cross(K.p1, K.a1); S1.a = K.a1;
  S2.l = cross(K.p2, K.a1); S2.a = K.a1;
  // ---- bias: rnea(q, v, 0) of this leg, gravity included
  SV v0, a0;
  v0.l = vb; v0.a = wb;
  a0.l = mulT(R, mk(0.0, 0.0, kModel.gravity)); a0.a = mk(0.0, 0.0, 0.0);
  const SV vj0 = dq3[0] * S0, vj1 = dq3[1] * S1, vj2 = dq3[2] * S2;
  const SV v1 = v0 + vj0, a1 = a0 + mcross(v1, vj0);
  const SV v2 = v1 + vj1, a2 = a1 + mcross(v2, vj1);
  const SV v3 = v2 + vj2, a3 = a2 + mcross(v3, vj2);
  const SV f3 = rb_force(b2, v3, a3);
  const SV f2 = rb_force(b1, v2, a2) + f3;
  const SV f1 = rb_force(b0, v1, a1) + f2;
  if constexpr (kTerrain) {
    __builtin_amdgcn_sched_barrier(0);
    P.f_world = sim_terrain_force(terrain::plane_of(hc, cu.f, cv.f, g.T.dx, g.T.dy), z_foot, v_foot, cp);
    fb = mulT(R, P.f_world);
  }
  // ---- right-hand sides
  P.rj[0] = tau3[0] + dot(K.J0, fb) - sdot(S0, f1);
  P.rj[1] = tau3[1] + dot(K.J1, fb) - sdot(S1, f2);
  P.rj[2] = tau3[2] + dot(K.J2, fb) - sdot(S2, f3);
  const V3 mb = cross(K.pf, fb);
  double w6[6] = {fb.x - f1.l.x, fb.y - f1.l.y, fb.z - f1.l.z, mb.x - f1.a.x, mb.y - f1.a.y, mb.z - f1.a.z};
  // ---- composite inertias, coupling block F and the leg's own block H
  const RB c1 = b1 + b2, c0 = b0 + c1;
  P.F[0] = rb_apply(c0, S0);
  P.F[1] = rb_apply(c1, S1);
  P.F[2] = rb_apply(b2, S2);
  const double h00 = sdot(S0, P.F[0]), h01 = sdot(S0, P.F[1]), h02 = sdot(S0, P.F[2]);
  const double h11 = sdot(S1, P.F[1]), h12 = sdot(S1, P.F[2]), h22 = sdot(S2, P.F[2]);
  {  // inverse of the symmetric 3x3 by cofactors
    const double c00 = h11 * h22 - h12 * h12, c01 = h02 * h12 - h01 * h22, c02 = h01 * h12 - h02 * h11;
    const double id = 1.0 / (h00 * c00 + h01 * c01 + h02 * c02);
    P.Hi[0] = c00 * id; P.Hi[1] = c01 * id; P.Hi[2] = c02 * id;
    P.Hi[3] = (h00 * h22 - h02 * h02) * id; P.Hi[4] = (h01 * h02 - h00 * h12) * id; P.Hi[5] = (h00 * h11 - h01 * h01) * id;
  }
  // G = F H^-1 (6x3), row i = (F[0][i], F[1][i], F[2][i]) H^-1
  double Fm[6][3], G[6][3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    Fm[0][k] = P.F[k].l.x; Fm[1][k] = P.F[k].l.y; Fm[2][k] = P.F[k].l.z;
    Fm[3][k] = P.F[k].a.x; Fm[4][k] = P.F[k].a.y; Fm[5][k] = P.F[k].a.z;
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    G[i][0] = Fm[i][0] * P.Hi[0] + Fm[i][1] * P.Hi[1] + Fm[i][2] * P.Hi[2];
    G[i][1] = Fm[i][0] * P.Hi[1] + Fm[i][1] * P.Hi[3] + Fm[i][2] * P.Hi[4];
    G[i][2] = Fm[i][0] * P.Hi[2] + Fm[i][1] * P.Hi[4] + Fm[i][2] * P.Hi[5];
  }
  // the leg's composite inertia as a 6x6: [m E, -[h]x; [h]x, I]
  const double m = c0.m;
  const V3 h = c0.h;
  const double Mc[21] = {m,   0.0, 0.0, 0.0,  h.z,  -h.y,      //
                         m,   0.0, -h.z, 0.0,  h.x,            //
                         m,   h.y, -h.x, 0.0,                  //
                         c0.I[0], c0.I[1], c0.I[2],            //
                         c0.I[3], c0.I[4],                     //
                         c0.I[5]};
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int k = i; k < 6; k++, e++) P.S[e] = Mc[e] - (G[i][0] * Fm[k][0] + G[i][1] * Fm[k][1] + G[i][2] * Fm[k][2]);
    P.r[i] = w6[i] - (G[i][0] * P.rj[0] + G[i][1] * P.rj[1] + G[i][2] * P.rj[2]);
  }
  return P;
}

// The base body's own share: its inertia into S, its bias wrench and the external wrench (world frame, at the base origin;
// fe = me = 0 for none) into r.  S and r arrive holding the sum over the four legs.
__device__ __forceinline__ void sim_base_part(const M3& R, V3 vb, V3 wb, V3 fe, V3 me, double S[21], double r[6]) {
  constexpr qrw_link_inertial BL = kModel.base;
  const double Ib[6] = {BL.inertia[0], BL.inertia[1], BL.inertia[2], BL.inertia[3], BL.inertia[4], BL.inertia[5]};
  M3 Id;
  Id.r0 = mk(1, 0, 0); Id.r1 = mk(0, 1, 0); Id.r2 = mk(0, 0, 1);
  const RB b = rb_of(BL.mass, mk(BL.com[0], BL.com[1], BL.com[2]), Ib, Id, mk(0.0, 0.0, 0.0));
  SV v0, a0;
  v0.l = vb; v0.a = wb;
  a0.l = mulT(R, mk(0.0, 0.0, kModel.gravity)); a0.a = mk(0.0, 0.0, 0.0);
  const SV f0 = rb_force(b, v0, a0);
  const V3 feb = mulT(R, fe), meb = mulT(R, me);
  r[0] += feb.x - f0.l.x; r[1] += feb.y - f0.l.y; r[2] += feb.z - f0.l.z;
  r[3] += meb.x - f0.a.x; r[4] += meb.y - f0.a.y; r[5] += meb.z - f0.a.z;
  S[0] += b.m; S[6] += b.m; S[11] += b.m;
  S[4] += b.h.z; S[5] -= b.h.y; S[8] -= b.h.z; S[10] += b.h.x; S[12] += b.h.y; S[13] -= b.h.x;
  S[15] += b.I[0]; S[16] += b.I[1]; S[17] += b.I[2]; S[18] += b.I[3]; S[19] += b.I[4]; S[20] += b.I[5];
}

// S x = r for the symmetric positive definite 6x6 whose upper triangle is S: elimination without pivoting
__device__ __forceinline__ void sim_solve6(const double S[21], const double r[6], double x[6]) {
  double A[6][6], b[6];
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    b[i] = r[i];
#pragma unroll
    for (int k = i; k < 6; k++, e++) A[i][k] = A[k][i] = S[e];
  }
#pragma unroll
  for (int p = 0; p < 6; p++) {
    const double ip = 1.0 / A[p][p];
#pragma unroll
    for (int i = p + 1; i < 6; i++) {
      const double l = A[i][p] * ip;
#pragma unroll
      for (int k = p + 1; k < 6; k++) A[i][k] -= l * A[p][k];
      b[i] -= l * b[p];
    }
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) s -= A[i][k] * x[k];
    x[i] = s / A[i][i];
  }
}

// the leg's joint accelerations once the base's are known: H^-1 (rj - F' ab)
__device__ __forceinline__ void sim_leg_ddq(const LegPart& P, const double ab[6], double ddq[3]) {
  SV a;
  a.l = mk(ab[0], ab[1], ab[2]); a.a = mk(ab[3], ab[4], ab[5]);
  const double t0 = P.rj[0] - sdot(a, P.F[0]), t1 = P.rj[1] - sdot(a, P.F[1]), t2 = P.rj[2] - sdot(a, P.F[2]);
  ddq[0] = P.Hi[0] * t0 + P.Hi[1] * t1 + P.Hi[2] * t2;
  ddq[1] = P.Hi[1] * t0 + P.Hi[3] * t1 + P.Hi[4] * t2;
  ddq[2] = P.Hi[2] * t0 + P.Hi[4] * t1 + P.Hi[5] * t2;
}

// quat <- normalise(quat (x) exp(w h)), xyzw
__device__ __forceinline__ void sim_quat_step(double q[4], V3 w, double h) {
  const V3 r = h * w;
  const double th = sqrt(dot(r, r));
  const double k = (th < 1e-8) ? 0.5 : sin(0.5 * th) / th;
  const double bx = k * r.x, by = k * r.y, bz = k * r.z, bw = cos(0.5 * th);
  const double ax = q[0], ay = q[1], az = q[2], aw = q[3];
  const double x = aw * bx + ax * bw + ay * bz - az * by;
  const double y = aw * by - ax * bz + ay * bw + az * bx;
  const double z = aw * bz + ax * by - ay * bx + az * bw;
  const double s = aw * bw - ax * bx - ay * by - az * bz;
  const double n = sqrt(x * x + y * y + z * z + s * s);
  q[0] = x / n; q[1] = y / n; q[2] = z / n; q[3] = s / n;
}

}  // namespace

}  // namespace qrw
