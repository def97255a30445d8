// The Kalman filter of the state estimator (KFilterBis, scripts/Estimator.py:88-181, and the Kalman branch of run_filter,
// :555-580) as plain C++ on doubles: no device intrinsics, so the same text is compiled into estimator_kernel.hip and into a
// stand-alone host program (tests/test_estimator_kalman_cpu.py), which is where this arithmetic is checked and debugged.
//
// State (18): base position (3), base velocity (3), the four foot positions (3 each).  Measurement (16): rows 3i+j the position
// of the IMU relative to foot i, rows 12+i the height of foot i (always 0).
//
// Two structural facts shape it (scripts/kalman_tolerance.py checks both against the dense form):
//  * the axes never couple.  A = I + dt [pos <- vel], H (:106-111), the diagonal Q and R (:167-181) and P0 = I touch, for axis j,
//    only the states {j, 3+j, 6+j, 9+j, 12+j, 15+j} and the measurements {j, 3+j, 6+j, 9+j} (and 12..15 for j = 2): the 18-state
//    filter is three 6-state filters (Axis below), and the cross-axis entries of the dense P stay exactly 0;
//  * R is diagonal, so the correction K = P H' inv(H P H' + R) (:163) is the measurements taken one at a time, each a scalar
//    division: s = h P h' + r, k = P h' / s, X += k (z - h X), P -= k (h P).  Every h has one or two nonzeros.
// P is kept as the full 6x6 block and is NOT symmetrised (the reference does not either, :165).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QRW_KF_FN __host__ __device__ __forceinline__
#define QRW_KF_UNROLL _Pragma("unroll")
#else
#define QRW_KF_FN inline
#define QRW_KF_UNROLL
#endif

namespace qrw {
namespace kf {

constexpr int kStates = 18, kMeas = 16, kAxisStates = 6;

// the tuning values (:133-137)
struct Tuning {
  double sigma_kin, sigma_h, sigma_a, sigma_dp, gamma;
};
QRW_KF_FN Tuning default_tuning() { return Tuning{0.1, 1.0, 0.1, 0.1, 30.0}; }

// ---- the exact index maps between an axis filter and the dense form
// local state k of axis j: 0 base position, 1 base velocity, 2 + i position of foot i
QRW_KF_FN int state_index(int axis, int k) { return k < 2 ? 3 * k + axis : 6 + 3 * (k - 2) + axis; }
QRW_KF_FN int kin_row(int axis, int foot) { return 3 * foot + axis; }  // measurement row of foot i on axis j (every axis)
QRW_KF_FN int height_row(int foot) { return 12 + foot; }               // ... of its height (axis 2 alone)

// updateCoeffs (:167-181): the diagonals of R and Q for one tick; neither is state
struct Coeffs {
  double r_kin[4], r_h[4];  // R on rows 3i..3i+2 and on row 12+i
  double q_foot[4], q_vel;  // Q on the states of foot i and on the velocity states (0 on the position states)
};
QRW_KF_FN Coeffs update_coeffs(const Tuning& t, double dt, const double status[4]) {
  Coeffs c;
  QRW_KF_UNROLL
  for (int i = 0; i < 4; i++) {
    const double trust = (status[i] == 0.0) ? 0.01 : 1.0;  // (:172-175)
    c.r_kin[i] = t.sigma_kin * t.sigma_kin / trust;
    c.r_h[i] = t.sigma_h * t.sigma_h / trust;
    c.q_foot[i] = t.sigma_dp * t.sigma_dp * (1.0 + exp(t.gamma * (0.5 - trust))) * (dt * dt);
  }
  c.q_vel = t.sigma_a * t.sigma_a * (dt * dt);
  return c;
}

// one axis: its 6 states and its 6x6 block of P, row-major
struct Axis {
  double x[kAxisStates];
  double p[kAxisStates * kAxisStates];
};

// the initial state (:121, :285): X = 0 but the base height, P = I
QRW_KF_FN void axis_init(Axis& a, double x0) {
  QRW_KF_UNROLL
  for (int k = 0; k < kAxisStates; k++) a.x[k] = 0.0;
  a.x[0] = x0;
  QRW_KF_UNROLL
  for (int k = 0; k < kAxisStates * kAxisStates; k++) a.p[k] = (k % (kAxisStates + 1) == 0) ? 1.0 : 0.0;
}

// predict (:152-157) with U = this axis' component of oRb IMU_lin_acc: X = A X + B U, P = A P A' + Q
QRW_KF_FN void predict(Axis& a, double dt, double u, const Coeffs& c) {
  const int n = kAxisStates;
  a.x[0] = (a.x[0] + dt * a.x[1]) + (0.5 * (dt * dt)) * u;
  a.x[1] = a.x[1] + dt * u;
  QRW_KF_UNROLL
  for (int k = 0; k < n; k++) a.p[k] += dt * a.p[n + k];  // A P: row 0 += dt row 1
  QRW_KF_UNROLL
  for (int k = 0; k < n; k++) a.p[n * k] += dt * a.p[n * k + 1];  // (A P) A': column 0 += dt column 1
  a.p[n * 1 + 1] += c.q_vel;
  QRW_KF_UNROLL
  for (int i = 0; i < 4; i++) a.p[n * (2 + i) + (2 + i)] += c.q_foot[i];
}

// correct (:159-165) for ONE measurement row z with noise r.  HEIGHT = false: a row 3i+j of H, +1 on the base position and -1
// on foot FOOT; HEIGHT = true: a row 12+i, +1 on foot FOOT.
template <int FOOT, bool HEIGHT>
QRW_KF_FN void scalar_update(Axis& a, double z, double r) {
  const int n = kAxisStates, f = 2 + FOOT;
  double pht[kAxisStates], hp[kAxisStates];  // P h' and h P (P is not symmetrised: they may differ in the last bits)
  QRW_KF_UNROLL
  for (int k = 0; k < n; k++) {
    pht[k] = HEIGHT ? a.p[n * k + f] : a.p[n * k] - a.p[n * k + f];
    hp[k] = HEIGHT ? a.p[n * f + k] : a.p[k] - a.p[n * f + k];
  }
  const double s = (HEIGHT ? pht[f] : pht[0] - pht[f]) + r;
  const double innov = z - (HEIGHT ? a.x[f] : a.x[0] - a.x[f]);
  double gain[kAxisStates];
  QRW_KF_UNROLL
  for (int k = 0; k < n; k++) gain[k] = pht[k] / s;
  QRW_KF_UNROLL
  for (int k = 0; k < n; k++) a.x[k] += gain[k] * innov;
  QRW_KF_UNROLL
  for (int k = 0; k < n; k++) {
    QRW_KF_UNROLL
    for (int l = 0; l < n; l++) a.p[n * k + l] -= gain[k] * hp[l];
  }
}

// One tick of one axis: predict, then the four kinematic rows of this axis (z_kin[i] = Z[3i+j]) and, on axis 2, the four height
// rows (Z[12+i] = 0, :570).
QRW_KF_FN void axis_step(Axis& a, bool height_rows, double dt, double u, const double z_kin[4], const Coeffs& c) {
  predict(a, dt, u, c);
  scalar_update<0, false>(a, z_kin[0], c.r_kin[0]);
  scalar_update<1, false>(a, z_kin[1], c.r_kin[1]);
  scalar_update<2, false>(a, z_kin[2], c.r_kin[2]);
  scalar_update<3, false>(a, z_kin[3], c.r_kin[3]);
  if (height_rows) {
    scalar_update<0, true>(a, 0.0, c.r_h[0]);
    scalar_update<1, true>(a, 0.0, c.r_h[1]);
    scalar_update<2, true>(a, 0.0, c.r_h[2]);
    scalar_update<3, true>(a, 0.0, c.r_h[3]);
  }
}

// ---- assembly of the results (:578-580).  The IMU's offset in the base frame (_1Mi.translation, :323-324):
QRW_KF_FN double imu_offset(int axis) { return axis == 0 ? 0.1163 : axis == 1 ? 0.0 : 0.02; }
// filt_lin_pos[j] = X[j] - offset[j]: the offset is NOT rotated (:579)
QRW_KF_FN double base_position(int axis, double x_pos) { return x_pos - imu_offset(axis); }
// filt_lin_vel = oRb' (X[3:6] - cross3(offset, IMU_ang_vel)) (:580); oRb row-major
QRW_KF_FN void base_velocity(const double oRb[9], const double x_vel[3], const double gyro[3], double out[3]) {
  const double ox = imu_offset(0), oy = imu_offset(1), oz = imu_offset(2);
  const double cx = oy * gyro[2] - oz * gyro[1];
  const double cy = oz * gyro[0] - ox * gyro[2];
  const double cz = ox * gyro[1] - oy * gyro[0];
  const double d[3] = {x_vel[0] - cx, x_vel[1] - cy, x_vel[2] - cz};
  QRW_KF_UNROLL
  for (int k = 0; k < 3; k++) out[k] = oRb[k] * d[0] + oRb[3 + k] * d[1] + oRb[6 + k] * d[2];
}

// ---- the whole filter on the dense layouts (X[18], the three P blocks, Z[16]): what the host program runs, and the order of
// operations of the kernel, where each axis is one lane
struct Filter {
  Axis axis[3];
};
QRW_KF_FN void filter_init(Filter& f, double h_init) {
  axis_init(f.axis[0], 0.0);
  axis_init(f.axis[1], 0.0);
  axis_init(f.axis[2], h_init);
}
QRW_KF_FN void filter_step(Filter& f, const Tuning& t, double dt, const double u[3], const double z[kMeas], const double status[4]) {
  const Coeffs c = update_coeffs(t, dt, status);
  for (int j = 0; j < 3; j++) {
    const double zk[4] = {z[kin_row(j, 0)], z[kin_row(j, 1)], z[kin_row(j, 2)], z[kin_row(j, 3)]};
    axis_step(f.axis[j], j == 2, dt, u[j], zk, c);
  }
}
QRW_KF_FN void filter_state(const Filter& f, double X[kStates]) {
  for (int j = 0; j < 3; j++)
    for (int k = 0; k < kAxisStates; k++) X[state_index(j, k)] = f.axis[j].x[k];
}
// dense P (row-major 18x18) from the blocks, exact zeros elsewhere
QRW_KF_FN void filter_covariance(const Filter& f, double P[kStates * kStates]) {
  for (int k = 0; k < kStates * kStates; k++) P[k] = 0.0;
  for (int j = 0; j < 3; j++)
    for (int k = 0; k < kAxisStates; k++)
      for (int l = 0; l < kAxisStates; l++) P[kStates * state_index(j, k) + state_index(j, l)] = f.axis[j].p[kAxisStates * k + l];
}

}  // namespace kf
}  // namespace qrw
