// State estimator for a batch of Solo12 instances — gfx950 (MI355X): sensors in, filtered state out.
//
// Replaces, per instance, Estimator.run_filter (scripts/Estimator.py:466-629) with the complementary filters
// (kf_enabled = False, the reference's default, scripts/Controller.py:110-111) and what it calls:
//   get_data_IMU                 scripts/Estimator.py:347-373  (quaternionToRPY :686-714, EulerToQuaternion :672-684)
//   get_data_joints              :375-385
//   get_data_FK                  :387-445  (BaseVelocityFromKinAndIMU :642-670)
//   get_xyz_feet                 :447-464
//   ComplementaryFilter.compute  :205-231
// Its four results q_filt, v_filt, RPY and v_secu are what Controller.compute reads first on every iteration
// (scripts/Controller.py:213, :344-351, :397-408), i.e. the inputs of qrw_control_pre / qrw_iteration_step.
//
// Mapping: lane = 4*instance_in_wave + leg (FL, FR, HL, HR), ONE QUAD PER ROBOT INSTANCE, 16 instances per wavefront -- the
// mapping of wbc_kernel.  Each lane runs the kinematics of its own leg (solo12_leg.h, shared with wbc_kernel.hip) and the
// velocity of its foot; the sums over the feet in contact go through DPP quad permutes (quad_sum).  The per-robot part (IMU
// attitude, the two filters) is a few dozen flops and is evaluated by all four lanes alike, which then share the stores.  No
// LDS, no scratch.  The persistent state is item-major ([item][B]) so that a wavefront's loads of one item coalesce.
//
// Kinematics: Pinocchio's forwardKinematics / getFrameVelocity on a base at the origin are the closed-form leg_kinematics and
// J dq here; the test checker goes through the oracle's rigid-body code instead (oracle.fixed_feet).
//
// The one departure: `remaining_steps` (:476-479) indexes past the gait matrix and raises IndexError when every row equals
// row 0; here the scan stops at N_gait.  Only an all-swing row 0 can do that (the unused rows of a gait matrix are zero rows),
// which no gait of the planners produces.
//
// The Kalman variant (KFilterBis, kf_enabled = True, :88-181 and :555-580) is the second instantiation of the kernel: only the
// block that replaces :519-553 differs.  Its arithmetic is kalman_filter.h (plain C++, also built for the host); here lanes 0, 1
// and 2 of the quad each own one axis of the filter -- 6 states and a 6x6 block of P in registers, the three axes never couple --
// and fetch their component of the four legs' measurement rows by quad permutes; lane 3 runs the z axis along with lane 2 and
// stores nothing of it.  The z lanes take 8 scalar updates where x and y take 4: the kernel is launch-latency bound, it is not
// balanced.  State of the filter: ks[item][B] (KalStateItem).  A robot whose readings are not finite keeps a non-finite filter
// from then on, as in the reference; no permute leaves its quad.
//
// Out of scope: KFilter (the 6-state class nothing constructs), the logging arrays and plot_graphs.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "kalman_filter.h"
#include "solo12_leg.h"
#include "qrw_device.h"
#include "qrw_kernels.h"

namespace qrw {

namespace {

__device__ __forceinline__ V3 quad_sum3(V3 v) { return mk(quad_sum(v.x), quad_sum(v.y), quad_sum(v.z)); }
__device__ __forceinline__ double quad_min(double v) {
  v = fmin(v, dpp_quad<0xB1>(v));
  v = fmin(v, dpp_quad<0x4E>(v));
  return v;
}
__device__ __forceinline__ double pick(V3 v, int j) { return j == 0 ? v.x : j == 1 ? v.y : v.z; }

// quaternionToRPY (scripts/Estimator.py:686-714), guards and clamp included.  The guards compare with exactly 0 and +-1, so the
// products and sums are rounded one by one as numpy rounds them (no fused multiply-add here).
__device__ __forceinline__ V3 quaternion_to_rpy(double qx, double qy, double qz, double qw) {
#pragma clang fp contract(off)
  const double xa0 = 2.0 * (qy * qz + qw * qx);
  const double xa1 = qw * qw - qx * qx - qy * qy + qz * qz;
  double rx = 0.0;
  if (xa0 != 0.0 && xa1 != 0.0) rx = atan2(xa0, xa1);
  const double ya0 = -2.0 * (qx * qz - qw * qy);
  double ry;
  if (ya0 >= 1.0) ry = M_PI / 2.0;
  else if (ya0 <= -1.0) ry = -M_PI / 2.0;
  else ry = asin(ya0);
  const double za0 = 2.0 * (qx * qy + qw * qz);
  const double za1 = qw * qw + qx * qx - qy * qy - qz * qz;
  double rz = 0.0;
  if (za0 != 0.0 && za1 != 0.0) rz = atan2(za0, za1);
  return mk(rx, ry, rz);
}

// pin.Quaternion(x, y, z, w).toRotationMatrix() (scripts/Estimator.py:522), rows
__device__ __forceinline__ M3 quat_to_rot(double x, double y, double z, double w) {
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  M3 R;
  R.r0 = mk(1.0 - (tyy + tzz), txy - twz, txz + twy);
  R.r1 = mk(txy + twz, 1.0 - (txx + tzz), tyz - twx);
  R.r2 = mk(txz - twy, tyz + twx, 1.0 - (txx + tyy));
  return R;
}

static_assert(kKsP - kKsX == kf::kStates && kKsZ - kKsP == 3 * kf::kAxisStates * kf::kAxisStates && kKalStItems - kKsZ == kf::kMeas,
              "KalStateItem is X, the three blocks of P, Z");

struct ES {  // accessor of one instance's estimator state (item-major)
  double* base;
  size_t stride;  // = batch
  __device__ __forceinline__ double& operator()(int item) const { return base[(size_t)item * stride]; }
  __device__ __forceinline__ V3 v3(int item) const { return mk((*this)(item), (*this)(item + 1), (*this)(item + 2)); }
};

}  // namespace

// Estimator.__init__ (scripts/Estimator.py:245-342): everything zero but FK_xyz[2] = filter_xyz_pos.LP_x[2] = h_init (:279-283)
__global__ __launch_bounds__(64) void estimator_init_kernel(EstimatorArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const ES s{a.es + b, (size_t)a.B};
  for (int i = 0; i < kEstStItems; i++) s(i) = 0.0;
  s(kEsFkXyz + 2) = a.h_init;
  if (!a.kalman) {
    s(kEsLPp + 2) = a.h_init;
    return;
  }
  // kf_enabled (:284-285, :121): the height goes into X[2] instead, P = I; Z starts at zero (:301)
  const ES k{a.ks + b, (size_t)a.B};
  for (int i = 0; i < kKalStItems; i++) k(i) = 0.0;
  k(kKsX + 2) = a.h_init;
  for (int i = 0; i < 3 * 6; i++) k(kKsP + 36 * (i / 6) + 7 * (i % 6)) = 1.0;  // the diagonals of the three 6x6 blocks
}

template <bool KALMAN>
__global__ __launch_bounds__(64) void estimator_kernel(EstimatorArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  const int b = t >> 2, j = t & 3;
  if (b >= a.B) return;  // (whole quads leave together: the quad permutes below never read a lane that left)
  const size_t B = (size_t)a.B;
  const ES s{a.es + b, B};

  // ---- feet_status = gait[0, :], remaining_steps = first row that differs from row 0 (:476-479); this lane holds column j
  double status, first;
  if (a.gait) {
    const double* g = a.gait + (size_t)b * a.N_gait * 4 + j;
    status = g[0];
    int f = a.N_gait;
    for (int i = a.N_gait - 1; i >= 1; i--)
      if (g[4 * i] != status) f = i;
    first = (double)f;
  } else {  // the planner's current gait: four 64-bit column masks, bit i = row i (planner_kernel.hip)
    const unsigned long long c = (unsigned long long)__double_as_longlong(a.ps[(size_t)(a.ps_cur + j) * B + b]);
    status = (c & 1ull) ? 1.0 : 0.0;
    const unsigned long long rows = (a.N_gait >= 64) ? ~0ull : ((1ull << a.N_gait) - 1ull);
    const unsigned long long d = ((c & 1ull) ? ~c : c) & rows & ~1ull;
    first = d ? (double)__builtin_ctzll(d) : (double)a.N_gait;
  }
  const double remaining_steps = quad_min(first);

  // ---- get_data_IMU (:347-373)
  const V3 acc = mk(a.lin_acc[(size_t)b * 3], a.lin_acc[(size_t)b * 3 + 1], a.lin_acc[(size_t)b * 3 + 2]);
  const V3 gyro = mk(a.ang_vel[(size_t)b * 3], a.ang_vel[(size_t)b * 3 + 1], a.ang_vel[(size_t)b * 3 + 2]);
  const double* qi = a.quat + (size_t)b * 4;
  V3 rpy = quaternion_to_rpy(qi[0], qi[1], qi[2], qi[3]);
  const double k_log = s(kEsKlog);
  double yaw_off = s(kEsYawOff);
  if (k_log <= 1.0) yaw_off = rpy.z;  // (:363-364: the first TWO calls latch)
  rpy.z -= yaw_off;
  double qx, qy, qz, qw;
  {  // EulerToQuaternion (:672-684)
    const double sr = sin(rpy.x / 2.), cr = cos(rpy.x / 2.), sp = sin(rpy.y / 2.), cp = cos(rpy.y / 2.);
    const double sy = sin(rpy.z / 2.), cy = cos(rpy.z / 2.);
    qx = sr * cp * cy - cr * sp * sy;
    qy = cr * sp * cy + sr * cp * sy;
    qz = cr * cp * sy - sr * sp * cy;
    qw = cr * cp * cy + sr * sp * sy;
  }
  const M3 oRb = quat_to_rot(qx, qy, qz, qw);

  // ---- get_data_joints (:375-385): this lane's leg
  double q3[3], dq3[3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    q3[i] = a.q_mes[(size_t)b * 12 + 3 * j + i];
    dq3[i] = a.v_mes[(size_t)b * 12 + 3 * j + i];
  }

  // ---- k_since_contact (:494-495), BEFORE the forward kinematics
  double ksc = s(kEsKsc + j);
  ksc += status;
  ksc *= status;

  // ---- get_data_FK (:387-445)
  const LegC C = leg_consts(j);
  const LegKin K = leg_kinematics(C, q3);
  const V3 v_foot = dq3[0] * K.J0 + dq3[1] * K.J1 + dq3[2] * K.J2;  // foot velocity, base at the origin with identity orientation
  V3 vel = cross(K.pf, gyro) - v_foot;                               // BaseVelocityFromKinAndIMU (:664-665)
  const V3 xyz = -1.0 * mul(oRb, K.pf);                              // -framePlacement.translation with the IMU orientation (:407-423)
  const double r_foot = 0.025;                                       // (:434-438)
  vel.x += r_foot * ((j <= 1) ? (dq3[1] - dq3[2]) : (dq3[1] + dq3[2]));
  const bool in_contact = status == 1.0;
  const bool use = in_contact && ksc >= 16.0;  // (:414-415)
  const double cpt = quad_sum(use ? 1.0 : 0.0);
  const V3 zero = mk(0.0, 0.0, 0.0);
  const V3 vel_est = quad_sum3(use ? vel : zero), xyz_est = quad_sum3(use ? xyz : zero);
  V3 fk_vel = s.v3(kEsFkVel), fk_xyz = s.v3(kEsFkXyz);
  if (cpt > 0.0) {  // (:441-443: kept otherwise)
    fk_vel = mk(vel_est.x / cpt, vel_est.y / cpt, vel_est.z / cpt);
    fk_xyz = mk(xyz_est.x / cpt, xyz_est.y / cpt, xyz_est.z / cpt);
  }

  // ---- get_xyz_feet (:447-464)
  V3 goal;
  if (a.goals) {
    const double* g = a.goals + (size_t)b * 12 + j;
    goal = mk(g[0], g[4], g[8]);
  } else {  // FootTrajectoryGenerator::getFootPosition of the handle's planner
    const double* g = a.ps + (size_t)(a.ps_pos + j) * B + b;
    goal = mk(g[0], g[4 * B], g[8 * B]);
  }
  const double cpt_feet = quad_sum(in_contact ? 1.0 : 0.0);
  const V3 feet_sum = quad_sum3(in_contact ? goal : zero);
  V3 mean_feet = s.v3(kEsMeanFeet);
  if (cpt_feet > 0.0) mean_feet = mk(feet_sum.x / cpt_feet, feet_sum.y / cpt_feet, feet_sum.z / cpt_feet);

  // ---- alpha schedule (:503-517), with the reference's literals
  const double ksc_max = quad_max(ksc);
  const double sa = ceil(ksc_max / 10) - 1;
  const double sb = remaining_steps;
  const double n = 1;
  const double v_max = 1.00, v_min = 0.97;
  const double c = ((sa + sb) - 2 * n) * 0.5;
  double alpha, close;
  if (sa <= (n - 1) || sb <= n) {
    alpha = v_max;
    close = 1.0;
  } else {
    alpha = v_min + (v_max - v_min) * fabs(c - (sa - n)) / c;
    close = 0.0;
  }

  // ---- the outputs that do not wait for the filters (:597-598, :605-606, :624-627), stored first: the Kalman filter below
  // needs the registers
  double* qf = a.q_filt + (size_t)b * 19;
  double* vf = a.v_filt + (size_t)b * 18;
  double* vs = a.v_secu + (size_t)b * 12;
#pragma unroll
  for (int i = 0; i < 3; i++) {  // this lane's leg
    const double sec = (1.0 - a.alpha_secu) * dq3[i] + a.alpha_secu * s(kEsVsecu + 3 * j + i);  // (:624)
    qf[7 + 3 * j + i] = q3[i];
    vf[6 + 3 * j + i] = dq3[i];
    vs[3 * j + i] = sec;
    s(kEsVsecu + 3 * j + i) = sec;
  }
  s(kEsKsc + j) = ksc;
  // the per-robot results: lanes 0..2 store component j of every 3-vector, lane 3 the scalars and the quaternion
  if (j < 3) {
    vf[3 + j] = pick(gyro, j);
    a.rpy[(size_t)b * 3 + j] = pick(rpy, j);
    s(kEsFkVel + j) = pick(fk_vel, j);
    s(kEsFkXyz + j) = pick(fk_xyz, j);
    s(kEsMeanFeet + j) = pick(mean_feet, j);
  } else {
    qf[3] = qx; qf[4] = qy; qf[5] = qz; qf[6] = qw;
    s(kEsAlpha) = alpha;
    s(kEsClose) = close;
    s(kEsYawOff) = yaw_off;
    s(kEsKlog) = k_log + 1.0;  // (:627)
  }

  const V3 lever = mk(0.1163, 0.0, 0.02);  // _1Mi.translation (:323-324)
  V3 pos, b_filt, hpv, lpv, hpp, lpp;
  if constexpr (!KALMAN) {
    // ---- cascade of complementary filters (:521-553)
    const V3 cross_product = cross(lever, gyro);
    const V3 i_fk = fk_vel + cross_product;
    const V3 oi_fk = mul(oRb, i_fk);
    const V3 o_acc = mul(oRb, acc);
    hpv = s.v3(kEsHPv), lpv = s.v3(kEsLPv);
    hpv = alpha * (hpv + a.dt * o_acc);             // ComplementaryFilter.compute (:223)
    lpv = alpha * lpv + (1.0 - alpha) * oi_fk;      // (:226)
    const V3 oi_filt = hpv + lpv;
    const V3 i_filt = mulT(oRb, oi_filt);
    b_filt = i_filt - cross_product;
    const V3 ob_filt = mul(oRb, b_filt);
    const V3 x_pos = fk_xyz + mean_feet;
    hpp = s.v3(kEsHPp), lpp = s.v3(kEsLPp);
    const double axy = 0.995, az = 0.9;             // (:549-550)
    hpp = mk(axy * (hpp.x + ob_filt.x * a.dt), axy * (hpp.y + ob_filt.y * a.dt), az * (hpp.z + ob_filt.z * a.dt));
    lpp = mk(axy * lpp.x + (1.0 - axy) * x_pos.x, axy * lpp.y + (1.0 - axy) * x_pos.y, az * lpp.z + (1.0 - az) * x_pos.z);
    pos = hpp + lpp;
  } else {
    // ---- Kalman filter (:555-580): lane j < 3 owns axis j, lane 3 shadows lane 2
    const int ax = j < 3 ? j : 2;
    const ES ks{a.ks + b, B};
    const V3 z = mul(oRb, lever - K.pf);  // this leg's rows 3j..3j+2 of Z (:569); its row 12+j is 0 (:570)
    const V3 z0 = mk(quad_bcast<0>(z.x), quad_bcast<0>(z.y), quad_bcast<0>(z.z));
    const V3 z1 = mk(quad_bcast<1>(z.x), quad_bcast<1>(z.y), quad_bcast<1>(z.z));
    const V3 z2 = mk(quad_bcast<2>(z.x), quad_bcast<2>(z.y), quad_bcast<2>(z.z));
    const V3 z3 = mk(quad_bcast<3>(z.x), quad_bcast<3>(z.y), quad_bcast<3>(z.z));
    const double z_kin[4] = {pick(z0, ax), pick(z1, ax), pick(z2, ax), pick(z3, ax)};
    const double st4[4] = {quad_bcast<0>(status), quad_bcast<1>(status), quad_bcast<2>(status), quad_bcast<3>(status)};
    const kf::Tuning tune{a.kf_sigma_kin, a.kf_sigma_h, a.kf_sigma_a, a.kf_sigma_dp, a.kf_gamma};
    const kf::Coeffs co = kf::update_coeffs(tune, a.dt, st4);  // updateCoeffs (:167-181)
    const V3 o_acc = mul(oRb, acc);
    kf::Axis A;
#pragma unroll
    for (int k = 0; k < 6; k++) A.x[k] = ks(kKsX + kf::state_index(ax, k));
#pragma unroll
    for (int k = 0; k < 36; k++) A.p[k] = ks(kKsP + 36 * ax + k);
    kf::axis_step(A, ax == 2, a.dt, pick(o_acc, ax), z_kin, co);  // predict (:152-157), correct (:159-165)
    if (j < 3) {
#pragma unroll
      for (int k = 0; k < 6; k++) ks(kKsX + kf::state_index(ax, k)) = A.x[k];
#pragma unroll
      for (int k = 0; k < 36; k++) ks(kKsP + 36 * ax + k) = A.p[k];
    }
    ks(kKsZ + 3 * j) = z.x; ks(kKsZ + 3 * j + 1) = z.y; ks(kKsZ + 3 * j + 2) = z.z;
    ks(kKsZ + 12 + j) = 0.0;
    // results (:578-580)
    const double xp[3] = {quad_bcast<0>(A.x[0]), quad_bcast<1>(A.x[0]), quad_bcast<2>(A.x[0])};
    const double xv[3] = {quad_bcast<0>(A.x[1]), quad_bcast<1>(A.x[1]), quad_bcast<2>(A.x[1])};
    pos = mk(kf::base_position(0, xp[0]), kf::base_position(1, xp[1]), kf::base_position(2, xp[2]));
    const double R9[9] = {oRb.r0.x, oRb.r0.y, oRb.r0.z, oRb.r1.x, oRb.r1.y, oRb.r1.z, oRb.r2.x, oRb.r2.y, oRb.r2.z};
    const double g3[3] = {gyro.x, gyro.y, gyro.z};
    double bv[3];
    kf::base_velocity(R9, xv, g3, bv);
    b_filt = mk(bv[0], bv[1], bv[2]);
  }

  // ---- the filtered position and velocity (:594-604)
  V3 v_new = b_filt;
  if (a.perfect) {
    pos.z = a.true_pos[(size_t)b * 3 + 2] - 0.0155;  // (:595-596)
    v_new = mk(a.true_b_vel[(size_t)b * 3], a.true_b_vel[(size_t)b * 3 + 1], a.true_b_vel[(size_t)b * 3 + 2]);  // (:601-602)
  }
  const V3 v_old = s.v3(kEsVfilt);
  const V3 v_lin = (1.0 - a.alpha_v) * v_old + a.alpha_v * v_new;
  if (j < 3) {
    qf[j] = pick(pos, j);
    vf[j] = pick(v_lin, j);
    if constexpr (!KALMAN) {  // (the reference leaves the complementary filters alone in Kalman mode)
      s(kEsHPv + j) = pick(hpv, j);
      s(kEsLPv + j) = pick(lpv, j);
      s(kEsHPp + j) = pick(hpp, j);
      s(kEsLPp + j) = pick(lpp, j);
    }
    s(kEsFiltVel + j) = pick(b_filt, j);
    s(kEsVfilt + j) = pick(v_lin, j);
  }
}

int estimator_launch(const EstimatorArgs& a, hipStream_t stream) {
  if (a.init) hipLaunchKernelGGL(estimator_init_kernel, dim3((a.B + 63) / 64), dim3(64), 0, stream, a);
  else if (a.kalman) hipLaunchKernelGGL(estimator_kernel<true>, dim3((a.B + 15) / 16), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(estimator_kernel<false>, dim3((a.B + 15) / 16), dim3(64), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qrw
