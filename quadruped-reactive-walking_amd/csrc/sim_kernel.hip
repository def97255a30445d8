// Rigid-body simulator for a batch of Solo12 instances — gfx950 (MI355X): torques in, sensor readings out.
//
// One tick is, per instance, what the reference's loop does between two controller calls (scripts/PyBulletSimulator.py):
//   SendCommand       :672-710  the PD+ law from the joint state at the start of the tick (:679-688), then the physics step
//   UpdateMeasurment  :588-633  the readings the estimator takes (qrw_estimator_step reads these buffers as they are written)
// The physics step is NOT PyBullet's: `substeps` semi-implicit Euler steps of the forward dynamics M(q) a = [0; tau] + J'f +
// external wrench - h(q, v) (sim_dynamics.h) with a penalty normal force and regularised Coulomb friction on the plane z = 0 or,
// in the kernel's second instantiation, on a triangulated heightfield shared by the batch (sim_terrain.h; each robot may look
// it up at an offset of its own).  No joint limits, no joint friction; nothing about PyBullet's numerics is reproduced or claimed.
//
// Mapping: lane = 4*instance_in_wave + leg (FL, FR, HL, HR), ONE QUAD PER ROBOT INSTANCE, 16 instances per wavefront -- the
// mapping of estimator_kernel.  Each lane works its own leg: kinematics, contact force, bias forces, its 3x3 block of the
// mass matrix and the Schur complement of that block onto the base.  The four legs' shares of the base's 6x6 system (21 + 6
// numbers) go through DPP quad sums; all four lanes then solve the 6x6 alike, integrate the base alike and share the stores.
// No LDS.  The persistent state is item-major ([item][B]).  The heightfield is read straight from global memory, four heights
// per lane and sub-step (two 16-byte loads) with no reuse across lanes (a 512 x 512 field is 2 MiB and stays in the L2); they are
// asked for as soon as the foot's position is known (sim_leg_part; what the compiler makes of that at 256 VGPRs: DESIGN.md 4.7).
// sim_kernel<false> is, instruction for instruction, the kernel from before there was a terrain.
//
// A robot whose new state is not finite sets its status item and is frozen: no state item and no output of that tick or
// any later one is stored (the buffers keep what the last finite tick wrote); its quad leaves at once on later ticks.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "sim_dynamics.h"
#include "qrw_device.h"
#include "qrw_kernels.h"

namespace qrw {

namespace {

__device__ __forceinline__ double pick3(V3 v, int j) { return j == 0 ? v.x : j == 1 ? v.y : v.z; }
__device__ __forceinline__ bool finite3(V3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

// the acceleration of (q, v) under tau for this lane's leg and the base: the quad's four lanes call it together
template <bool kTerrain>
__device__ __forceinline__ void sim_accel(int j, const double q3[3], const double dq3[3], const double tau3[3], const M3& R, double px,
                                          double py, double pz, V3 vb, V3 wb, V3 fe, V3 me, const SimContact& cp, const SimGround& g,
                                          double ab[6], double ddq[3], V3& f_world) {
  const LegPart P = sim_leg_part<kTerrain>(j, q3, dq3, tau3, R, px, py, pz, vb, wb, cp, g);
  double S[21], r[6];
#pragma unroll
  for (int e = 0; e < 21; e++) S[e] = quad_sum(P.S[e]);
#pragma unroll
  for (int e = 0; e < 6; e++) r[e] = quad_sum(P.r[e]);
  sim_base_part(R, vb, wb, fe, me, S, r);
  sim_solve6(S, r, ab);
  sim_leg_ddq(P, ab, ddq);
  f_world = P.f_world;
}

}  // namespace

template <bool kTerrain>
__global__ __launch_bounds__(64) void sim_kernel(SimArgs a) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  const int b = t >> 2, j = t & 3;
  if (b >= a.B) return;  // (whole quads leave together: the quad permutes never read a lane that left)
  const size_t B = (size_t)a.B;
  double* const s = a.ss + b;
  const SimContact cp{a.kn, a.dn, a.mu, a.vs, a.foot_radius};
  V3 fe = mk(0.0, 0.0, 0.0), me = fe;
  if (a.f_ext) {
    const double* f = a.f_ext + (size_t)b * 6;
    fe = mk(f[0], f[1], f[2]);
    me = mk(f[3], f[4], f[5]);
  }
  SimGround g{};
  if constexpr (kTerrain) {
    g.T = terrain::Field{a.terrain, a.t_rows, a.t_cols, a.t_x0, a.t_y0, a.t_dx, a.t_dy};
    if (a.t_origin) {
      g.ox = a.t_origin[(size_t)b * 2];
      g.oy = a.t_origin[(size_t)b * 2 + 1];
    }
  }

  if (a.mode == 2) {  // forward dynamics only (tests): a18 and the contact forces of the given state
    const double* q = a.fd_q + (size_t)b * 19;
    const double* v = a.fd_v + (size_t)b * 18;
    double q3[3], dq3[3], tau3[3], ab[6], ddq[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      q3[i] = q[7 + 3 * j + i];
      dq3[i] = v[6 + 3 * j + i];
      tau3[i] = a.fd_tau[(size_t)b * 12 + 3 * j + i];
    }
    const M3 R = sim_quat_to_rot(q[3], q[4], q[5], q[6]);
    V3 fw;
    sim_accel<kTerrain>(j, q3, dq3, tau3, R, q[0], q[1], q[2], mk(v[0], v[1], v[2]), mk(v[3], v[4], v[5]), fe, me, cp, g, ab, ddq, fw);
    double* o = a.fd_a + (size_t)b * 18;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      o[6 + 3 * j + i] = ddq[i];
      a.contact_forces[(size_t)b * 12 + 3 * j + i] = pick3(fw, i);
    }
    if (j < 3) {
      o[j] = ab[j];
      o[3 + j] = ab[3 + j];
    }
    return;
  }

  // ---- state in
  double p[3], quat[4], q3[3], dq3[3];
  V3 vb, wb, prev;
  double tick = 0.0;
  if (a.mode == 1) {  // init: q from the caller, everything else zero (the reference's first UpdateMeasurment: prev_o_imuVel = 0)
    const double* q = a.q_init + (size_t)b * a.q_ld;
    if (a.q_ld == 19) {
      p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
      quat[0] = q[3]; quat[1] = q[4]; quat[2] = q[5]; quat[3] = q[6];
      q += 7;
    } else {
      p[0] = 0.0; p[1] = 0.0; p[2] = a.base_height;
      quat[0] = 0.0; quat[1] = 0.0; quat[2] = 0.0; quat[3] = 1.0;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
      q3[i] = q[3 * j + i];
      dq3[i] = 0.0;
    }
    if constexpr (kTerrain) {
      // the joints alone: the level base at (0, 0) stands base_height above the highest ground under its four feet
      if (a.q_ld != 19) {
        const V3 pf = leg_kinematics(leg_consts(j), q3).pf;
        p[2] += quad_max(terrain::surface(g.T, pf.x + g.ox, pf.y + g.oy).h);
      }
    }
    vb = wb = prev = mk(0.0, 0.0, 0.0);
  } else {
    if (s[(size_t)kSsStatus * B] != 0.0) return;  // frozen (the whole quad reads the same word)
#pragma unroll
    for (int i = 0; i < 3; i++) {
      p[i] = s[(size_t)(kSsQ + i) * B];
      q3[i] = s[(size_t)(kSsQ + 7 + 3 * j + i) * B];
      dq3[i] = s[(size_t)(kSsV + 6 + 3 * j + i) * B];
    }
#pragma unroll
    for (int i = 0; i < 4; i++) quat[i] = s[(size_t)(kSsQ + 3 + i) * B];
    vb = mk(s[(size_t)(kSsV + 0) * B], s[(size_t)(kSsV + 1) * B], s[(size_t)(kSsV + 2) * B]);
    wb = mk(s[(size_t)(kSsV + 3) * B], s[(size_t)(kSsV + 4) * B], s[(size_t)(kSsV + 5) * B]);
    prev = mk(s[(size_t)(kSsPrevImu + 0) * B], s[(size_t)(kSsPrevImu + 1) * B], s[(size_t)(kSsPrevImu + 2) * B]);
    tick = s[(size_t)kSsTick * B];
  }

  // ---- SendCommand (:679-688): PD+ torques from the joint state at the start of the tick, held over the sub-steps
  double tau3[3] = {0.0, 0.0, 0.0};
  V3 fw = mk(0.0, 0.0, 0.0);
  if (a.mode == 0) {
    const size_t c = (size_t)b * a.cmd_ld + 3 * j;
#pragma unroll
    for (int i = 0; i < 3; i++)
      tau3[i] = a.tau_ff[c + i] + a.P[c + i] * (a.q_des[c + i] - q3[i]) + a.D[c + i] * (a.v_des[c + i] - dq3[i]);
    const double h = a.dt / (double)a.substeps;
    for (int k = 0; k < a.substeps; k++) {
      const M3 R = sim_quat_to_rot(quat[0], quat[1], quat[2], quat[3]);
      double ab[6], ddq[3];
      sim_accel<kTerrain>(j, q3, dq3, tau3, R, p[0], p[1], p[2], vb, wb, fe, me, cp, g, ab, ddq, fw);
      // semi-implicit Euler: velocities first, positions from the new velocities
      vb = vb + h * mk(ab[0], ab[1], ab[2]);
      wb = wb + h * mk(ab[3], ab[4], ab[5]);
      const V3 dp = mul(R, vb);
      p[0] += h * dp.x; p[1] += h * dp.y; p[2] += h * dp.z;
      sim_quat_step(quat, wb, h);
#pragma unroll
      for (int i = 0; i < 3; i++) {
        dq3[i] += h * ddq[i];
        q3[i] += h * dq3[i];
      }
    }
  }

  // ---- UpdateMeasurment (:593-631)
  const M3 R = sim_quat_to_rot(quat[0], quat[1], quat[2], quat[3]);
  const V3 o_imu = mul(R, vb) + mul(R, cross(mk(0.1163, 0.0, 0.02), wb));  // (:626)
  const V3 acc = (1.0 / a.dt) * mulT(R, o_imu - prev);                      // (:628)

  // ---- finite, or frozen from here on
  bool ok = isfinite(q3[0]) && isfinite(q3[1]) && isfinite(q3[2]) && isfinite(dq3[0]) && isfinite(dq3[1]) && isfinite(dq3[2]) &&
            finite3(fw) && isfinite(tau3[0]) && isfinite(tau3[1]) && isfinite(tau3[2]);
  ok = ok && isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(quat[0]) && isfinite(quat[1]) && isfinite(quat[2]) &&
       isfinite(quat[3]) && finite3(vb) && finite3(wb) && finite3(acc) && finite3(o_imu);
  if (quad_max(ok ? 0.0 : 1.0) != 0.0) {
    if (j == 3) s[(size_t)kSsStatus * B] = 1.0;
    return;
  }

  // ---- stores: every lane its leg; lanes 0..2 component j of the 3-vectors, lane 3 the quaternion and the scalars
#pragma unroll
  for (int i = 0; i < 3; i++) {
    s[(size_t)(kSsQ + 7 + 3 * j + i) * B] = q3[i];
    s[(size_t)(kSsV + 6 + 3 * j + i) * B] = dq3[i];
    a.q_mes[(size_t)b * 12 + 3 * j + i] = q3[i];
    a.v_mes[(size_t)b * 12 + 3 * j + i] = dq3[i];
    a.contact_forces[(size_t)b * 12 + 3 * j + i] = pick3(fw, i);
    a.joint_torques[(size_t)b * 12 + 3 * j + i] = tau3[i];
  }
  if (j < 3) {
    s[(size_t)(kSsQ + j) * B] = p[j];
    s[(size_t)(kSsV + j) * B] = pick3(vb, j);
    s[(size_t)(kSsV + 3 + j) * B] = pick3(wb, j);
    s[(size_t)(kSsPrevImu + j) * B] = pick3(o_imu, j);  // (:629)
    a.ang_vel[(size_t)b * 3 + j] = pick3(wb, j);        // (:620: the world's angular velocity back in the base frame)
    a.o_imu_vel[(size_t)b * 3 + j] = pick3(o_imu, j);
    a.lin_acc[(size_t)b * 3 + j] = pick3(acc, j);
    a.true_pos[(size_t)b * 3 + j] = p[j];               // dummyPos (:604)
    a.true_b_vel[(size_t)b * 3 + j] = pick3(vb, j);     // b_baseVel (:624)
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      s[(size_t)(kSsQ + 3 + i) * B] = quat[i];
      a.quat[(size_t)b * 4 + i] = quat[i];
    }
    s[(size_t)kSsTick * B] = (a.mode == 1) ? 0.0 : tick + 1.0;
    if (a.mode == 1) s[(size_t)kSsStatus * B] = 0.0;
  }
}

int sim_launch(const SimArgs& a, hipStream_t stream) {
  if (a.terrain) hipLaunchKernelGGL(sim_kernel<true>, dim3((a.B + 15) / 16), dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(sim_kernel<false>, dim3((a.B + 15) / 16), dim3(64), 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qrw
