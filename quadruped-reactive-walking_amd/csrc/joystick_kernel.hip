// Joystick stage for a batch of Solo12 instances -- gfx950 (MI355X): the tick in, reference velocity, gait code and push out.
//
// Replaces, per instance, the first line of the reference's control iteration, Joystick.update_v_ref(k, velID)
// (scripts/Controller.py:210), and the pushes the simulator applies on its own account:
//   handle_v_switch / apply_velocity_change   scripts/Joystick.py:160-190   joystick_kernel<kProfile>
//   update_v_ref_multi_simu                   :289-315                      joystick_kernel<kRamp>
//   update_v_ref_gamepad's filter, dead band  :135-137                      joystick_kernel<kGamepad>
//   computeCode                               :144-158                      a schedule of (tick, code) pairs, every mode
//   apply_external_force                      scripts/PyBulletSimulator.py:402-431 (used at :354-356), every mode
// The arithmetic is joystick_profile.h (plain C++, also built for the host); this file is the mapping and the stop latch.
//
// Mapping: ONE THREAD PER ROBOT, 64 robots per wavefront.  The tables are item-major, so a wavefront reads one entry of its 64
// robots as contiguous rows; the segment of a profile is found from the k_switch rows alone (at most 32 int32 per robot) and
// only the two v_switch columns it needs are loaded.  No LDS, no scratch.  The outputs go out in the layouts their consumers
// read: d_joy_vref [B][6] (qrw_controller_update_state, qrw_control_pre, qrw_iteration_bind), d_code [B] int32 (the planners'
// d_code), d_f_ext [B][6] (qrw_sim_step).
//
// Stop latch: the first tick on which d_stop[b] != 0 (the controller's error flag) is stored in the robot's state; from that
// tick on its three outputs are zero and its filter state is frozen, also when the flag is cleared again.  The reference
// leaves its loop at the first error (scripts/main_solo12_control.py:180); k_stop is that outcome per robot.  Nothing crosses
// robots: no permute, no shared memory, no atomics.
//
// Departure: the wrench of a push is the simulator's world wrench at the base origin (d_f_ext of qrw_sim_step), not Bullet's
// LINK_FRAME.  Out of scope: the gamepad client, the `reduced` flag, joystick.stop reaching the controller's security branch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "joystick_profile.h"
#include "joystick_kernel.h"

namespace qrw {

template <int MODE>
__global__ __launch_bounds__(64) void joystick_kernel(JoystickArgs a) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.t.B) return;
  const size_t B = (size_t)a.t.B;
  double* st = a.st + b;  // [kJoyStItems][B]
  if (a.init) {
    for (int i = 0; i < 6; i++) st[(size_t)(kJsVref + i) * B] = 0.0;
    st[(size_t)kJsKstop * B] = -1.0;
    return;
  }
  double k_stop = st[(size_t)kJsKstop * B];
  if (k_stop < 0.0 && a.stop && a.stop[b] != 0) {
    k_stop = (double)a.k;
    st[(size_t)kJsKstop * B] = k_stop;
  }
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int32_t code = 0;
  if (k_stop < 0.0) {
    if (MODE == joy::kProfile) joy::profile_eval(a.t, b, a.k, v);
    if (MODE == joy::kRamp) joy::ramp_eval(a.t, b, a.k, v);
    if (MODE == joy::kGamepad) {
#pragma unroll
      for (int c = 0; c < 6; c++) {
        v[c] = joy::gamepad_filter(a.t.gp_alpha, a.t.gp_deadband, a.v_gp[(size_t)b * 6 + c], st[(size_t)(kJsVref + c) * B]);
        st[(size_t)(kJsVref + c) * B] = v[c];
      }
    }
    code = joy::code_at(a.t, b, a.k);
    if (a.f_ext) joy::push_sum(a.t, b, a.k, w);
  }
#pragma unroll
  for (int c = 0; c < 6; c++) a.joy_vref[(size_t)b * 6 + c] = v[c];
  if (a.code) a.code[b] = code;
  if (a.f_ext) {
#pragma unroll
    for (int c = 0; c < 6; c++) a.f_ext[(size_t)b * 6 + c] = w[c];
  }
}

int joystick_launch(const JoystickArgs& a, int mode, hipStream_t stream) {
  const dim3 grid((a.t.B + 63) / 64), block(64);
  if (mode == joy::kProfile) hipLaunchKernelGGL(joystick_kernel<joy::kProfile>, grid, block, 0, stream, a);
  else if (mode == joy::kRamp) hipLaunchKernelGGL(joystick_kernel<joy::kRamp>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(joystick_kernel<joy::kGamepad>, grid, block, 0, stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qrw
