// Host <-> kernel argument block and per-instance state layout of the joystick stage (joystick_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "joystick_profile.h"

namespace qrw {

// persistent state: js[item][B] (item-major, as the estimator's)
enum JoyStateItem {
  kJsVref = 0,   // the gamepad filter's v_ref (6); stays zero in the other modes
  kJsKstop = 6,  // tick of the first stop flag, -1 while there was none
  kJoyStItems = 7
};
struct JoystickArgs {
  joy::Tables t;
  int32_t k;
  int init;               // 1: write the initial state and nothing else
  const double* v_gp;     // gamepad mode: [B][6] this tick's unfiltered command
  const int32_t* stop;    // [B] or null
  double* st;             // [kJoyStItems][B]
  double* joy_vref;       // [B][6]
  int32_t* code;          // [B] or null
  double* f_ext;          // [B][6] or null
};
int joystick_launch(const JoystickArgs& a, int mode, hipStream_t stream);

}  // namespace qrw
