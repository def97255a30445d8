// The joystick stage's arithmetic (scripts/Joystick.py, scripts/PyBulletSimulator.py:402-431) as plain C++ on doubles and
// int32_t: no device intrinsics, so the same text is compiled into joystick_kernel.hip and into a stand-alone host program
// (tests/test_joystick_cpu.py builds one under the address and undefined-behaviour sanitizers and compares its outputs with the
// numpy checker bit for bit).  Every function that rounds carries `#pragma clang fp contract(off)`: no fused multiply-add, so
// host, device and numpy evaluate the same correctly rounded IEEE sequence of + - * /.
//
// STATELESS IN THE TICK: except for the gamepad filter (and the stop latch, which lives in the kernel) every output is a function
// of the tick k and the tables alone.
//
// Tables are item-major, entry e of robot b at [e * B + b] (six-vectors: [(e * 6 + c) * B + b]): a wavefront of 64 consecutive
// robots reads one entry as contiguous rows.
//
// Limits (derived, not chosen: every integer power below must be exact in a double, whose significand holds 53 bits):
//   a profile segment is at most 2^17 ticks: t1^3 <= 2^51, and ev <= t1 there;
//   a push lasts 1 .. 2^13 ticks:            t1^4 <= 2^52, and ev <= t1 while it is active;
//   k_switch[0] <= 0 and k >= 0:             the evaluated tick always lies inside the segment found (below).
// check_profile / check_push / check_ramp say whether a robot's host tables keep them; qrw_joystick_init asks them before any
// launch and the kernel does not test again.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QRW_JOY_FN __host__ __device__ __forceinline__
#else
#define QRW_JOY_FN inline
#endif
#if defined(__clang__)
#define QRW_JOY_NO_CONTRACT _Pragma("clang fp contract(off)")
#define QRW_JOY_UNROLL _Pragma("unroll")
#else
#define QRW_JOY_NO_CONTRACT  // (other compilers: built with -ffp-contract=off)
#define QRW_JOY_UNROLL
#endif

namespace qrw {
namespace joy {

enum Mode { kProfile = 0, kRamp = 1, kGamepad = 2 };
constexpr int kMaxSwitch = 32, kMaxCodes = 16, kMaxPushes = 8;
constexpr int64_t kMaxSegment = 1 << 17;  // ticks between two consecutive switches
constexpr int64_t kMaxPush = 1 << 13;     // ticks a push lasts

struct Tables {
  int B;                             // robots = stride between two entries
  int n_switch, n_codes, n_pushes;   // entries per robot (the fleet's common lengths; shorter tables come padded, see below)
  int32_t k_start;                   // ramp mode: the tick the ramps start at
  double gp_alpha, gp_deadband;      // gamepad mode
  const int32_t* k_switch;           // [n_switch][B]
  const double* v_switch;            // [n_switch][6][B]
  const double* ramp_v;              // [3][B]: Vx, Vy, Vw
  const int32_t *code_k, *code_v;    // [n_codes][B]
  const int32_t *push_start, *push_dur;  // [n_pushes][B]
  const double* push_w;              // [n_pushes][6][B]: F (3), M (3)
};

// ---- profile mode: Joystick.apply_velocity_change (scripts/Joystick.py:183-188) for one component.
// A3 = 2 (v0 - v1) / t1^3, A2 = (-3/2) t1 A3, v = v0 + A2 ev^2 + A3 ev^3 in the reference's order and association; the integer
// powers are formed as products of the exactly converted integers (numpy forms them in int64 and converts: the same values).
QRW_JOY_FN double profile_blend(double v0, double v1, int32_t ev, int32_t t1) {
  QRW_JOY_NO_CONTRACT
  const double e = (double)ev, t = (double)t1;
  const double t3 = (t * t) * t, e2 = e * e, e3 = (e * e) * e;  // exact: |ev| <= t1 <= 2^17
  const double A3 = (2.0 * (v0 - v1)) / t3;
  const double A2 = (-1.5 * t) * A3;
  return (v0 + A2 * e2) + A3 * e3;
}

// Joystick.handle_v_switch (:167-171) for robot b at tick k >= 0, all six components.
// The reference scans i = 1; while i < n and k_switch[i] <= k: i++, evaluates segment (i-1, i) when i != n and otherwise LEAVES
// v_ref at what the previous tick wrote.  A loop that visits every tick from 0 therefore holds, from k_switch[n-1] on, the value
// of tick k_switch[n-1] - 1: the stateless equivalent is to evaluate at k' = min(k, k_switch[n-1] - 1), and where no tick
// 0 .. k has i != n (k_switch[n-1] <= 0, n = 1 among them) the value is the initial v_ref, zeros.  With k_switch[0] <= 0 <= k'
// the segment found has k_switch[i-1] <= k' < k_switch[i]: t1 > 0 and 0 <= ev < t1.  Equal consecutive entries are never
// selected (the scan passes both or stops before the first), so a table padded by repeating its last column gives the same bits.
QRW_JOY_FN void profile_eval(const Tables& T, int b, int32_t k, double v[6]) {
  const size_t B = (size_t)T.B;
  const int n = T.n_switch;
  const int32_t k_last = T.k_switch[(size_t)(n - 1) * B + b];
  if (k_last <= 0) {
    for (int c = 0; c < 6; c++) v[c] = 0.0;
    return;
  }
  const int32_t ke = k < k_last - 1 ? k : k_last - 1;
  int32_t lo = T.k_switch[b], hi = lo;
  int seg = 0;  // (always found: k_switch[n-1] > ke)
  for (int i = 1; i < n; i++) {
    const int32_t cur = T.k_switch[(size_t)i * B + b];
    if (seg == 0) {
      if (cur > ke) { seg = i; hi = cur; }
      else lo = cur;
    }
  }
  const int32_t ev = ke - lo, t1 = hi - lo;
  const double* c0 = T.v_switch + (size_t)(seg - 1) * 6 * B + b;
  const double* c1 = T.v_switch + (size_t)seg * 6 * B + b;
QRW_JOY_UNROLL
  for (int c = 0; c < 6; c++) v[c] = profile_blend(c0[(size_t)c * B], c1[(size_t)c * B], ev, t1);
}

// ---- ramp mode: Joystick.update_v_ref_multi_simu (:302-313) for one component; scale 10000 for Vx, Vy and 2500 for Vw.
// beta = (int) max(|V| scale, 100.0); alpha = max(min((k - k_start) / beta, 1.0), 0.0); V alpha.
QRW_JOY_FN double ramp_component(double V, double scale, int32_t k, int32_t k_start) {
  QRW_JOY_NO_CONTRACT
  const double m = fabs(V) * scale;
  const int32_t beta = (int32_t)(m > 100.0 ? m : 100.0);  // (check_ramp: below 2^31)
  const double x = (double)((int64_t)k - (int64_t)k_start) / (double)beta;
  const double lo = x < 1.0 ? x : 1.0;
  const double alpha = lo > 0.0 ? lo : 0.0;
  return V * alpha;
}
QRW_JOY_FN void ramp_eval(const Tables& T, int b, int32_t k, double v[6]) {
  const size_t B = (size_t)T.B;
  v[0] = ramp_component(T.ramp_v[b], 10000.0, k, T.k_start);
  v[1] = ramp_component(T.ramp_v[B + b], 10000.0, k, T.k_start);
  v[2] = v[3] = v[4] = 0.0;
  v[5] = ramp_component(T.ramp_v[2 * B + b], 2500.0, k, T.k_start);
}

// ---- gamepad mode: the low-pass filter and its dead band (:136-137) for one component; the comparisons are strict.
QRW_JOY_FN double gamepad_filter(double alpha, double band, double v_gp, double v_ref) {
  QRW_JOY_NO_CONTRACT
  const double v = alpha * v_gp + (1.0 - alpha) * v_ref;
  return (v < band && v > -band) ? 0.0 : v;
}

// ---- codes: computeCode's one-shot (:144-158) from a schedule: `code` on tick code_k, 0 on every other; later pairs win.
// (k >= 0: an entry with a negative tick never fires, which is how a shorter table is padded.)
QRW_JOY_FN int32_t code_at(const Tables& T, int b, int32_t k) {
  const size_t B = (size_t)T.B;
  int32_t code = 0;
  for (int e = 0; e < T.n_codes; e++)
    if (T.code_k[(size_t)e * B + b] == k) code = T.code_v[(size_t)e * B + b];
  return code;
}

// ---- pushes: apply_external_force (scripts/PyBulletSimulator.py:415-425).  A4 = 16 / t1^4, A3 = -2 t1 A4, A2 = t1^2 A4,
// alpha = A2 ev^2 + A3 ev^3 + A4 ev^4, for 0 <= ev <= t1 <= 2^13.
QRW_JOY_FN double push_alpha(int32_t ev, int32_t t1) {
  QRW_JOY_NO_CONTRACT
  const double e = (double)ev, t = (double)t1;
  const double t2 = t * t, t4 = t2 * t2, e2 = e * e, e3 = e2 * e, e4 = e2 * e2;  // exact
  const double A4 = 16.0 / t4;
  const double A3 = (-2.0 * t) * A4;
  const double A2 = t2 * A4;
  return (A2 * e2 + A3 * e3) + A4 * e4;
}
// the sum over the entries active at tick k (start <= k <= start + duration), in table order, of alpha [F; M]
QRW_JOY_FN void push_sum(const Tables& T, int b, int32_t k, double w[6]) {
  QRW_JOY_NO_CONTRACT
  const size_t B = (size_t)T.B;
QRW_JOY_UNROLL
  for (int c = 0; c < 6; c++) w[c] = 0.0;
  for (int e = 0; e < T.n_pushes; e++) {
    const int64_t ev = (int64_t)k - (int64_t)T.push_start[(size_t)e * B + b];
    const int32_t t1 = T.push_dur[(size_t)e * B + b];
    if (ev < 0 || ev > (int64_t)t1) continue;
    const double alpha = push_alpha((int32_t)ev, t1);
    const double* F = T.push_w + (size_t)e * 6 * B + b;
QRW_JOY_UNROLL
    for (int c = 0; c < 6; c++) w[c] = w[c] + alpha * F[(size_t)c * B];
  }
}

// ---- what the init entry point asks of one robot's HOST tables (rows of that robot, contiguous) before any launch.
// 0 = fine; otherwise a reason (1 ..) with *entry the offending entry.
enum Bad { kOk = 0, kBadFirst = 1, kBadDecreasing = 2, kBadSegment = 3, kBadDuration = 4, kBadRamp = 5 };
inline int check_profile(const int32_t* k_switch, int n, int* entry) {
  *entry = 0;
  if (k_switch[0] > 0) return kBadFirst;
  for (int i = 1; i < n; i++) {
    *entry = i;
    const int64_t d = (int64_t)k_switch[i] - (int64_t)k_switch[i - 1];
    if (d < 0) return kBadDecreasing;
    if (d > kMaxSegment) return kBadSegment;
  }
  return kOk;
}
inline int check_push(const int32_t* duration, int n, int* entry) {
  for (int e = 0; e < n; e++) {
    *entry = e;
    if (duration[e] < 1 || (int64_t)duration[e] > kMaxPush) return kBadDuration;
  }
  return kOk;
}
inline int check_ramp(const double* V3, int* entry) {  // finite, and beta fits an int32_t
  const double scale[3] = {10000.0, 10000.0, 2500.0};
  for (int c = 0; c < 3; c++) {
    *entry = c;
    if (!(fabs(V3[c]) * scale[c] < 2147483647.0)) return kBadRamp;
  }
  return kOk;
}

}  // namespace joy
}  // namespace qrw
