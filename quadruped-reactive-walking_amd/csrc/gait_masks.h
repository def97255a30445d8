// The gait matrices of the planners (Gait, src/Gait.cpp:19-260) as bit masks, in plain C++ on integers: the same text is compiled
// into planner_kernel.hip and into a stand-alone host program (tests/test_gait_masks_cpu.py), which is where this arithmetic is
// checked, row by row against the dense matrices of oracle/planner_oracle.c, and debugged.
//
// The reference keeps the three gait matrices (past / current / desired, N_gait x 4 entries that are only ever
// 0 or 1) as dense double matrices and rolls them with chains of row swaps; run literally against HBM that is
// thousands of dependent memory round trips per control iteration.  Here a matrix is four 64-bit column masks in
// registers and in the persistent state (bit i = row i; the host getters unpack them), so
// "row i is all zero", "roll rows 0..n" and the phase-duration scans are a few integer instructions.
//
// THE SIZE RULE (gait_table_fits).  Everything below assumes that a zero row follows the live rows and that no shift count
// reaches 64.  Both hold when no generator can set bit 63, i.e. when every gait a joystick code can select fits the table:
//     N_gait <= 63,   n_steps + 1 <= N_gait,   gait_rows_needed(T_gait, dt_mpc) <= N_gait
// where gait_rows_needed is the largest number of rows create_desired writes: 2 lround(0.5 T_gait / dt_mpc) (pacing, bounding,
// trot), 4 lround(0.25 T_gait / dt_mpc) (walk), lround(T_gait / dt_mpc) (static).  The reference's Gait::initialize tests only the
// last of the three (src/Gait.cpp:30-31) and writes outside its matrices when one of the others is larger.  A period that fills
// the table exactly is legal: row N_gait then counts as a zero row -- which is what the masks do on their own (bits N_gait..63
// are never set), and where the reference reads one row past its matrices.
// qrw_planner_init applies the rule on the host BEFORE the first launch; the kernels rely on it and do not test it again.
//
// The functions that read planner parameters are templates over the argument block: they use its members T_gait, dt_mpc,
// n_steps and k_mpc (qrw::PlannerArgs in the kernels, a four-member struct in the host program).
#pragma once
#include <limits.h>
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QRW_GM_FN static __host__ __device__
#define QRW_GM_INL static __host__ __device__ __forceinline__
#define QRW_GM_UNROLL _Pragma("unroll")
#else
#define QRW_GM_FN static inline
#define QRW_GM_INL static inline
#define QRW_GM_UNROLL
#endif

namespace qrw {

// 1-based index of the lowest set bit (0 for 0) / number of leading zeros (x != 0): the device intrinsics in device code, the
// compiler's builtins on the host
QRW_GM_INL int gm_ffs(unsigned long long x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)x);
#else
  return __builtin_ffsll((long long)x);
#endif
}
QRW_GM_INL int gm_clz(unsigned long long x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __clzll((long long)x);
#else
  return __builtin_clzll(x);
#endif
}

// ---- the size rule (see the head of this file); host and device round alike: these are create_desired's own expressions
QRW_GM_INL int gait_rows_needed(double T_gait, double dt_mpc) {
  const double per = T_gait / dt_mpc;
  if (!(per >= 0.0 && per < 1.0e6)) return INT_MAX;  // (NaN, negative, or beyond what lround may be asked to convert)
  const long half = 2 * lround(0.5 * T_gait / dt_mpc), quarter = 4 * lround(0.25 * T_gait / dt_mpc), whole = lround(T_gait / dt_mpc);
  const long m = (half > quarter) ? ((half > whole) ? half : whole) : ((quarter > whole) ? quarter : whole);
  return (int)m;
}
QRW_GM_INL bool gait_table_fits(int N_gait, int n_steps, double T_gait, double dt_mpc) {
  return N_gait >= 1 && N_gait <= 63 && n_steps >= 1 && n_steps + 1 <= N_gait && gait_rows_needed(T_gait, dt_mpc) <= N_gait;
}

struct Gm {
  unsigned long long c[4];
};
QRW_GM_INL unsigned long long gm_any(const Gm& m) { return m.c[0] | m.c[1] | m.c[2] | m.c[3]; }
QRW_GM_INL bool rz(const Gm& m, int i) { return ((gm_any(m) >> i) & 1ull) == 0ull; }
QRW_GM_INL bool gbit(const Gm& m, int i, int j) {
  const unsigned long long col = (j == 0) ? m.c[0] : (j == 1) ? m.c[1] : (j == 2) ? m.c[2] : m.c[3];
  return ((col >> i) & 1ull) != 0ull;
}
QRW_GM_INL unsigned long long lowmask(int n) { return (n >= 64) ? ~0ull : ((1ull << n) - 1ull); }
// rows 0..n-1: new[r] = old[r+1] (r < n-1), new[n-1] = old[0]   (what "swap(0,1), swap(1,2), ..., swap(n-2,n-1)" does)
QRW_GM_INL void rot_up(Gm& m, int n) {
  if (n < 2) return;
  QRW_GM_UNROLL
  for (int c = 0; c < 4; c++) {
    const unsigned long long lo = m.c[c] & lowmask(n), hi = m.c[c] & ~lowmask(n);
    m.c[c] = hi | (lo >> 1) | ((lo & 1ull) << (n - 1));
  }
}
// rows 0..n-1: new[0] = old[n-1], new[r] = old[r-1]              ("swap(n-1,n-2), ..., swap(1,0)")
QRW_GM_INL void rot_down(Gm& m, int n) {
  if (n < 2) return;
  QRW_GM_UNROLL
  for (int c = 0; c < 4; c++) {
    const unsigned long long lo = m.c[c] & lowmask(n), hi = m.c[c] & ~lowmask(n);
    m.c[c] = hi | ((lo << 1) & lowmask(n)) | ((lo >> (n - 1)) & 1ull);
  }
}
// rows r0 .. r0 + n - 1 (r0 + n <= 64, r0 < 64)
QRW_GM_INL void rows_fill(Gm& m, int r0, int n, bool a, bool b, bool c, bool d) {
  const unsigned long long f = lowmask(n) << r0;
  if (a) m.c[0] |= f;
  if (b) m.c[1] |= f;
  if (c) m.c[2] |= f;
  if (d) m.c[3] |= f;
}

// desired gait of one period (src/Gait.cpp:38-108); code 5 = walk (exists in the reference but is not reachable there)
template <class Args>
QRW_GM_FN void create_desired(Gm& des, const Args& a, int code) {
  des.c[0] = des.c[1] = des.c[2] = des.c[3] = 0ull;
  const int Nh = (int)lround(0.5 * a.T_gait / a.dt_mpc);
  if (code == 1) { rows_fill(des, 0, Nh, 1, 0, 1, 0); rows_fill(des, Nh, Nh, 0, 1, 0, 1); }
  else if (code == 2) { rows_fill(des, 0, Nh, 1, 1, 0, 0); rows_fill(des, Nh, Nh, 0, 0, 1, 1); }
  else if (code == 3) { rows_fill(des, 0, Nh, 1, 0, 0, 1); rows_fill(des, Nh, Nh, 0, 1, 1, 0); }
  else if (code == 4) { rows_fill(des, 0, (int)lround(a.T_gait / a.dt_mpc), 1, 1, 1, 1); }
  else if (code == 5) {
    const int Nq = (int)lround(0.25 * a.T_gait / a.dt_mpc);
    rows_fill(des, 0, Nq, 0, 1, 1, 1); rows_fill(des, Nq, Nq, 1, 0, 1, 1);
    rows_fill(des, 2 * Nq, Nq, 1, 1, 0, 1); rows_fill(des, 3 * Nq, Nq, 1, 1, 1, 0);
  }
}

// Gait::initialize (src/Gait.cpp:19-36) + create_gait_f (:110-139)
template <class Args>
QRW_GM_FN void gait_init(Gm& past, Gm& cur, Gm& des, const Args& a) {
  past.c[0] = past.c[1] = past.c[2] = past.c[3] = 0ull;
  cur = past;
  create_desired(des, a, 3);
  int i = 0;
  for (int j = 0; j < a.n_steps; j++) {
    QRW_GM_UNROLL
    for (int c = 0; c < 4; c++) cur.c[c] |= ((des.c[c] >> i) & 1ull) << j;
    i++;
    if (rz(des, i)) i = 0;
  }
  int index = 1;
  // ends at index <= N_gait <= 63: by the size rule no generator sets bit 63, so a zero row is always found and the shift count
  // of rz stays below 64
  while (!rz(des, index)) index++;
  for (int k = 0; k < i; k++) rot_up(des, index);
}

// Gait::getPhaseDuration (src/Gait.cpp:141-182); also leaves remainingTime_.  The reference walks the rows one by one (forwards
// through the current gait and on into the desired one, backwards through the current one and on into the past one); on column
// masks each walk is "count the consecutive rows whose bit equals `value`" = a count of trailing / leading ones: no loop (round 4:
// the loops' trip counts differ per lane, a wavefront paid the longest one, ~1 k instructions per call).
// Defined for any three masks and 0 <= i <= 63: a row beyond 63 counts as a zero row.
QRW_GM_INL int trailing_ones(unsigned long long x) { return (~x == 0ull) ? 64 : (gm_ffs(~x) - 1); }
template <class Args>
QRW_GM_FN double phase_duration(const Gm& past, const Gm& cur, const Gm& des, const Args& a, int i, int j, bool value,
                                double& remain) {
  const unsigned long long ccur = (j == 0) ? cur.c[0] : (j == 1) ? cur.c[1] : (j == 2) ? cur.c[2] : cur.c[3];
  const unsigned long long cdes = (j == 0) ? des.c[0] : (j == 1) ? des.c[1] : (j == 2) ? des.c[2] : des.c[3];
  const unsigned long long cpast = (j == 0) ? past.c[0] : (j == 1) ? past.c[1] : (j == 2) ? past.c[2] : past.c[3];
  const unsigned long long vcur = value ? ccur : ~ccur, vdes = value ? cdes : ~cdes, vpast = value ? cpast : ~cpast;
  const unsigned long long nzc = gm_any(cur);
  // forwards: rows i + 1, i + 2, ... while the row is not all zero and the foot's entry equals `value` (:147-152)
  const unsigned long long fwd = (i + 1 < 64) ? ((vcur & nzc) >> (i + 1)) : 0ull;
  const int run = trailing_ones(fwd);
  int cnt = 1 + run;
  const int inext = i + run + 1;
  if (inext >= 64 || ((nzc >> inext) & 1ull) == 0ull) cnt += trailing_ones(vdes & gm_any(des));  // the walk ran into the zero row: on into the desired gait (:154-162)
  remain = (double)cnt;  // remainingTime_ (:164)
  // backwards from the ORIGINAL row: rows i - 1, i - 2, ... while the entry equals `value` (no zero-row test, :167-171)
  const unsigned long long miss = ~vcur & lowmask(i);  // rows below i whose entry differs
  const int runb = (miss == 0ull) ? i : (i - 1 - (63 - gm_clz(miss)));
  cnt += runb;
  if (runb == i) cnt += trailing_ones(vpast & gm_any(past));  // reached row 0: on into the past gait (:173-180)
  return (double)cnt * a.dt_mpc;
}

// Gait::updateGait = changeGait + rollGait (src/Gait.cpp:184-260); returns whether the gait matrices were rolled
template <class Args>
QRW_GM_FN void gait_update(Gm& past, Gm& cur, Gm& des, const Args& a, int k, int code, double& newphase) {
  if (code >= 1 && code <= 5) create_desired(des, a, code);
  if (k % a.k_mpc != 0) return;
  rot_down(past, a.n_steps + 1);
  bool differ = false;
  QRW_GM_UNROLL
  for (int c = 0; c < 4; c++) {
    past.c[c] = (past.c[c] & ~1ull) | (cur.c[c] & 1ull);
    differ = differ || ((cur.c[c] & 1ull) != ((cur.c[c] >> 1) & 1ull));
  }
  newphase = differ ? 1.0 : 0.0;
  int index = 1;
  // the current gait never holds more than N_gait <= 63 rows (it starts with n_steps and a roll takes one row and adds at most
  // one), so bit 63 is never set: the loop ends at index <= 63 and rz never shifts by 64
  while (!rz(cur, index)) index++;
  rot_up(cur, index);
  QRW_GM_UNROLL
  for (int c = 0; c < 4; c++) cur.c[c] = (cur.c[c] & ~(1ull << (index - 1))) | ((des.c[c] & 1ull) << (index - 1));
  index = 1;
  // the desired gait holds at most gait_rows_needed <= N_gait <= 63 rows (the size rule): bit 63 is never set, as above
  while (!rz(des, index)) index++;
  rot_up(des, index);
}

}  // namespace qrw
