// What the two host translation units of libqrw_hip.so share (qrw_api.hip: the product entry points; qrw_selftest.hip: the
// self-test, the poison kernels and the qrw_test_* entry points).  Internal: never installed, no kernel unit includes it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/qrw_hip.h"
#include "../../include/qrw_hip_test.h"
#include "qrw_kernels.h"

namespace qrw::host {

// Sets the calling thread's qrw_last_error() text ("what", or "what: <HIP's text for e>") and returns `code`.
int fail(int code, const char* what, hipError_t e = hipSuccess);

#define HIP_OK(expr, what)                              \
  do {                                                  \
    hipError_t e__ = (expr);                            \
    if (e__ != hipSuccess) return fail(-10, what, e__); \
  } while (0)

// One device allocation of `count` T's, freed when its owner goes.  Move-only; an empty one is false and frees nothing.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); return *this; }  // (o frees what this held)
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr; bytes = 0;
  }
  hipError_t alloc(size_t count) {  // (a failed one leaves the owner empty: the next attempt starts from nothing)
    reset();
    const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) p = nullptr;
    else bytes = count * sizeof(T);
    return e;
  }
  hipError_t fill(int byte, hipStream_t stream) const { return hipMemsetAsync(p, byte, bytes, stream); }
  size_t count() const { return bytes / sizeof(T); }
  operator T*() const { return p; }
};
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && std::is_nothrow_move_constructible<DevBuf<int>>::value, "DevBuf is move-only");
// ... and its sibling for one pinned, host-mapped word: a kernel writes it through `dev`, the host reads `host` without a device sync.
struct PinnedWord {
  unsigned *host = nullptr, *dev = nullptr;
  PinnedWord() = default;
  PinnedWord(const PinnedWord&) = delete;
  PinnedWord& operator=(const PinnedWord&) = delete;
  ~PinnedWord() { if (host) (void)hipHostFree(host); }
  hipError_t alloc() {
    hipError_t e = hipHostMalloc((void**)&host, 64, hipHostMallocMapped);
    if (e != hipSuccess) { host = nullptr; return e; }
    if ((e = hipHostGetDevicePointer((void**)&dev, host, 0)) == hipSuccess) host[0] = 0u;
    return e;
  }
};

// state families of a handle: which launches a getter has to wait for
// (the controller-glue kernels write state no getter reads: their launches are not tracked)
enum Family { kFamNone = -1, kFamMpc = 0, kFamWbc = 1, kFamPlan = 2, kFamEst = 3, kFamSim = 4, kFamJoy = 5, kFamCount = 6 };

}  // namespace qrw::host

struct qrw_handle_s {
  template <class T>
  using DevBuf = qrw::host::DevBuf<T>;
  qrw_config cfg;
  // Synchronisation is per handle, never device-wide: the *_host entry points and the getters run their copies and launches on
  // `host_stream` (private, non-blocking: it neither waits for nor stalls the legacy default stream or any other handle's
  // streams) and wait for exactly two things -- the last launch of the state family they read (wait_family) and their own copies.
  hipStream_t host_stream = nullptr;
  hipEvent_t order_ev = nullptr;    // qrw_stream_wait_stream (created on first use)
  // MPC
  DevBuf<double> mpc_st;
  DevBuf<int> mpc_gait, mpc_flags, mpc_iters, mpc_status, mpc_rho_updates, mpc_order;
  DevBuf<float> mpc_ema;  // moving average of each instance's iteration counts (longest-first block order)
  bool mpc_have_order = false;
  DevBuf<double> mpc_rho, mpc_pri, mpc_dua, mpc_prof;
  // sequences (qrw_mpc_solve_sequence), allocated at the first one: task queue, counters, argument block re-read by the persistent kernel
  DevBuf<int> seq_queue, seq_hot, seq_first;
  DevBuf<unsigned> seq_ctr;
  int seq_groups = 0;
  // preemptive launch of qrw_mpc_solve (N > 16, more instances than resident slots): FIFO of parked solves, counters
  DevBuf<int> pre_queue, pause_it;
  DevBuf<unsigned> pre_ctr;
  int pre_chunk = 0, pre_cmax = 0, pre_min_batch = 0, pre_levels = 1, pre_bin = 200;
  int pre_slots = 0;                // two-wavefront instances resident at a time (2 per compute unit)
  qrw::host::PinnedWord pre_err;    // the kernel's give-up code of a time-sliced launch (read on entry of the next)
  bool force_giveup = false;        // tests (QRW_PREEMPT_FORCE_GIVEUP=1): every time-sliced launch starts with its error word set
  // WBC
  DevBuf<double> wbc_st;
  DevBuf<int> wbc_iters, wbc_status;
  int wbc_lanes16 = 1;  // full WBC compute with sixteen lanes per instance (wbc16_kernel); qrw_wbc_set_lanes / QRW_WBC16=0: one quad
  double Y[6];
  // controller glue, planners
  DevBuf<double> ctrl_st, plan_st;
  qrw_planner_config pcfg;
  bool plan_ready = false;
  // state estimator
  DevBuf<double> est_st;
  qrw_estimator_config ecfg;
  double est_alpha_v = 0.0, est_alpha_secu = 0.0;
  bool est_ready = false;
  DevBuf<double> kal_st;     // the Kalman variant's state, allocated by the first qrw_estimator_init_kalman
  qrw_kalman_config kcfg;
  bool est_kalman = false;   // which filter the last initialisation chose
  // rigid-body simulator: its state, its parameters, and the measurement buffers of the host-buffer entry points (allocated by
  // qrw_sim_init_host: a frozen robot's rows keep their last finite values there, as in a caller's device buffers)
  DevBuf<double> sim_st, sim_out;
  qrw_sim_params sim_prm;
  bool sim_ready = false;
  // the simulator's heightfield terrain (qrw_sim_set_terrain): the handle's own copy of the heights and of the per-robot
  // origins, kept across qrw_sim_init; the buffers are reallocated only when their size changes
  DevBuf<double> sim_terrain, sim_origin;
  int sim_t_rows = 0, sim_t_cols = 0;
  double sim_t_x0 = 0.0, sim_t_y0 = 0.0, sim_t_dx = 0.0, sim_t_dy = 0.0;
  bool sim_terrain_on = false, sim_origin_on = false;
  // joystick stage (qrw_joystick_init): its state (allocated by the first init), the handle's item-major copies of the tables
  // (reallocated only when their size changes) and the configuration they were validated against
  DevBuf<double> joy_st, joy_td;
  DevBuf<int32_t> joy_ti;
  qrw_joystick_config jcfg;
  bool joy_ready = false;
  // staging for the host-buffer entry points
  DevBuf<double> stage;
  DevBuf<int32_t> stage_i;
  qrw_iteration_buffers iter_bufs;  // qrw_iteration_bind
  bool iter_bound = false;
  // (atomics: qrw_stream_destroy, called from whatever thread owns the stream, clears these in every live handle)
  std::atomic<hipStream_t> last_stream[qrw::host::kFamCount] = {};
  std::atomic<bool> launched[qrw::host::kFamCount] = {};
  // host_stream drains before the members above free their buffers (the zero fills of a creation that failed half-way run on it)
  ~qrw_handle_s() {
    if (host_stream) { (void)hipStreamSynchronize(host_stream); (void)hipStreamDestroy(host_stream); }
    if (order_ev) (void)hipEventDestroy(order_ev);
  }
};

namespace qrw::host {

inline void note_launch(qrw_handle_s* h, int fam, hipStream_t s) {
  h->last_stream[fam].store(s, std::memory_order_relaxed);
  h->launched[fam].store(true, std::memory_order_release);
}
// Wait for the family's most recent launch (whatever stream the caller gave it), nothing else on the device.  Only the LAST
// stream of a family is remembered: a caller that launches one family of one handle on several streams that are not ordered
// among themselves has to order them itself before it calls a getter.  A stream the caller has destroyed since (its work had to
// be complete for that) is answered with an error by the runtime: cleared, and the conservative device-wide wait taken instead.
inline hipError_t wait_family(qrw_handle_s* h, int fam) {
  if (fam == kFamNone || !h->launched[fam].load(std::memory_order_acquire)) return hipSuccess;
  const hipStream_t last = h->last_stream[fam].load(std::memory_order_relaxed);
  if (last == h->host_stream) return hipSuccess;  // (host_stream work is waited for below / was at its call)
  hipError_t e = hipStreamSynchronize(last);
  if (e == hipSuccess) return e;
  (void)hipGetLastError();
  h->launched[fam] = false;
  return hipDeviceSynchronize();
}
inline hipError_t d2h(qrw_handle_s* h, void* dst, const void* src, size_t bytes) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->host_stream);
}
inline hipError_t h2d(qrw_handle_s* h, void* dst, const void* src, size_t bytes) {
  return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->host_stream);
}
inline hipError_t host_done(qrw_handle_s* h) { return hipStreamSynchronize(h->host_stream); }

// A getter's read-back: wait for the last launch of `fam` (kFamNone: the caller has waited already), queue the copies on
// host_stream (a null dst is a result the caller does not want), wait for them.  `who` is the entry point, for the error text.
struct Copy { void* dst; const void* src; size_t bytes; };
inline int read_back(qrw_handle_s* h, int fam, const char* who, std::initializer_list<Copy> copies) {
  HIP_OK(wait_family(h, fam), who);
  for (const Copy& c : copies)
    if (c.dst) HIP_OK(d2h(h, c.dst, c.src, c.bytes), who);
  HIP_OK(host_done(h), who);
  return 0;
}

// Every entry point works on the device its handle was created on and leaves the caller's current device alone.
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  explicit DeviceScope(int device) {
    if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = (hipSetDevice(device) == hipSuccess);
  }
  ~DeviceScope() {
    if (switched) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};
// Every entry point that queues copies from / to the CALLER'S host buffers (or the handle's staging area) on host_stream holds one
// of these: on ANY return -- the error paths too -- host_stream has drained, so nothing touches the caller's memory or h->stage
// after the call has come back.  On the normal path the function's own host_done() has already waited; this second
// wait on an idle stream costs ~1 us.
struct HostStreamGuard {
  qrw_handle_s* h;
  explicit HostStreamGuard(qrw_handle_s* handle) : h(handle) {}
  ~HostStreamGuard() {
    if (h && h->host_stream) (void)hipStreamSynchronize(h->host_stream);
  }
  HostStreamGuard(const HostStreamGuard&) = delete;
  HostStreamGuard& operator=(const HostStreamGuard&) = delete;
};
// The preamble of an entry point that takes a handle: a null handle or `bad` arguments are refused (-1, `what`); from here to the
// return, launches and copies go to the handle's GPU, and the caller's current device is restored on the way out.
#define QRW_ENTER(h, bad, what)                  \
  if (!(h) || (bad)) return fail(-1, what);      \
  qrw::host::DeviceScope dev_scope__((h)->cfg.device)
// ... of one that moves host buffers over host_stream as well
#define QRW_ENTER_HOST(h, bad, what) \
  QRW_ENTER(h, bad, what);           \
  qrw::host::HostStreamGuard host_guard__(h)

// the handle's terrain into a simulator launch (none set: the arguments stay zero and sim_launch picks the flat instantiation)
inline void sim_terrain_args(const qrw_handle_s* h, qrw::SimArgs& a) {
  if (!h->sim_terrain_on) return;
  a.terrain = h->sim_terrain;
  a.t_rows = h->sim_t_rows; a.t_cols = h->sim_t_cols;
  a.t_x0 = h->sim_t_x0; a.t_y0 = h->sim_t_y0; a.t_dx = h->sim_t_dx; a.t_dy = h->sim_t_dy;
  a.t_origin = h->sim_origin_on ? h->sim_origin.p : nullptr;
}

// the launch form qrw_mpc_solve uses for this handle (decided once, at creation)
inline bool mpc_time_sliced(const qrw_handle_s* h) { return h->pre_chunk > 0 && h->cfg.batch > h->pre_min_batch && h->pre_cmax > 1; }

// ---- qrw_selftest.hip
// QRW_DEBUG_POISON_LDS=1 (diagnostic): LDS and vector registers of the whole chip filled with NaN bits on `stream`, before a launch
void debug_poison_lds(hipStream_t stream);
// The known-answer gate of mpc_solve_kernel in launch form `mode` at horizon N: run once per process and device, remembered
// after that.  0 = passed; otherwise -20, with the error text (prefixed `who`) set.
enum KatMode { kKatPlain = 0, kKatSliced = 1, kKatSequence = 2, kKatModes = 3 };
int mpc_known_answer_gate(const char* who, int device, int N, int mode);

}  // namespace qrw::host
