// Host side of libqrw_hip.so: the C ABI declared in include/qrw_hip.h (all of it but qrw_selftest_sweeps: qrw_selftest.hip).
// Owns the per-instance persistent solver state in HBM and launches the gfx950 kernels.
// There is NO CPU fallback: every entry point needs a HIP device and fails loudly otherwise.
#include <cmath>
#include <mutex>
#include <string>

#include "../../include/qrw_solo12_model.h"
#include "gait_masks.h"
#include "joystick_kernel.h"
#include "kalman_filter.h"
#include "qrw_host.h"

using namespace qrw::host;

namespace {
thread_local std::string g_err;
// live handles: qrw_stream_destroy forgets a destroyed stream in every handle that launched on it last
std::mutex g_handles_mutex;
std::vector<qrw_handle_s*> g_handles;
}  // namespace

int qrw::host::fail(int code, const char* what, hipError_t e) {
  char buf[512];
  if (e != hipSuccess) snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  else snprintf(buf, sizeof(buf), "%s", what);
  g_err = buf;
  return code;
}

extern "C" const char* qrw_last_error(void) { return g_err.c_str(); }

static void base_inertia_diag(double Y[6]) {
  // diag of crba(q_neutral)[:6,:6] (scripts/QP_WBC.py:89-93): total mass and the composite
  // rotational inertia about the base origin with every joint at zero (all link frames axis-aligned).
  const qrw_solo12_model& Mo = QRW_SOLO12_MODEL;
  double m = 0, I[3] = {0, 0, 0};
  auto add = [&](const qrw_link_inertial& L, const double o[3]) {
    const double c[3] = {o[0] + L.com[0], o[1] + L.com[1], o[2] + L.com[2]};
    const double n2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2];
    m += L.mass;
    I[0] += L.inertia[0] + L.mass * (n2 - c[0] * c[0]);
    I[1] += L.inertia[3] + L.mass * (n2 - c[1] * c[1]);
    I[2] += L.inertia[5] + L.mass * (n2 - c[2] * c[2]);
  };
  const double z[3] = {0, 0, 0};
  add(Mo.base, z);
  for (int l = 0; l < 4; l++) {
    const qrw_leg_model& G = Mo.leg[l];
    double o0[3], o1[3], o2[3], o3[3];
    for (int i = 0; i < 3; i++) {
      o0[i] = G.haa_xyz[i];
      o1[i] = o0[i] + G.hfe_xyz[i];
      o2[i] = o1[i] + G.kfe_xyz[i];
      o3[i] = o2[i] + G.foot_xyz[i];
    }
    add(G.shoulder, o0);
    add(G.upper, o1);
    add(G.lower, o2);
    add(G.foot, o3);
  }
  Y[0] = Y[1] = Y[2] = m;
  Y[3] = I[0];
  Y[4] = I[1];
  Y[5] = I[2];
}

extern "C" int qrw_create(const qrw_config* cfg, qrw_handle* out) {
  if (!cfg || !out) return fail(-1, "qrw_create: null argument");
  if (cfg->batch < 1) return fail(-1, "qrw_create: batch must be >= 1");
  if (cfg->n_steps < 1 || cfg->n_steps > qrw::kMpcMaxN)
    return fail(-1, "qrw_create: n_steps must be in 1..32 (16 horizon steps per wavefront, at most two wavefronts)");
  if (cfg->N_gait < cfg->n_steps) return fail(-1, "qrw_create: N_gait must be >= n_steps");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return fail(-2, "qrw_create: no HIP device (this library has no CPU path)");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(-2, "qrw_create: bad device ordinal");
  DeviceScope dev_scope__(cfg->device);
  qrw_handle h = new qrw_handle_s();
  h->cfg = *cfg;
  const size_t B = (size_t)cfg->batch;
  const int N = cfg->n_steps;
  // from here on a failure deletes the handle (never registered: its members free what they hold), then sets the error
  auto give_up = [&](const char* what, hipError_t e) { delete h; return fail(-10, what, e); };
  hipError_t e = hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    h->host_stream = nullptr;
    return give_up("qrw_create: hipStreamCreateWithFlags", e);
  }
  // every buffer starts zeroed (fills on host_stream, waited for at the end); the first failure is kept, what follows it is skipped
  const char* failed = nullptr;
  auto zeroed = [&](auto& buf, size_t count, const char* what) {
    if (e != hipSuccess) return;
    if ((e = buf.alloc(count)) == hipSuccess) e = buf.fill(0, h->host_stream);
    if (e != hipSuccess) failed = what;
  };
  zeroed(h->mpc_st, B * qrw::kMpcStItems * qrw::mpc_threads(N), "qrw_create: hipMalloc mpc_st");
  zeroed(h->mpc_gait, B * cfg->N_gait * 4, "qrw_create: hipMalloc mpc_gait");
  for (auto* b : {&h->mpc_flags, &h->mpc_iters, &h->mpc_status, &h->mpc_rho_updates, &h->mpc_order})
    zeroed(*b, B, "qrw_create: hipMalloc of a per-instance MPC counter");
  zeroed(h->mpc_ema, B, "qrw_create: hipMalloc mpc_ema");
  for (auto* b : {&h->mpc_rho, &h->mpc_pri, &h->mpc_dua}) zeroed(*b, B, "qrw_create: hipMalloc of a per-instance MPC residual");
  zeroed(h->mpc_prof, B * qrw::kMpcProfItems, "qrw_create: hipMalloc mpc_prof");
  if (e != hipSuccess) return give_up(failed, e);
  if (N > 16) {
    // round-robin time slicing of the solves of one call (mpc_kernel.hip, PRE): slices of QRW_PREEMPT_CHUNK iterations
    // (default 600, rounded up to a multiple of 200; 0 switches it off), used when the batch exceeds the resident slots
    const char* ce = getenv("QRW_PREEMPT_CHUNK");
    int chunk = ce ? atoi(ce) : 600;
    if (chunk > 0) {
      chunk = ((chunk + 199) / 200) * 200;
      hipDeviceProp_t prop;
      if ((e = hipGetDeviceProperties(&prop, cfg->device)) != hipSuccess) return give_up("qrw_create: hipGetDeviceProperties", e);
      h->pre_chunk = chunk;
      h->pre_cmax = (4000 + chunk - 1) / chunk;
      h->pre_min_batch = 2 * prop.multiProcessorCount;  // two two-wavefront instances per compute unit are resident
      h->pre_slots = h->pre_min_batch;
      if (const char* mb = getenv("QRW_PREEMPT_MIN_BATCH")) h->pre_min_batch = atoi(mb);  // tests: slice small batches too
      // priority levels of the parked solves (mpc_kernel.hip, PRE): QRW_PREEMPT_LEVELS = 1 is one FIFO (plain round robin),
      // the default 9 = first-slice FIFO + 8 levels of QRW_PREEMPT_BIN (200) predicted remaining iterations each (everything beyond
      // 1400 shares the first of them; 400 and 200 measure 91.4 k and 91.9 k steps/s on one box, the simulation 1.033 and 1.028)
      h->pre_levels = qrw::kPreMaxLevels;
      if (const char* le = getenv("QRW_PREEMPT_LEVELS")) h->pre_levels = atoi(le);
      if (h->pre_levels < 1) h->pre_levels = 1;
      if (h->pre_levels > qrw::kPreMaxLevels) h->pre_levels = qrw::kPreMaxLevels;
      if (const char* be = getenv("QRW_PREEMPT_BIN")) h->pre_bin = atoi(be);
      if (h->pre_bin < 25) h->pre_bin = 25;
      zeroed(h->pause_it, B, "qrw_create: hipMalloc pause_it");
      zeroed(h->pre_ctr, qrw::kPreCtrWords, "qrw_create: hipMalloc pre_ctr");
      zeroed(h->pre_queue, (size_t)h->pre_levels * B * (size_t)(h->pre_cmax > 1 ? h->pre_cmax - 1 : 1), "qrw_create: hipMalloc pre_queue");
      if (e != hipSuccess) return give_up(failed, e);
      // the launch's error word, mirrored where the host can read it without synchronising the device
      if ((e = h->pre_err.alloc()) != hipSuccess) return give_up("qrw_create: hipHostMalloc of the time-sliced launch's error word", e);
      // tests: the launch starts with its error word set, so every queue-fed workgroup leaves at once ("somebody gave up
      // already") and no parked solve is ever finished -- the state a queue that gave up leaves behind, without waiting 2 s for it
      if (const char* ge = getenv("QRW_PREEMPT_FORCE_GIVEUP")) h->force_giveup = (ge[0] == '1');
    }
  }
  // known answer through the instantiation of mpc_solve_kernel this handle's qrw_mpc_solve will launch
  if (const int rc = mpc_known_answer_gate("qrw_create", cfg->device, N, mpc_time_sliced(h) ? kKatSliced : kKatPlain)) {
    delete h;
    return rc;
  }
  zeroed(h->wbc_st, B * qrw::kWbcStItems, "qrw_create: hipMalloc wbc_st");
  zeroed(h->wbc_iters, B, "qrw_create: hipMalloc wbc_iters");
  zeroed(h->wbc_status, B, "qrw_create: hipMalloc wbc_status");
  zeroed(h->ctrl_st, B * (size_t)qrw::kCtrlStItems, "qrw_create: hipMalloc ctrl_st");
  zeroed(h->plan_st, B * (size_t)qrw::planner_state_items(cfg->N_gait), "qrw_create: hipMalloc plan_st");
  zeroed(h->est_st, B * (size_t)qrw::kEstStItems, "qrw_create: hipMalloc est_st");
  // staging: the largest host-API call moves M (324) + Jc (216) + ... per instance
  zeroed(h->stage, B * (size_t)(12 * (N + 1) + cfg->N_gait * 12 + 24 * N + 1024), "qrw_create: hipMalloc stage");
  zeroed(h->stage_i, B, "qrw_create: hipMalloc stage_i");
  if (e != hipSuccess) return give_up(failed, e);
  base_inertia_diag(h->Y);
  if (const char* e16 = getenv("QRW_WBC16")) h->wbc_lanes16 = (e16[0] != '0');
  // the zero fills above are complete before the caller can launch on any stream (this handle's own work only: no device-wide wait)
  if ((e = host_done(h)) != hipSuccess) return give_up("qrw_create sync", e);
  {
    std::lock_guard<std::mutex> lock(g_handles_mutex);
    g_handles.push_back(h);
  }
  *out = h;
  return 0;
}

extern "C" int qrw_destroy(qrw_handle h) {
  if (!h) return 0;
  {
    std::lock_guard<std::mutex> lock(g_handles_mutex);
    for (size_t i = 0; i < g_handles.size(); i++)
      if (g_handles[i] == h) { g_handles.erase(g_handles.begin() + i); break; }
  }
  DeviceScope dev_scope__(h->cfg.device);
  delete h;
  return 0;
}

// (the persistent solver state of the MPC and the WBC and the estimator's filters -- the Kalman filter's once a handle has
// allocated it, the joystick stage's likewise: not the diagnostics, planner, controller, staging or queue buffers)
extern "C" int64_t qrw_state_bytes(qrw_handle h) {
  if (!h) return 0;
  return (int64_t)(h->mpc_st.bytes + h->mpc_gait.bytes + h->mpc_flags.bytes + h->mpc_iters.bytes + h->mpc_status.bytes +
                   h->mpc_rho_updates.bytes + h->mpc_order.bytes + h->mpc_ema.bytes + h->mpc_rho.bytes + h->mpc_pri.bytes +
                   h->mpc_dua.bytes + h->wbc_st.bytes + h->wbc_iters.bytes + h->wbc_status.bytes + h->est_st.bytes + h->kal_st.bytes + h->sim_st.bytes + h->joy_st.bytes);
}

// what every MPC launch of a handle is told about its persistent state; xref / fsteps / out as the caller lays them out
static qrw::MpcArgs mpc_args(qrw_handle h, const double* d_xref, const double* d_fsteps, const int32_t* d_num_iter, int32_t num_iter_scalar,
                             double* d_out) {
  qrw::MpcArgs a;
  memset(&a, 0, sizeof(a));
  a.B = h->cfg.batch; a.N = h->cfg.n_steps; a.N_gait = h->cfg.N_gait; a.dt = h->cfg.dt_mpc;
  a.xref = d_xref; a.fsteps = d_fsteps; a.num_iter = d_num_iter; a.num_iter_scalar = num_iter_scalar;
  a.out = d_out; a.st = h->mpc_st; a.gait = h->mpc_gait; a.flags = h->mpc_flags; a.iters = h->mpc_iters;
  a.status = h->mpc_status; a.rho_out = h->mpc_rho; a.pri = h->mpc_pri; a.dua = h->mpc_dua;
  a.rho_updates = h->mpc_rho_updates;
  a.prof = h->mpc_prof;  // only diagnostic builds (-DQRW_PROFILE_PHASES, -DQRW_TRACE_RES, -DQRW_SEQ_STATS) write it
  a.order = h->mpc_have_order ? h->mpc_order.p : nullptr;
  return a;
}
// next launch's block order = this solve's iteration counts, longest first (same stream: ordered after the solve); false = launch failed
static bool mpc_reorder(qrw_handle h, hipStream_t stream) {
  static const int order_min = getenv("QRW_ORDER_MIN") ? atoi(getenv("QRW_ORDER_MIN")) : 1024;  // experiments only
  if (h->cfg.batch <= order_min) return true;
  if (qrw::mpc_order_launch(h->mpc_iters, h->mpc_ema, h->mpc_order, h->cfg.batch, stream) != 0) return false;
  h->mpc_have_order = true;
  return true;
}

extern "C" int qrw_mpc_solve(qrw_handle h, const double* d_xref, const double* d_fsteps, const int32_t* d_num_iter,
                             int32_t num_iter_scalar, double* d_out, void* stream) {
  QRW_ENTER(h, !d_xref || !d_fsteps || !d_out, "qrw_mpc_solve: null argument");
  const hipStream_t s = (hipStream_t)stream;
  if (h->pre_err.host) {
    // A time-sliced launch whose queue gave up (never expected) wrote its code into a host-mapped word: seen here, at the next
    // call that follows the failed launch's end, without a device sync.  Reported ONCE (this call launches nothing); the
    // unfinished instances' results of that launch are NaN, and the next solve starts them cold (mpc_kernel.hip, `aborted`).
    const unsigned code = __atomic_exchange_n(h->pre_err.host, 0u, __ATOMIC_ACQ_REL);
    if (code != 0u) {
      char msg[256];
      snprintf(msg, sizeof(msg), "qrw_mpc_solve: an earlier time-sliced MPC launch of this handle gave up (code %u: %s); its unfinished "
               "instances hold NaN results and restart cold at the next call", code,
               code == 2u ? "a priority level's queue overran" : code == 9u ? "forced by QRW_PREEMPT_FORCE_GIVEUP" : "a parked solve reserved for a taker workgroup did not arrive");
      return fail(-12, msg);
    }
  }
  qrw::MpcArgs a = mpc_args(h, d_xref, d_fsteps, d_num_iter, num_iter_scalar, d_out);
  if (mpc_time_sliced(h)) {
    // more instances than resident slots at N > 16: the solves are time-sliced round robin inside the launch (same results)
    a.pre_chunk = h->pre_chunk; a.pre_cmax = h->pre_cmax; a.pre_cap = h->cfg.batch * (h->pre_cmax - 1);
    a.pre_queue = h->pre_queue; a.pre_ctr = h->pre_ctr; a.pause_it = h->pause_it;
    a.pre_levels = h->pre_levels; a.pre_bin = h->pre_bin;
    HIP_OK(h->pre_queue.fill(0xFF, s), "qrw_mpc_solve: queue reset");  // (all pre_levels * pre_cap slots: the whole buffer)
    HIP_OK(h->pre_ctr.fill(0, s), "qrw_mpc_solve: counter reset");
    // a solve that a given-up queue left unfinished (never expected; qrw_mpc_get_stats reports it) must not leave the previous
    // call's numbers in the caller's buffer: NaN (all-ones bytes) until the finishing slice writes the result (~10 us per call)
    HIP_OK(hipMemsetAsync(d_out, 0xFF, (size_t)h->cfg.batch * 24 * (size_t)h->cfg.n_steps * sizeof(double), s), "qrw_mpc_solve: result prefill");
    if (h->force_giveup) {
      static const unsigned forced = 9u;
      HIP_OK(hipMemcpyAsync(h->pre_ctr + qrw::kPreErrWord, &forced, sizeof(unsigned), hipMemcpyHostToDevice, s), "qrw_mpc_solve: forced give-up");
    }
    debug_poison_lds(s);
    if (qrw::mpc_preemptive_launch(a, h->pre_slots, s) != 0 || qrw::mpc_pre_error_flush(h->pre_ctr, h->pre_err.dev, s) != 0)
      return fail(-11, "qrw_mpc_solve: kernel launch failed", hipGetLastError());
  } else {
    debug_poison_lds(s);
    if (qrw::mpc_launch(a, s) != 0) return fail(-11, "qrw_mpc_solve: kernel launch failed", hipGetLastError());
  }
  note_launch(h, kFamMpc, s);
  if (!mpc_reorder(h, s)) return fail(-11, "qrw_mpc_solve: order kernel launch failed", hipGetLastError());
  return 0;
}

extern "C" int qrw_mpc_solve_host(qrw_handle h, const double* h_xref, const double* h_fsteps, const int32_t* h_num_iter,
                                  int32_t num_iter_scalar, double* h_out) {
  QRW_ENTER_HOST(h, !h_xref || !h_fsteps || !h_out, "qrw_mpc_solve_host: null argument");
  const size_t B = h->cfg.batch, N = h->cfg.n_steps, Ng = h->cfg.N_gait;
  double* dx = h->stage;
  double* df = dx + B * 12 * (N + 1);
  double* dout = df + B * Ng * 12;
  HIP_OK(wait_family(h, kFamMpc), "qrw_mpc_solve_host: earlier solve of this handle");
  HIP_OK(h2d(h, dx, h_xref, B * 12 * (N + 1) * sizeof(double)), "qrw_mpc_solve_host: H2D xref");
  HIP_OK(h2d(h, df, h_fsteps, B * Ng * 12 * sizeof(double)), "qrw_mpc_solve_host: H2D fsteps");
  if (h_num_iter) HIP_OK(h2d(h, h->stage_i, h_num_iter, B * sizeof(int32_t)), "qrw_mpc_solve_host: H2D num_iter");
  int rc = qrw_mpc_solve(h, dx, df, h_num_iter ? h->stage_i.p : nullptr, num_iter_scalar, dout, (void*)h->host_stream);
  if (rc) return rc;
  return read_back(h, kFamNone, "qrw_mpc_solve_host: D2H result", {{h_out, dout, B * 24 * N * sizeof(double)}});
}

extern "C" int qrw_mpc_solve_sequence(qrw_handle h, int32_t K, const double* d_xref, const double* d_fsteps, int32_t first_num_iter,
                                      double* d_out, int32_t* d_iters, void* stream) {
  QRW_ENTER(h, !d_xref || !d_fsteps || !d_out || K < 1, "qrw_mpc_solve_sequence: bad argument");
  const hipStream_t s = (hipStream_t)stream;
  // the SEQ instantiation's known answer, once per process, device and horizon
  if (const int rc = mpc_known_answer_gate("qrw_mpc_solve_sequence", h->cfg.device, h->cfg.n_steps, kKatSequence)) return rc;
  const size_t need = (size_t)K * (size_t)h->cfg.batch;
  if (need > (size_t)0x7fffffff) return fail(-1, "qrw_mpc_solve_sequence: K * batch too large");
  if (need > h->seq_queue.count()) {  // grown on demand (first call / longer sequence), never on a steady-state call
    HIP_OK(hipStreamSynchronize(s), "qrw_mpc_solve_sequence sync");
    HIP_OK(h->seq_queue.alloc(need), "qrw_mpc_solve_sequence: hipMalloc queue");
  }
  // (each on its own: a call that failed half-way is retried from where it failed; the kernel initialises all three)
  if (!h->seq_ctr) HIP_OK(h->seq_ctr.alloc(qrw::kSeqQctrWords), "qrw_mpc_solve_sequence: hipMalloc counters");
  if (!h->seq_first) HIP_OK(h->seq_first.alloc(h->cfg.batch), "qrw_mpc_solve_sequence: hipMalloc first tasks");
  if (!h->seq_hot) HIP_OK(h->seq_hot.alloc(h->cfg.batch), "qrw_mpc_solve_sequence: hipMalloc hot flags");
  if (!h->seq_groups) {
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, h->cfg.device), "qrw_mpc_solve_sequence: hipGetDeviceProperties");
    // resident workgroups: one 512-register wavefront per SIMD (N <= 16: 4 workgroups per CU; N > 16: 2 of two wavefronts).
    // Only a scheduling hint: the first seq_groups workgroups take call 0 of the seq_groups longest-ranked instances by
    // index instead of through the queues.  On a CU-masked stream (or beside another stream group) fewer workgroups are
    // resident at a time; the dealt ones then simply start in several rounds.  What forward progress does rest on is that
    // workgroups START IN INDEX ORDER (every workgroup with a dealt task starts before any queue-fed one can hold the
    // last free slot) -- how the hardware dispatcher works, and what the one-call kernel's longest-first order already
    // assumes; tests/test_gpu_mpc.py runs a sequence on a masked stream beside a second stream to pin it.
    h->seq_groups = prop.multiProcessorCount * (h->cfg.n_steps <= 16 ? 4 : 2);
  }
  qrw::MpcArgs a = mpc_args(h, d_xref, d_fsteps, nullptr, first_num_iter, d_out);
  a.seq_K = K; a.queue = h->seq_queue; a.qctr = h->seq_ctr; a.seq_hot = h->seq_hot; a.seq_first = h->seq_first; a.seq_iters = d_iters;
  a.seq_groups = h->seq_groups < h->cfg.batch ? h->seq_groups : h->cfg.batch;
  // a task that never runs (queue give-up, see qrw_mpc_sequence_error) must not leave plausible numbers behind: results
  // are pre-filled with NaN (all-ones bytes) and the iteration counts with -1
  HIP_OK(hipMemsetAsync(d_out, 0xFF, need * 24 * (size_t)h->cfg.n_steps * sizeof(double), s), "qrw_mpc_solve_sequence prefill");
  if (d_iters) HIP_OK(hipMemsetAsync(d_iters, 0xFF, need * sizeof(int32_t), s), "qrw_mpc_solve_sequence prefill iters");
  debug_poison_lds(s);
  if (qrw::mpc_sequence_launch(a, s) != 0) return fail(-11, "qrw_mpc_solve_sequence: kernel launch failed", hipGetLastError());
  note_launch(h, kFamMpc, s);
  if (!mpc_reorder(h, s)) return fail(-11, "qrw_mpc_solve_sequence: order kernel launch failed", hipGetLastError());
  return 0;
}

extern "C" int qrw_mpc_sequence_error(qrw_handle h, int32_t* timed_out) {
  QRW_ENTER_HOST(h, !timed_out, "qrw_mpc_sequence_error: null argument");
  *timed_out = 0;
  if (!h->seq_ctr) return 0;
  // like every other getter: waits for this handle's last MPC launch (the sequence in flight), not for the device
  unsigned c[qrw::kSeqQctrWords];
  if (const int rc = read_back(h, kFamMpc, "qrw_mpc_sequence_error", {{c, h->seq_ctr, sizeof(c)}})) return rc;
  *timed_out = (int32_t)c[qrw::kSeqErrWord];
  if (getenv("QRW_SEQ_STATS")) {
    fprintf(stderr, "qrw sequence: levels taken/queued");
    for (int l = 0; l < qrw::kSeqErrWord / 16; l++) fprintf(stderr, " %u/%u", c[16 * l], c[16 * l + 1]);
    fprintf(stderr, ", looking-for-work ticks (100 MHz, summed) %u\n", c[qrw::kSeqErrWord + 1]);
  }
  return 0;
}

extern "C" int qrw_mpc_copy_iters(qrw_handle h, int32_t* d_iters, void* stream) {
  QRW_ENTER(h, !d_iters, "qrw_mpc_copy_iters: null argument");
  HIP_OK(hipMemcpyAsync(d_iters, h->mpc_iters, h->mpc_iters.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream), "qrw_mpc_copy_iters");
  return 0;
}

extern "C" int qrw_mpc_get_gait(qrw_handle h, int32_t b, double* h_gait, double* h_Sgait) {
  QRW_ENTER_HOST(h, b < 0 || b >= h->cfg.batch, "qrw_mpc_get_gait: bad argument");
  const int N = h->cfg.n_steps, Ng = h->cfg.N_gait, T = qrw::mpc_threads(N);
  std::vector<int> g(Ng * 4);
  std::vector<double> s(3 * T);
  if (const int rc = read_back(h, kFamMpc, "qrw_mpc_get_gait",
                               {{h_gait ? g.data() : nullptr, h->mpc_gait + (size_t)b * Ng * 4, g.size() * sizeof(int)},
                                {h_Sgait ? s.data() : nullptr, h->mpc_st + ((size_t)b * qrw::kMpcStItems + qrw::kStS) * T, s.size() * sizeof(double)}}))
    return rc;
  if (h_gait)
    for (int i = 0; i < Ng * 4; i++) h_gait[i] = (double)g[i];
  if (h_Sgait)
    for (int k = 0; k < N; k++)
      for (int j = 0; j < 4; j++)
        for (int t = 0; t < 3; t++) h_Sgait[12 * k + 3 * j + t] = s[t * T + 4 * k + j];
  return 0;
}

extern "C" int qrw_mpc_get_stats(qrw_handle h, int32_t* h_iters, int32_t* h_status, double* h_rho, double* h_pri_res,
                                 double* h_dua_res) {
  QRW_ENTER_HOST(h, false, "qrw_mpc_get_stats: null handle");
  const size_t B = h->cfg.batch;
  // this handle's last solve only: another handle's launch in flight is not waited for
  HIP_OK(wait_family(h, kFamMpc), "qrw_mpc_get_stats: earlier solve of this handle");
  if (h->pre_ctr) {  // a time-sliced launch whose queue gave up (never expected) left solves unfinished: say so, loudly
    unsigned c[qrw::kPreCtrWords];
    if (const int rc = read_back(h, kFamNone, "qrw_mpc_get_stats: D2H pre_ctr", {{c, h->pre_ctr, sizeof(c)}})) return rc;
    if (c[qrw::kPreErrWord] != 0) return fail(-12, "qrw_mpc_get_stats: the last time-sliced MPC launch left solves unfinished (a parked solve did not reach its taker "
                                     "within 2 s, or a queue overran); results of that call are incomplete");
  }
  return read_back(h, kFamNone, "qrw_mpc_get_stats",
                   {{h_iters, h->mpc_iters, B * sizeof(int)}, {h_status, h->mpc_status, B * sizeof(int)}, {h_rho, h->mpc_rho, B * sizeof(double)},
                    {h_pri_res, h->mpc_pri, B * sizeof(double)}, {h_dua_res, h->mpc_dua, B * sizeof(double)}});
}

// Diagnostic: bookkeeping of the last time-sliced qrw_mpc_solve (N > 16, batch above the resident slots; zeros otherwise).
extern "C" int qrw_mpc_get_slice_stats(qrw_handle h, int32_t* levels, int32_t* chunk, uint32_t* h_parks_per_level /* [9] */,
                                       uint32_t* h_takers, uint32_t* h_finished) {
  QRW_ENTER_HOST(h, !levels || !chunk || !h_parks_per_level || !h_takers || !h_finished, "qrw_mpc_get_slice_stats: null argument");
  *levels = h->pre_ctr ? h->pre_levels : 0;
  *chunk = h->pre_ctr ? h->pre_chunk : 0;
  for (int l = 0; l < qrw::kPreMaxLevels; l++) h_parks_per_level[l] = 0;
  *h_takers = *h_finished = 0;
  if (!h->pre_ctr) return 0;
  unsigned c[qrw::kPreCtrWords];
  if (const int rc = read_back(h, kFamMpc, "qrw_mpc_get_slice_stats", {{c, h->pre_ctr, sizeof(c)}})) return rc;
  for (int l = 0; l < qrw::kPreMaxLevels; l++) h_parks_per_level[l] = c[qrw::kPreLevelWord + 2 * l + 1];
  *h_takers = c[qrw::kPreTicketWord];
  *h_finished = c[qrw::kPreDoneWord];
  return 0;
}

extern "C" int qrw_mpc_get_order(qrw_handle h, int32_t* h_order, float* h_ema, int32_t* has_order) {
  QRW_ENTER_HOST(h, !has_order, "qrw_mpc_get_order: null argument");
  HIP_OK(wait_family(h, kFamMpc), "qrw_mpc_get_order sync");
  *has_order = h->mpc_have_order ? 1 : 0;
  return read_back(h, kFamNone, "qrw_mpc_get_order", {{h_order, h->mpc_order, h->mpc_order.bytes}, {h_ema, h->mpc_ema, h->mpc_ema.bytes}});
}

extern "C" int qrw_mpc_get_state(qrw_handle h, int32_t b, double* h_x, double* h_z, double* h_y, double* h_D,
                                 double* h_E, double* h_c) {
  QRW_ENTER_HOST(h, b < 0 || b >= h->cfg.batch, "qrw_mpc_get_state: bad argument");
  const int N = h->cfg.n_steps, T = qrw::mpc_threads(N);
  std::vector<double> s((size_t)qrw::kMpcStItems * T);
  if (const int rc = read_back(h, kFamMpc, "qrw_mpc_get_state", {{s.data(), h->mpc_st + (size_t)b * qrw::kMpcStItems * T, s.size() * sizeof(double)}}))
    return rc;
  auto at = [&](int item, int k, int j) { return s[(size_t)item * T + 4 * k + j]; };
  for (int k = 0; k < N; k++)
    for (int j = 0; j < 4; j++) {
      for (int t = 0; t < 3; t++) {
        const int i = 12 * k + 3 * j + t;
        if (h_x) { h_x[i] = at(qrw::kStXX + t, k, j); h_x[12 * N + i] = at(qrw::kStXF + t, k, j); }
        if (h_D) { h_D[i] = at(qrw::kStDX + t, k, j); h_D[12 * N + i] = at(qrw::kStDF + t, k, j); }
        if (h_z) { h_z[i] = at(qrw::kStZD + t, k, j); h_z[12 * N + i] = 0.0; }
        if (h_y) { h_y[i] = at(qrw::kStYD + t, k, j); h_y[12 * N + i] = at(qrw::kStYS + t, k, j); }
        if (h_E) { h_E[i] = at(qrw::kStED + t, k, j); h_E[12 * N + i] = at(qrw::kStES + t, k, j); }
      }
      for (int c = 0; c < 5; c++) {
        const int r = 24 * N + 20 * k + 5 * j + c;
        if (h_z) h_z[r] = at(qrw::kStZC + c, k, j);
        if (h_y) h_y[r] = at(qrw::kStYC + c, k, j);
        if (h_E) h_E[r] = at(qrw::kStEC + c, k, j);
      }
    }
  if (h_c) *h_c = s[(size_t)qrw::kStC * T];
  return 0;
}

// Diagnostic (profiling builds only, -DQRW_PROFILE_PHASES): per-instance shader-clock totals of the MPC kernel phases.
extern "C" int qrw_mpc_get_phase_cycles(qrw_handle h, double* h_prof /* [B][10] */) {
  QRW_ENTER_HOST(h, !h_prof, "qrw_mpc_get_phase_cycles: null argument");
  return read_back(h, kFamMpc, "qrw_mpc_get_phase_cycles", {{h_prof, h->mpc_prof, h->mpc_prof.bytes}});
}

// ------------------------------------------------------------------ WBC
static void wbc_common(qrw_handle h, qrw::WbcArgs& a) {
  memset(&a, 0, sizeof(a));
  a.B = h->cfg.batch;
  a.dt = h->cfg.dt_wbc;
  a.st = h->wbc_st;
  a.iters = h->wbc_iters;
  a.status = h->wbc_status;
  for (int i = 0; i < 6; i++) a.Y[i] = h->Y[i];
  a.lanes16 = h->wbc_lanes16;
}
// the full WBC step (mode 0) on the caller's device buffers
static qrw::WbcArgs wbc_step_args(qrw_handle h, const double* d_q, const double* d_dq, const double* d_f_cmd, const double* d_contacts,
                                  const double* d_pgoals, const double* d_vgoals, const double* d_agoals, double* d_tau_ff, double* d_qdes,
                                  double* d_vdes, double* d_f_with_delta, double* d_ddq_res, double* d_feet) {
  qrw::WbcArgs a;
  wbc_common(h, a);
  a.mode = 0;
  a.q = d_q; a.dq = d_dq; a.f_cmd = d_f_cmd; a.contacts = d_contacts;
  a.pgoals = d_pgoals; a.vgoals = d_vgoals; a.agoals = d_agoals;
  a.tau_ff = d_tau_ff; a.qdes = d_qdes; a.vdes = d_vdes; a.f_with_delta = d_f_with_delta;
  a.ddq_res = d_ddq_res; a.feet = d_feet;
  return a;
}
static int wbc_step_launch(qrw_handle h, const qrw::WbcArgs& a, hipStream_t stream, const char* launch_failed) {
  debug_poison_lds(stream);
  if (qrw::wbc_launch(a, stream) != 0) return fail(-11, launch_failed, hipGetLastError());
  note_launch(h, kFamWbc, stream);
  return 0;
}

extern "C" int qrw_wbc_set_lanes(qrw_handle h, int32_t lanes) {
  if (!h || (lanes != 4 && lanes != 16)) return fail(-1, "qrw_wbc_set_lanes: lanes must be 4 or 16");
  h->wbc_lanes16 = (lanes == 16);
  return 0;
}

extern "C" int qrw_wbc_compute(qrw_handle h, const double* d_q, const double* d_dq, const double* d_f_cmd,
                               const double* d_contacts, const double* d_pgoals, const double* d_vgoals,
                               const double* d_agoals, double* d_tau_ff, double* d_qdes, double* d_vdes,
                               double* d_f_with_delta, double* d_ddq_res, double* d_feet, void* stream) {
  QRW_ENTER(h, !d_q || !d_dq || !d_f_cmd || !d_contacts || !d_pgoals || !d_vgoals || !d_agoals, "qrw_wbc_compute: null input");
  const qrw::WbcArgs a = wbc_step_args(h, d_q, d_dq, d_f_cmd, d_contacts, d_pgoals, d_vgoals, d_agoals, d_tau_ff, d_qdes, d_vdes,
                                       d_f_with_delta, d_ddq_res, d_feet);
  return wbc_step_launch(h, a, (hipStream_t)stream, "qrw_wbc_compute: kernel launch failed");
}

extern "C" int qrw_wbc_compute_result(qrw_handle h, const double* d_q, const double* d_dq, const double* d_f_cmd,
                                      const double* d_contacts, const double* d_pgoals, const double* d_vgoals,
                                      const double* d_agoals, double* d_tau_ff, double* d_qdes, double* d_vdes,
                                      double* d_f_with_delta, double* d_ddq_res, double* d_feet, const double* d_q_filt,
                                      const double* d_v_secu, double* d_result, int32_t* d_error_flag, void* stream) {
  QRW_ENTER(h, !d_q || !d_dq || !d_f_cmd || !d_contacts || !d_pgoals || !d_vgoals || !d_agoals || !d_q_filt || !d_v_secu || !d_result,
            "qrw_wbc_compute_result: null argument");
  qrw::WbcArgs a = wbc_step_args(h, d_q, d_dq, d_f_cmd, d_contacts, d_pgoals, d_vgoals, d_agoals, d_tau_ff, d_qdes, d_vdes,
                                 d_f_with_delta, d_ddq_res, d_feet);
  a.c_cs = h->ctrl_st; a.c_qfilt = d_q_filt; a.c_vsecu = d_v_secu; a.c_result = d_result; a.c_err = d_error_flag;
  return wbc_step_launch(h, a, (hipStream_t)stream, "qrw_wbc_compute_result: kernel launch failed");
}

namespace {
struct Stager {
  qrw_handle h;
  size_t off = 0;
  bool ok = true;
  explicit Stager(qrw_handle hh) : h(hh) {}
  double* in(const double* src, size_t n) {
    double* d = out(n);
    if (d && src && h2d(h, d, src, n * sizeof(double)) != hipSuccess) ok = false;
    return d;
  }
  double* out(size_t n) {
    if (off + n > h->stage.count()) { ok = false; return nullptr; }
    double* d = h->stage + off;
    off += n;
    return d;
  }
  // (asynchronous on the handle's host stream: the caller ends with host_done)
  bool back(double* dst, const double* d, size_t n) {
    if (!dst) return true;
    return d2h(h, dst, d, n * sizeof(double)) == hipSuccess;
  }
};
}  // namespace

extern "C" int qrw_wbc_compute_host(qrw_handle h, const double* h_q, const double* h_dq, const double* h_f_cmd,
                                    const double* h_contacts, const double* h_pgoals, const double* h_vgoals,
                                    const double* h_agoals, double* h_tau_ff, double* h_qdes, double* h_vdes,
                                    double* h_f_with_delta, double* h_ddq_res, double* h_feet) {
  QRW_ENTER_HOST(h, false, "qrw_wbc_compute_host: null handle");
  const size_t B = h->cfg.batch;
  HIP_OK(wait_family(h, kFamWbc), "qrw_wbc_compute_host: earlier WBC step of this handle");
  Stager s(h);
  double *q = s.in(h_q, B * 19), *dq = s.in(h_dq, B * 18), *f = s.in(h_f_cmd, B * 12), *c = s.in(h_contacts, B * 4);
  double *pg = s.in(h_pgoals, B * 12), *vg = s.in(h_vgoals, B * 12), *ag = s.in(h_agoals, B * 12);
  double *tau = s.out(B * 12), *qd = s.out(B * 19), *vd = s.out(B * 18), *fw = s.out(B * 12), *dd = s.out(B * 6),
         *ft = s.out(B * 36);
  if (!s.ok) return fail(-12, "qrw_wbc_compute_host: staging failed");
  int rc = qrw_wbc_compute(h, q, dq, f, c, pg, vg, ag, tau, qd, vd, fw, dd, ft, (void*)h->host_stream);
  if (rc) return rc;
  if (!(s.back(h_tau_ff, tau, B * 12) && s.back(h_qdes, qd, B * 19) && s.back(h_vdes, vd, B * 18) &&
        s.back(h_f_with_delta, fw, B * 12) && s.back(h_ddq_res, dd, B * 6) && s.back(h_feet, ft, B * 36)))
    return fail(-12, "qrw_wbc_compute_host: D2H failed");
  HIP_OK(host_done(h), "qrw_wbc_compute_host sync");
  return 0;
}

extern "C" int qrw_wbc_get_stats(qrw_handle h, int32_t* h_iters, int32_t* h_status, double* h_rho,
                                 double* h_k_since_contact) {
  QRW_ENTER_HOST(h, false, "qrw_wbc_get_stats: null handle");
  const size_t B = h->cfg.batch;
  std::vector<double> s((h_rho || h_k_since_contact) ? B * qrw::kWbcStItems : 0);
  if (const int rc = read_back(h, kFamWbc, "qrw_wbc_get_stats",
                               {{h_iters, h->wbc_iters, B * sizeof(int)}, {h_status, h->wbc_status, B * sizeof(int)},
                                {s.empty() ? nullptr : s.data(), h->wbc_st, s.size() * sizeof(double)}}))
    return rc;
  for (size_t b = 0; b < B && !s.empty(); b++) {
    if (h_rho) h_rho[b] = s[b * qrw::kWbcStItems + qrw::kWsRho];
    if (h_k_since_contact)
      for (int i = 0; i < 4; i++) h_k_since_contact[b * 4 + i] = s[b * qrw::kWbcStItems + qrw::kWsKsc + i];
  }
  return 0;
}

extern "C" int qrw_fixed_feet_host(qrw_handle h, const double* h_q12, const double* h_dq12, double* h_posf, double* h_vf,
                                   double* h_wf, double* h_af, double* h_Jf) {
  QRW_ENTER_HOST(h, !h_q12 || !h_dq12, "qrw_fixed_feet_host: null argument");
  const size_t B = h->cfg.batch;
  Stager s(h);
  qrw::WbcArgs a;
  wbc_common(h, a);
  a.mode = 1;
  a.in0 = s.in(h_q12, B * 12); a.in1 = s.in(h_dq12, B * 12);
  a.out0 = s.out(B * 12); a.out1 = s.out(B * 12); a.out2 = s.out(B * 12); a.out3 = s.out(B * 12); a.out4 = s.out(B * 144);
  if (!s.ok) return fail(-12, "qrw_fixed_feet_host: staging failed");
  if (qrw::wbc_launch(a, h->host_stream) != 0) return fail(-11, "qrw_fixed_feet_host: launch failed", hipGetLastError());
  if (!(s.back(h_posf, a.out0, B * 12) && s.back(h_vf, a.out1, B * 12) && s.back(h_wf, a.out2, B * 12) &&
        s.back(h_af, a.out3, B * 12) && s.back(h_Jf, a.out4, B * 144)))
    return fail(-12, "qrw_fixed_feet_host: D2H failed");
  HIP_OK(host_done(h), "qrw_fixed_feet_host sync");
  return 0;
}

extern "C" int qrw_invkin_host(qrw_handle h, const double* h_contacts, const double* h_goals, const double* h_vgoals,
                               const double* h_agoals, const double* h_posf, const double* h_vf, const double* h_wf,
                               const double* h_af, const double* h_Jf, double* h_ddq, double* h_dq_cmd,
                               double* h_q_step) {
  QRW_ENTER_HOST(h, false, "qrw_invkin_host: null handle");
  const size_t B = h->cfg.batch;
  Stager s(h);
  qrw::WbcArgs a;
  wbc_common(h, a);
  a.mode = 2;
  a.in0 = s.in(h_contacts, B * 4); a.in1 = s.in(h_goals, B * 12); a.in2 = s.in(h_vgoals, B * 12);
  a.in3 = s.in(h_agoals, B * 12); a.in4 = s.in(h_posf, B * 12); a.in5 = s.in(h_vf, B * 12);
  a.in6 = s.in(h_wf, B * 12); a.in7 = s.in(h_af, B * 12); a.in8 = s.in(h_Jf, B * 144);
  a.out0 = s.out(B * 12); a.out1 = s.out(B * 12); a.out2 = s.out(B * 12);
  if (!s.ok) return fail(-12, "qrw_invkin_host: staging failed");
  if (qrw::wbc_launch(a, h->host_stream) != 0) return fail(-11, "qrw_invkin_host: launch failed", hipGetLastError());
  if (!(s.back(h_ddq, a.out0, B * 12) && s.back(h_dq_cmd, a.out1, B * 12) && s.back(h_q_step, a.out2, B * 12)))
    return fail(-12, "qrw_invkin_host: D2H failed");
  HIP_OK(host_done(h), "qrw_invkin_host sync");
  return 0;
}

extern "C" int qrw_qpwbc_host(qrw_handle h, const double* h_M, const double* h_Jc, const double* h_f_cmd,
                              const double* h_RNEA, double* h_f_res, double* h_ddq_res, double* h_H) {
  QRW_ENTER_HOST(h, !h_M || !h_Jc || !h_f_cmd || !h_RNEA, "qrw_qpwbc_host: null argument");
  const size_t B = h->cfg.batch;
  HIP_OK(wait_family(h, kFamWbc), "qrw_qpwbc_host: earlier WBC step of this handle");
  Stager s(h);
  qrw::WbcArgs a;
  wbc_common(h, a);
  a.mode = 3;
  a.in0 = s.in(h_M, B * 324); a.in1 = s.in(h_Jc, B * 216); a.in2 = s.in(h_f_cmd, B * 12); a.in3 = s.in(h_RNEA, B * 6);
  a.out0 = s.out(B * 12); a.out1 = s.out(B * 6); a.out2 = h_H ? s.out(B * 144) : nullptr;
  // M[:6,:6] diagonal in every instance (what scripts/QP_WBC.py:93 hands over): the kernel inverts it in place; otherwise the
  // general pseudoInverse<> of include/qrw/InvKin.hpp:60-66 is computed first (pinv6_kernel)
  bool diagonal = true;
  for (size_t b = 0; b < B && diagonal; b++)
    for (int i = 0; i < 6 && diagonal; i++)
      for (int c = 0; c < 6; c++)
        if (i != c && h_M[b * 324 + i * 18 + c] != 0.0) { diagonal = false; break; }
  double* d_yinv = nullptr;
  if (!diagonal) d_yinv = s.out(B * 36);
  if (!s.ok) return fail(-12, "qrw_qpwbc_host: staging failed");
  if (d_yinv) {
    if (qrw::pinv6_launch(a.in0, d_yinv, (int)B, h->host_stream) != 0) return fail(-11, "qrw_qpwbc_host: launch failed", hipGetLastError());
    a.in4 = d_yinv;
  }
  if (qrw::wbc_launch(a, h->host_stream) != 0) return fail(-11, "qrw_qpwbc_host: launch failed", hipGetLastError());
  note_launch(h, kFamWbc, h->host_stream);
  if (!(s.back(h_f_res, a.out0, B * 12) && s.back(h_ddq_res, a.out1, B * 6) && s.back(h_H, a.out2, B * 144)))
    return fail(-12, "qrw_qpwbc_host: D2H failed");
  HIP_OK(host_done(h), "qrw_qpwbc_host sync");
  return 0;
}

extern "C" int qrw_get_base_inertia_diag(qrw_handle h, double* h_Y6) {
  QRW_ENTER(h, !h_Y6, "qrw_get_base_inertia_diag: null argument");
  for (int i = 0; i < 6; i++) h_Y6[i] = h->Y[i];
  return 0;
}

// ------------------------------------------------------------------ planners
static void planner_common(qrw_handle h, qrw::PlannerArgs& a) {
  memset(&a, 0, sizeof(a));
  a.B = h->cfg.batch; a.n_steps = h->cfg.n_steps; a.N_gait = h->cfg.N_gait; a.k_mpc = h->pcfg.k_mpc;
  a.dt_mpc = h->cfg.dt_mpc; a.dt_wbc = h->cfg.dt_wbc; a.T_gait = h->cfg.T_gait; a.T_mpc = h->cfg.dt_mpc * h->cfg.n_steps;
  a.h_ref = h->pcfg.h_ref; a.k_feedback = 0.03; a.g = 9.81; a.L = 0.155;  // FootstepPlanner.cpp:5-7
  a.max_height = h->pcfg.max_height; a.lock_time = h->pcfg.lock_time;
  for (int i = 0; i < 12; i++) { a.shoulders[i] = h->pcfg.shoulders[i]; a.init_target[i] = h->pcfg.init_target[i]; a.init_pos[i] = h->pcfg.init_foot_pos[i]; }
  a.ps = h->plan_st;
  a.q_ld = 7;
}
// iteration k of the planners (gait, footsteps, trajectories, state) on the caller's device buffers
static qrw::PlannerArgs planner_step_args(qrw_handle h, int32_t k, const double* d_q7, int32_t q_ld, const double* d_hv, const double* d_vref,
                                          const int32_t* d_code, int32_t code_scalar, double* d_xref, double* d_fsteps, double* d_gait,
                                          double* d_target, double* d_feet_pva, double* d_contacts) {
  qrw::PlannerArgs a;
  planner_common(h, a);
  a.mode = qrw::kPlanGait | qrw::kPlanFootsteps | qrw::kPlanTraj | qrw::kPlanState;
  a.k = k;
  a.refresh = ((k % a.k_mpc) == 0 && k != 0) ? 1 : 0;     // scripts/Controller.py:225
  a.k_footsteps = a.k_mpc - k % a.k_mpc;                  // scripts/Controller.py:226
  a.q7 = d_q7; a.q_ld = q_ld; a.hv = d_hv; a.vref = d_vref; a.code = d_code; a.code_scalar = code_scalar;
  a.xref = d_xref; a.fsteps = d_fsteps; a.gait = d_gait; a.target = d_target; a.feet_pva = d_feet_pva;
  a.contacts = d_contacts;
  return a;
}

extern "C" int qrw_gait_table_fits(qrw_handle h) {  // (host arithmetic on the handle's configuration: no device is touched)
  if (!h) return fail(-1, "qrw_gait_table_fits: null handle");
  return qrw::gait_table_fits(h->cfg.N_gait, h->cfg.n_steps, h->cfg.T_gait, h->cfg.dt_mpc) ? 1 : 0;
}

extern "C" int qrw_planner_init(qrw_handle h, const qrw_planner_config* pc, void* stream) {
  QRW_ENTER(h, !pc, "qrw_planner_init: null argument");
  if (pc->k_mpc < 1) return fail(-1, "qrw_planner_init: k_mpc must be >= 1");
  if (h->cfg.N_gait > 63) return fail(-1, "qrw_planner_init: N_gait must be <= 63 (gait matrices are 64-bit column masks)");
  // Gait::initialize throws when the matrices are too small (src/Gait.cpp:30-31).  The size rule of csrc/gait_masks.h -- every
  // gait a code can select fits the table -- is tested HERE, ahead of the launch: the kernels' mask arithmetic relies on it
  // (a table it refuses could keep their zero-row searches from ending) and does not test it again.
  if (!qrw::gait_table_fits(h->cfg.N_gait, h->cfg.n_steps, h->cfg.T_gait, h->cfg.dt_mpc))
    return fail(-3, "Sizes of matrices are too small for considered durations. Increase N_gait in config file.");
  h->pcfg = *pc;
  qrw::PlannerArgs a;
  planner_common(h, a);
  a.mode = qrw::kPlanInit;
  if (qrw::planner_launch(a, (hipStream_t)stream) != 0) return fail(-11, "qrw_planner_init: launch failed", hipGetLastError());
  note_launch(h, kFamPlan, (hipStream_t)stream);
  h->plan_ready = true;
  return 0;
}

extern "C" int qrw_planner_step(qrw_handle h, int32_t k, const double* d_q7, int32_t q_ld, const double* d_hv,
                                const double* d_vref, const int32_t* d_code, int32_t code_scalar, double* d_xref,
                                double* d_fsteps, double* d_gait, double* d_target, double* d_feet_pva,
                                double* d_contacts, void* stream) {
  QRW_ENTER(h, !h->plan_ready, "qrw_planner_step: planner not initialised");
  if (!d_q7 || !d_hv || !d_vref) return fail(-1, "qrw_planner_step: null input");
  if (q_ld < 7) return fail(-1, "qrw_planner_step: q_ld must be at least 7");
  const qrw::PlannerArgs a = planner_step_args(h, k, d_q7, q_ld, d_hv, d_vref, d_code, code_scalar, d_xref, d_fsteps, d_gait, d_target,
                                               d_feet_pva, d_contacts);
  if (qrw::planner_launch(a, (hipStream_t)stream) != 0) return fail(-11, "qrw_planner_step: launch failed", hipGetLastError());
  note_launch(h, kFamPlan, (hipStream_t)stream);
  return 0;
}

extern "C" int qrw_planner_call_host(qrw_handle h, int32_t mode, int32_t k, int32_t k_footsteps, int32_t refresh,
                                     const double* h_q7, const double* h_v6, const double* h_vref6, int32_t code,
                                     const double* h_target_in, double z_average, double* h_xref, double* h_fsteps,
                                     double* h_gait, double* h_target, double* h_feet_pva) {
  QRW_ENTER_HOST(h, !h->plan_ready, "qrw_planner_call_host: planner not initialised");
  const size_t B = h->cfg.batch, N = h->cfg.n_steps, Ng = h->cfg.N_gait;
  HIP_OK(wait_family(h, kFamPlan), "qrw_planner_call_host: earlier planner step of this handle");
  Stager s(h);
  qrw::PlannerArgs a;
  planner_common(h, a);
  a.mode = mode & ~qrw::kPlanInit;
  a.k = k; a.k_footsteps = k_footsteps; a.refresh = refresh; a.code_scalar = code; a.z_average = z_average;
  a.q7 = h_q7 ? s.in(h_q7, B * 7) : nullptr;
  a.hv = h_v6 ? s.in(h_v6, B * 6) : nullptr;
  a.vref = h_vref6 ? s.in(h_vref6, B * 6) : nullptr;
  a.target_in = h_target_in ? s.in(h_target_in, B * 12) : nullptr;
  a.xref = h_xref ? s.out(B * 12 * (N + 1)) : nullptr;
  a.fsteps = h_fsteps ? s.out(B * Ng * 12) : nullptr;
  a.gait = h_gait ? s.out(B * Ng * 4) : nullptr;
  a.target = h_target ? s.out(B * 12) : nullptr;
  a.feet_pva = h_feet_pva ? s.out(B * 36) : nullptr;
  if (!s.ok) return fail(-12, "qrw_planner_call_host: staging failed");
  if (qrw::planner_launch(a, h->host_stream) != 0) return fail(-11, "qrw_planner_call_host: launch failed", hipGetLastError());
  note_launch(h, kFamPlan, h->host_stream);
  if (!(s.back(h_xref, a.xref, B * 12 * (N + 1)) && s.back(h_fsteps, a.fsteps, B * Ng * 12) && s.back(h_gait, a.gait, B * Ng * 4) &&
        s.back(h_target, a.target, B * 12) && s.back(h_feet_pva, a.feet_pva, B * 36)))
    return fail(-12, "qrw_planner_call_host: D2H failed");
  HIP_OK(host_done(h), "qrw_planner_call_host sync");
  return 0;
}

extern "C" int qrw_planner_get_host(qrw_handle h, int32_t which, int32_t b, int32_t count, double* h_out) {
  QRW_ENTER_HOST(h, !h_out || b < 0 || b >= h->cfg.batch || count < 1, "qrw_planner_get_host: bad argument");
  const int off = qrw::planner_item_offset(h->cfg.N_gait, which);
  const size_t B = h->cfg.batch;
  const bool gait = which >= 0 && which <= 2;  // a gait matrix: stored as four 64-bit column masks, returned as N_gait x 4 doubles
  HIP_OK(wait_family(h, kFamPlan), "qrw_planner_get_host: earlier planner step of this handle");
  if (gait ? count > h->cfg.N_gait * 4 : (off < 0 || off + count > qrw::planner_state_items(h->cfg.N_gait)))
    return fail(-1, "qrw_planner_get_host: bad item");
  double raw[4];  // (state items are [item][B]: one instance's items are B doubles apart)
  HIP_OK(hipMemcpy2DAsync(gait ? raw : h_out, sizeof(double), h->plan_st + (size_t)off * B + b, B * sizeof(double), sizeof(double),
                          gait ? 4 : count, hipMemcpyDeviceToHost, h->host_stream), "qrw_planner_get_host: D2H planner state");
  HIP_OK(host_done(h), "qrw_planner_get_host: D2H planner state");
  for (int e = 0; gait && e < count; e++) {
    unsigned long long mask;
    memcpy(&mask, &raw[e % 4], sizeof(mask));
    h_out[e] = ((mask >> (e / 4)) & 1ull) ? 1.0 : 0.0;
  }
  return 0;
}

// ------------------------------------------------------------------ controller glue
static qrw::ControllerArgs ctrl_common(qrw_handle h, int mode) {
  qrw::ControllerArgs a;
  memset(&a, 0, sizeof(a));
  a.B = h->cfg.batch; a.n_steps = h->cfg.n_steps; a.mode = mode; a.dt_wbc = h->cfg.dt_wbc; a.h_ref = h->pcfg.h_ref;
  a.n_gait = h->cfg.N_gait;
  a.cs = h->ctrl_st;
  return a;
}
static qrw::ControllerArgs update_state_args(qrw_handle h, const double* d_joy_vref, const double* d_q_filt, const double* d_v_filt,
                                             const double* d_rpy, double* d_q, double* d_v, double* d_hv, double* d_vref, double* d_oRh_oTh) {
  qrw::ControllerArgs a = ctrl_common(h, qrw::kCtrlUpdateState);
  a.in0 = d_joy_vref; a.in1 = d_q_filt; a.in2 = d_v_filt; a.in3 = d_rpy;
  a.out0 = d_q; a.out1 = d_v; a.out2 = d_hv; a.out3 = d_vref; a.out4 = d_oRh_oTh;
  return a;
}
static qrw::ControllerArgs wbc_inputs_args(qrw_handle h, const double* d_x_f_mpc, const double* d_xref, const double* d_feet_pva,
                                           const double* d_v, double* d_x_f_wbc, double* d_q_wbc, double* d_b_v, double* d_f_cmd,
                                           double* d_feet_cmd) {
  qrw::ControllerArgs a = ctrl_common(h, qrw::kCtrlWbcInputs);
  a.in0 = d_x_f_mpc; a.in1 = d_xref; a.in2 = d_feet_pva; a.in3 = d_v;
  a.out0 = d_x_f_wbc; a.out1 = d_q_wbc; a.out2 = d_b_v; a.out3 = d_f_cmd; a.out4 = d_feet_cmd;
  return a;
}
static int ctrl_launch(const qrw::ControllerArgs& a, void* stream, const char* launch_failed) {
  return qrw::controller_launch(a, (hipStream_t)stream) ? fail(-11, launch_failed, hipGetLastError()) : 0;
}

extern "C" int qrw_mpc_result_shift(qrw_handle h, const double* d_gait, double* d_x_f_mpc, void* stream) {
  QRW_ENTER(h, !d_gait || !d_x_f_mpc, "qrw_mpc_result_shift: null argument");
  qrw::ControllerArgs a = ctrl_common(h, qrw::kCtrlMpcShift);
  a.in0 = d_gait;
  a.out0 = d_x_f_mpc;
  return ctrl_launch(a, stream, "qrw_mpc_result_shift: launch failed");
}
extern "C" int qrw_controller_init(qrw_handle h, const double* d_q_init12, double h_ref, void* stream) {
  QRW_ENTER(h, false, "qrw_controller_init: null handle");
  h->pcfg.h_ref = h_ref;
  qrw::ControllerArgs a = ctrl_common(h, qrw::kCtrlInit);
  a.in0 = d_q_init12;
  return ctrl_launch(a, stream, "qrw_controller_init: launch failed");
}
extern "C" int qrw_controller_update_state(qrw_handle h, const double* d_joy_vref, const double* d_q_filt,
                                           const double* d_v_filt, const double* d_rpy, double* d_q, double* d_v,
                                           double* d_hv, double* d_vref, double* d_oRh_oTh, void* stream) {
  QRW_ENTER(h, !d_joy_vref || !d_q_filt || !d_v_filt || !d_rpy || !d_q || !d_v || !d_hv, "qrw_controller_update_state: null argument");
  return ctrl_launch(update_state_args(h, d_joy_vref, d_q_filt, d_v_filt, d_rpy, d_q, d_v, d_hv, d_vref, d_oRh_oTh), stream,
                     "qrw_controller_update_state: launch failed");
}
extern "C" int qrw_controller_wbc_inputs(qrw_handle h, const double* d_x_f_mpc, const double* d_xref,
                                         const double* d_feet_pva, const double* d_v, double* d_x_f_wbc, double* d_q_wbc,
                                         double* d_b_v, double* d_f_cmd, double* d_feet_cmd, void* stream) {
  QRW_ENTER(h, !d_x_f_mpc || !d_xref || !d_feet_pva || !d_v || !d_q_wbc || !d_b_v || !d_feet_cmd, "qrw_controller_wbc_inputs: null argument");
  return ctrl_launch(wbc_inputs_args(h, d_x_f_mpc, d_xref, d_feet_pva, d_v, d_x_f_wbc, d_q_wbc, d_b_v, d_f_cmd, d_feet_cmd), stream,
                     "qrw_controller_wbc_inputs: launch failed");
}
extern "C" int qrw_controller_result(qrw_handle h, const double* d_tau_ff, const double* d_qdes, const double* d_vdes,
                                     const double* d_q_filt, const double* d_v_secu, double* d_result,
                                     int32_t* d_error_flag, void* stream) {
  QRW_ENTER(h, !d_tau_ff || !d_qdes || !d_vdes || !d_q_filt || !d_v_secu || !d_result, "qrw_controller_result: null argument");
  qrw::ControllerArgs a = ctrl_common(h, qrw::kCtrlResult);
  a.in0 = d_tau_ff; a.in1 = d_qdes; a.in2 = d_vdes; a.in3 = d_q_filt; a.in4 = d_v_secu;
  a.out0 = d_result; a.iout = d_error_flag;
  return ctrl_launch(a, stream, "qrw_controller_result: launch failed");
}

// ------------------------------------------------------------------ state estimator (scripts/Estimator.py)
// cut-off frequency -> first-order filter coefficient (scripts/Estimator.py:254-262)
static double filter_alpha(double fc, double dt) {
  const double y = 1 - cos(2 * M_PI * fc * dt);
  return -y + sqrt(y * y + 2 * y);
}
static qrw::EstimatorArgs estimator_common(qrw_handle h) {
  qrw::EstimatorArgs a;
  memset(&a, 0, sizeof(a));
  a.B = h->cfg.batch; a.N_gait = h->cfg.N_gait; a.perfect = h->ecfg.perfect ? 1 : 0;
  a.dt = h->cfg.dt_wbc; a.h_init = h->ecfg.h_init; a.alpha_v = h->est_alpha_v; a.alpha_secu = h->est_alpha_secu;
  a.es = h->est_st;
  a.kalman = h->est_kalman ? 1 : 0;
  if (h->est_kalman) {
    a.ks = h->kal_st;
    a.kf_sigma_kin = h->kcfg.sigma_kin; a.kf_sigma_h = h->kcfg.sigma_h; a.kf_sigma_a = h->kcfg.sigma_a;
    a.kf_sigma_dp = h->kcfg.sigma_dp; a.kf_gamma = h->kcfg.gamma;
  }
  return a;
}
// Estimator.__init__ for the filter `kalman` chooses: the handle's mode, its filter coefficients, the init launch
static int estimator_reset(qrw_handle h, const qrw_estimator_config* cfg, bool kalman, void* stream, const char* failed) {
  h->ecfg = *cfg;
  h->est_kalman = kalman;
  h->est_alpha_v = filter_alpha(50.0, h->cfg.dt_wbc);
  h->est_alpha_secu = filter_alpha(6.0, h->cfg.dt_wbc);
  qrw::EstimatorArgs a = estimator_common(h);
  a.init = 1;
  if (qrw::estimator_launch(a, (hipStream_t)stream) != 0) return fail(-11, failed, hipGetLastError());
  note_launch(h, kFamEst, (hipStream_t)stream);
  h->est_ready = true;
  return 0;
}

extern "C" int qrw_estimator_init(qrw_handle h, const qrw_estimator_config* cfg, void* stream) {
  QRW_ENTER(h, !cfg, "qrw_estimator_init: null argument");
  return estimator_reset(h, cfg, false, stream, "qrw_estimator_init: launch failed");
}

extern "C" int qrw_estimator_init_kalman(qrw_handle h, const qrw_estimator_config* cfg, const qrw_kalman_config* kcfg, void* stream) {
  QRW_ENTER(h, !cfg, "qrw_estimator_init_kalman: null argument");
  const qrw_kalman_config k = kcfg ? *kcfg : qrw_kalman_config{0.1, 1.0, 0.1, 0.1, 30.0};  // (scripts/Estimator.py:133-137)
  for (const double sigma : {k.sigma_kin, k.sigma_h, k.sigma_a, k.sigma_dp})
    if (!(sigma > 0.0) || !std::isfinite(sigma)) return fail(-1, "qrw_estimator_init_kalman: the sigmas must be > 0 and finite");
  if (!std::isfinite(k.gamma)) return fail(-1, "qrw_estimator_init_kalman: gamma must be finite");
  if (!h->kal_st) {  // (the init kernel writes every item: no fill)
    const hipError_t e = h->kal_st.alloc((size_t)h->cfg.batch * qrw::kKalStItems);
    if (e != hipSuccess) return fail(-10, "qrw_estimator_init_kalman: hipMalloc kal_st", e);
  }
  h->kcfg = k;
  return estimator_reset(h, cfg, true, stream, "qrw_estimator_init_kalman: launch failed");
}

extern "C" int qrw_estimator_step(qrw_handle h, const double* d_lin_acc, const double* d_ang_vel, const double* d_quat,
                                  const double* d_q_mes, const double* d_v_mes, const double* d_gait, const double* d_goals,
                                  const double* d_true_pos, const double* d_true_b_vel, double* d_q_filt, double* d_v_filt,
                                  double* d_rpy, double* d_v_secu, void* stream) {
  QRW_ENTER(h, !h->est_ready, "qrw_estimator_step: estimator not initialised");
  if ((!d_gait || !d_goals) && !h->plan_ready)
    return fail(-1, "qrw_estimator_step: planner not initialised (d_gait / d_goals NULL take the planner's gait and foot positions)");
  if (!d_lin_acc || !d_ang_vel || !d_quat || !d_q_mes || !d_v_mes) return fail(-1, "qrw_estimator_step: null input");
  if (!d_q_filt || !d_v_filt || !d_rpy || !d_v_secu) return fail(-1, "qrw_estimator_step: null output");
  if (h->ecfg.perfect ? (!d_true_pos || !d_true_b_vel) : (d_true_pos || d_true_b_vel))
    return fail(-1, h->ecfg.perfect ? "qrw_estimator_step: a perfect estimator needs both d_true_pos and d_true_b_vel"
                                    : "qrw_estimator_step: d_true_pos / d_true_b_vel given to an estimator that is not perfect");
  qrw::EstimatorArgs a = estimator_common(h);
  a.lin_acc = d_lin_acc; a.ang_vel = d_ang_vel; a.quat = d_quat; a.q_mes = d_q_mes; a.v_mes = d_v_mes;
  a.gait = d_gait; a.goals = d_goals; a.true_pos = d_true_pos; a.true_b_vel = d_true_b_vel;
  a.ps = h->plan_st;
  a.ps_cur = qrw::planner_item_offset(h->cfg.N_gait, 1);
  a.ps_pos = qrw::planner_item_offset(h->cfg.N_gait, 9);
  a.q_filt = d_q_filt; a.v_filt = d_v_filt; a.rpy = d_rpy; a.v_secu = d_v_secu;
  if (qrw::estimator_launch(a, (hipStream_t)stream) != 0) return fail(-11, "qrw_estimator_step: launch failed", hipGetLastError());
  note_launch(h, kFamEst, (hipStream_t)stream);
  return 0;
}

extern "C" int qrw_estimator_step_host(qrw_handle h, const double* h_lin_acc, const double* h_ang_vel, const double* h_quat,
                                       const double* h_q_mes, const double* h_v_mes, const double* h_gait, const double* h_goals,
                                       const double* h_true_pos, const double* h_true_b_vel, double* h_q_filt, double* h_v_filt,
                                       double* h_rpy, double* h_v_secu) {
  QRW_ENTER_HOST(h, !h->est_ready, "qrw_estimator_step_host: estimator not initialised");
  if (!h_lin_acc || !h_ang_vel || !h_quat || !h_q_mes || !h_v_mes) return fail(-1, "qrw_estimator_step_host: null input");
  const size_t B = h->cfg.batch, Ng = h->cfg.N_gait;
  HIP_OK(wait_family(h, kFamEst), "qrw_estimator_step_host: earlier estimator step of this handle");
  if (!h_gait || !h_goals) HIP_OK(wait_family(h, kFamPlan), "qrw_estimator_step_host: earlier planner step of this handle");
  Stager s(h);
  const double *la = s.in(h_lin_acc, B * 3), *av = s.in(h_ang_vel, B * 3), *qt = s.in(h_quat, B * 4), *qm = s.in(h_q_mes, B * 12),
               *vm = s.in(h_v_mes, B * 12);
  const double* gt = h_gait ? s.in(h_gait, B * Ng * 4) : nullptr;
  const double* gl = h_goals ? s.in(h_goals, B * 12) : nullptr;
  const double* tp = h_true_pos ? s.in(h_true_pos, B * 3) : nullptr;
  const double* tv = h_true_b_vel ? s.in(h_true_b_vel, B * 3) : nullptr;
  double *qf = s.out(B * 19), *vf = s.out(B * 18), *rp = s.out(B * 3), *vs = s.out(B * 12);
  if (!s.ok) return fail(-12, "qrw_estimator_step_host: staging failed");
  if (const int rc = qrw_estimator_step(h, la, av, qt, qm, vm, gt, gl, tp, tv, qf, vf, rp, vs, (void*)h->host_stream)) return rc;
  if (!(s.back(h_q_filt, qf, B * 19) && s.back(h_v_filt, vf, B * 18) && s.back(h_rpy, rp, B * 3) && s.back(h_v_secu, vs, B * 12)))
    return fail(-12, "qrw_estimator_step_host: D2H failed");
  HIP_OK(host_done(h), "qrw_estimator_step_host sync");
  return 0;
}

extern "C" int qrw_estimator_get_host(qrw_handle h, int32_t which, int32_t b, int32_t count, double* h_out) {
  QRW_ENTER_HOST(h, !h_out || b < 0 || b >= h->cfg.batch || count < 1, "qrw_estimator_get_host: bad argument");
  static const int kOff[13] = {qrw::kEsKsc, qrw::kEsFkVel, qrw::kEsFkXyz, qrw::kEsMeanFeet, qrw::kEsHPv, qrw::kEsLPv, qrw::kEsHPp,
                               qrw::kEsLPp, qrw::kEsAlpha, qrw::kEsClose, qrw::kEsYawOff, qrw::kEsKlog, qrw::kEsFiltVel};
  static const int kLen[13] = {4, 3, 3, 3, 3, 3, 3, 3, 1, 1, 1, 1, 3};
  if (which < 0 || which >= 13 || count > kLen[which]) return fail(-1, "qrw_estimator_get_host: bad item");
  const size_t B = h->cfg.batch;
  HIP_OK(wait_family(h, kFamEst), "qrw_estimator_get_host: earlier estimator step of this handle");
  // (state items are [item][B]: one instance's items are B doubles apart)
  HIP_OK(hipMemcpy2DAsync(h_out, sizeof(double), h->est_st + (size_t)kOff[which] * B + b, B * sizeof(double), sizeof(double), count,
                          hipMemcpyDeviceToHost, h->host_stream), "qrw_estimator_get_host: D2H estimator state");
  HIP_OK(host_done(h), "qrw_estimator_get_host: D2H estimator state");
  return 0;
}

extern "C" int qrw_estimator_kalman_get_host(qrw_handle h, int32_t which, int32_t b, int32_t count, double* h_out) {
  QRW_ENTER_HOST(h, !h_out || b < 0 || b >= h->cfg.batch || count < 1, "qrw_estimator_kalman_get_host: bad argument");
  if (!h->est_ready || !h->est_kalman) return fail(-1, "qrw_estimator_kalman_get_host: not in Kalman mode");
  static const int kLen[3] = {qrw::kf::kStates, qrw::kf::kStates * qrw::kf::kStates, qrw::kf::kMeas};
  if (which < 0 || which >= 3 || count > kLen[which]) return fail(-1, "qrw_estimator_kalman_get_host: bad item");
  const size_t B = h->cfg.batch;
  HIP_OK(wait_family(h, kFamEst), "qrw_estimator_kalman_get_host: earlier estimator step of this handle");
  double blocks[3 * 36];
  const int off = which == 0 ? qrw::kKsX : which == 1 ? qrw::kKsP : qrw::kKsZ;
  const int items = which == 1 ? 3 * 36 : count;
  HIP_OK(hipMemcpy2DAsync(which == 1 ? blocks : h_out, sizeof(double), h->kal_st + (size_t)off * B + b, B * sizeof(double),
                          sizeof(double), items, hipMemcpyDeviceToHost, h->host_stream), "qrw_estimator_kalman_get_host: D2H filter state");
  HIP_OK(host_done(h), "qrw_estimator_kalman_get_host: D2H filter state");
  if (which == 1) {  // the dense P from the per-axis blocks: exact zeros between the axes
    double P[qrw::kf::kStates * qrw::kf::kStates];
    qrw::kf::Filter f;
    for (int j = 0; j < 3; j++) memcpy(f.axis[j].p, blocks + 36 * j, sizeof(f.axis[j].p));
    qrw::kf::filter_covariance(f, P);
    memcpy(h_out, P, (size_t)count * sizeof(double));
  }
  return 0;
}

// ------------------------------------------------------------------ rigid-body simulator (sim_kernel.hip)
static const char* sim_bad_params(const qrw_sim_params* p) {
  if (!(p->dt > 0.0) || p->substeps < 1 || p->substeps > 1024) return "dt must be > 0 and substeps in 1..1024";
  if (!(p->kn >= 0.0) || !(p->dn >= 0.0) || !(p->mu >= 0.0) || !(p->vs > 0.0)) return "kn, dn, mu must be >= 0 and vs > 0";
  return nullptr;
}
static bool sim_buffers_complete(const qrw_sim_buffers* o) {
  return o && o->d_q_mes && o->d_v_mes && o->d_quat && o->d_ang_vel && o->d_lin_acc && o->d_o_imu_vel && o->d_true_pos && o->d_true_b_vel &&
         o->d_contact_forces && o->d_joint_torques;
}
static qrw::SimArgs sim_common(qrw_handle h, int mode, const qrw_sim_buffers* o) {
  qrw::SimArgs a;
  memset(&a, 0, sizeof(a));
  const qrw_sim_params& p = h->sim_prm;
  a.B = h->cfg.batch; a.mode = mode; a.substeps = p.substeps; a.cmd_ld = 12; a.q_ld = 19;
  a.dt = p.dt; a.kn = p.kn; a.dn = p.dn; a.mu = p.mu; a.vs = p.vs; a.foot_radius = p.foot_radius; a.base_height = p.base_height;
  a.ss = h->sim_st;
  a.q_mes = o->d_q_mes; a.v_mes = o->d_v_mes; a.quat = o->d_quat; a.ang_vel = o->d_ang_vel; a.lin_acc = o->d_lin_acc;
  a.o_imu_vel = o->d_o_imu_vel; a.true_pos = o->d_true_pos; a.true_b_vel = o->d_true_b_vel;
  a.contact_forces = o->d_contact_forces; a.joint_torques = o->d_joint_torques;
  sim_terrain_args(h, a);
  return a;
}
// the handle's own measurement buffers (host-buffer entry points), carved out of sim_out
static qrw_sim_buffers sim_own_buffers(qrw_handle h) {
  const size_t B = h->cfg.batch;
  double* p = h->sim_out;
  qrw_sim_buffers o;
  o.d_q_mes = p; p += B * 12;
  o.d_v_mes = p; p += B * 12;
  o.d_quat = p; p += B * 4;
  o.d_ang_vel = p; p += B * 3;
  o.d_lin_acc = p; p += B * 3;
  o.d_o_imu_vel = p; p += B * 3;
  o.d_true_pos = p; p += B * 3;
  o.d_true_b_vel = p; p += B * 3;
  o.d_contact_forces = p; p += B * 12;
  o.d_joint_torques = p;
  return o;
}
constexpr size_t kSimOutPerInstance = 12 + 12 + 4 + 3 * 5 + 12 + 12;
static int sim_read_own(qrw_handle h, const qrw_sim_buffers* ho, const char* who) {
  const size_t B = h->cfg.batch;
  const qrw_sim_buffers d = sim_own_buffers(h);
  return read_back(h, kFamNone, who,
                   {{ho->d_q_mes, d.d_q_mes, B * 12 * sizeof(double)}, {ho->d_v_mes, d.d_v_mes, B * 12 * sizeof(double)},
                    {ho->d_quat, d.d_quat, B * 4 * sizeof(double)}, {ho->d_ang_vel, d.d_ang_vel, B * 3 * sizeof(double)},
                    {ho->d_lin_acc, d.d_lin_acc, B * 3 * sizeof(double)}, {ho->d_o_imu_vel, d.d_o_imu_vel, B * 3 * sizeof(double)},
                    {ho->d_true_pos, d.d_true_pos, B * 3 * sizeof(double)}, {ho->d_true_b_vel, d.d_true_b_vel, B * 3 * sizeof(double)},
                    {ho->d_contact_forces, d.d_contact_forces, B * 12 * sizeof(double)},
                    {ho->d_joint_torques, d.d_joint_torques, B * 12 * sizeof(double)}});
}

extern "C" int qrw_sim_init(qrw_handle h, const double* d_q_init, int32_t q_ld, const qrw_sim_params* params, const qrw_sim_buffers* out,
                            void* stream) {
  QRW_ENTER(h, !d_q_init || !params || !out, "qrw_sim_init: null argument");
  if (q_ld != 19 && q_ld != 12) return fail(-1, "qrw_sim_init: q_ld must be 19 (q19) or 12 (joints)");
  if (const char* bad = sim_bad_params(params)) return fail(-1, (std::string("qrw_sim_init: ") + bad).c_str());
  if (!sim_buffers_complete(out)) return fail(-1, "qrw_sim_init: null output buffer");
  if (!h->sim_st) {
    HIP_OK(h->sim_st.alloc((size_t)h->cfg.batch * qrw::kSimStItems), "qrw_sim_init: hipMalloc sim_st");
    HIP_OK(h->sim_st.fill(0, (hipStream_t)stream), "qrw_sim_init: zero fill of sim_st");
  }
  h->sim_prm = *params;
  qrw::SimArgs a = sim_common(h, 1, out);
  a.q_init = d_q_init; a.q_ld = q_ld;
  if (qrw::sim_launch(a, (hipStream_t)stream) != 0) return fail(-11, "qrw_sim_init: launch failed", hipGetLastError());
  note_launch(h, kFamSim, (hipStream_t)stream);
  h->sim_ready = true;
  return 0;
}

extern "C" int qrw_sim_step(qrw_handle h, const double* d_P, const double* d_D, const double* d_q_des, const double* d_v_des,
                            const double* d_tau_ff, int32_t cmd_ld, const double* d_f_ext, const qrw_sim_buffers* out, void* stream) {
  QRW_ENTER(h, !h->sim_ready, "qrw_sim_step: simulator not initialised");
  if (!d_P || !d_D || !d_q_des || !d_v_des || !d_tau_ff) return fail(-1, "qrw_sim_step: null input");
  if (cmd_ld < 12) return fail(-1, "qrw_sim_step: cmd_ld must be >= 12");
  if (!sim_buffers_complete(out)) return fail(-1, "qrw_sim_step: null output buffer");
  qrw::SimArgs a = sim_common(h, 0, out);
  a.P = d_P; a.D = d_D; a.q_des = d_q_des; a.v_des = d_v_des; a.tau_ff = d_tau_ff; a.cmd_ld = cmd_ld; a.f_ext = d_f_ext;
  if (qrw::sim_launch(a, (hipStream_t)stream) != 0) return fail(-11, "qrw_sim_step: launch failed", hipGetLastError());
  note_launch(h, kFamSim, (hipStream_t)stream);
  return 0;
}

extern "C" int qrw_sim_init_host(qrw_handle h, const double* h_q_init, int32_t q_ld, const qrw_sim_params* params,
                                 const qrw_sim_buffers* h_out) {
  QRW_ENTER_HOST(h, !h_q_init || !params || !h_out, "qrw_sim_init_host: null argument");
  if (q_ld != 19 && q_ld != 12) return fail(-1, "qrw_sim_init_host: q_ld must be 19 (q19) or 12 (joints)");
  const size_t B = h->cfg.batch;
  HIP_OK(wait_family(h, kFamSim), "qrw_sim_init_host: earlier simulator step of this handle");
  if (!h->sim_out) {
    HIP_OK(h->sim_out.alloc(B * kSimOutPerInstance), "qrw_sim_init_host: hipMalloc sim_out");
    HIP_OK(h->sim_out.fill(0, h->host_stream), "qrw_sim_init_host: zero fill of sim_out");
  }
  Stager s(h);
  const double* q = s.in(h_q_init, B * (size_t)q_ld);
  if (!s.ok) return fail(-12, "qrw_sim_init_host: staging failed");
  const qrw_sim_buffers own = sim_own_buffers(h);
  if (const int rc = qrw_sim_init(h, q, q_ld, params, &own, (void*)h->host_stream)) return rc;
  return sim_read_own(h, h_out, "qrw_sim_init_host");
}

extern "C" int qrw_sim_step_host(qrw_handle h, const double* h_P, const double* h_D, const double* h_q_des, const double* h_v_des,
                                 const double* h_tau_ff, const double* h_f_ext, const qrw_sim_buffers* h_out) {
  QRW_ENTER_HOST(h, !h->sim_ready || !h->sim_out, "qrw_sim_step_host: simulator not initialised with qrw_sim_init_host");
  if (!h_P || !h_D || !h_q_des || !h_v_des || !h_tau_ff || !h_out) return fail(-1, "qrw_sim_step_host: null argument");
  const size_t B = h->cfg.batch;
  HIP_OK(wait_family(h, kFamSim), "qrw_sim_step_host: earlier simulator step of this handle");
  Stager s(h);
  const double *P = s.in(h_P, B * 12), *D = s.in(h_D, B * 12), *qd = s.in(h_q_des, B * 12), *vd = s.in(h_v_des, B * 12),
               *tf = s.in(h_tau_ff, B * 12);
  const double* fe = h_f_ext ? s.in(h_f_ext, B * 6) : nullptr;
  if (!s.ok) return fail(-12, "qrw_sim_step_host: staging failed");
  const qrw_sim_buffers own = sim_own_buffers(h);
  if (const int rc = qrw_sim_step(h, P, D, qd, vd, tf, 12, fe, &own, (void*)h->host_stream)) return rc;
  return sim_read_own(h, h_out, "qrw_sim_step_host");
}

extern "C" int qrw_sim_get_host(qrw_handle h, double* h_state) {
  QRW_ENTER_HOST(h, !h_state, "qrw_sim_get_host: null argument");
  if (!h->sim_ready) return fail(-1, "qrw_sim_get_host: simulator not initialised");
  return read_back(h, kFamSim, "qrw_sim_get_host", {{h_state, h->sim_st.p, h->sim_st.bytes}});
}

extern "C" int qrw_sim_set_host(qrw_handle h, const double* h_state) {
  QRW_ENTER_HOST(h, !h_state, "qrw_sim_set_host: null argument");
  if (!h->sim_ready) return fail(-1, "qrw_sim_set_host: simulator not initialised");
  HIP_OK(wait_family(h, kFamSim), "qrw_sim_set_host: earlier simulator step of this handle");
  HIP_OK(h2d(h, h->sim_st.p, h_state, h->sim_st.bytes), "qrw_sim_set_host: H2D simulator state");
  HIP_OK(host_done(h), "qrw_sim_set_host: H2D simulator state");
  note_launch(h, kFamSim, h->host_stream);
  return 0;
}

// ---- heightfield terrain of the simulator
static const char* sim_bad_terrain(const double* heights, int32_t rows, int32_t cols, double x0, double y0, double dx, double dy) {
  if (!heights) return "null heights";
  if (rows < 2 || cols < 2) return "rows and cols must be >= 2";
  if (!(dx > 0.0) || !(dy > 0.0) || !std::isfinite(dx) || !std::isfinite(dy)) return "dx and dy must be positive and finite";
  if (!std::isfinite(x0) || !std::isfinite(y0)) return "x0 and y0 must be finite";
  return nullptr;
}
// The handle's own copy of the field (and of the origins), `kind` the direction of the copies on `stream`.  The buffers are
// reallocated only when the size changes (hipFree waits for the device, so no launch still reads what goes); the setting takes
// effect only once both copies are queued.
static int sim_store_terrain(qrw_handle h, const char* who, const double* heights, int32_t rows, int32_t cols, double x0, double y0,
                             double dx, double dy, const double* origin_xy, hipMemcpyKind kind, hipStream_t stream) {
  const size_t count = (size_t)rows * (size_t)cols, B = (size_t)h->cfg.batch;
  if (h->sim_terrain.count() != count) {
    h->sim_terrain_on = false;
    HIP_OK(h->sim_terrain.alloc(count), who);
  }
  if (origin_xy && h->sim_origin.count() != 2 * B) {
    h->sim_origin_on = false;
    HIP_OK(h->sim_origin.alloc(2 * B), who);
  }
  HIP_OK(hipMemcpyAsync(h->sim_terrain.p, heights, h->sim_terrain.bytes, kind, stream), who);
  if (origin_xy) HIP_OK(hipMemcpyAsync(h->sim_origin.p, origin_xy, h->sim_origin.bytes, kind, stream), who);
  h->sim_t_rows = rows; h->sim_t_cols = cols;
  h->sim_t_x0 = x0; h->sim_t_y0 = y0; h->sim_t_dx = dx; h->sim_t_dy = dy;
  h->sim_terrain_on = true;
  h->sim_origin_on = origin_xy != nullptr;
  note_launch(h, kFamSim, stream);
  return 0;
}

extern "C" int qrw_sim_set_terrain(qrw_handle h, const double* d_heights, int32_t rows, int32_t cols, double x0, double y0, double dx,
                                   double dy, const double* d_origin_xy, void* stream) {
  QRW_ENTER(h, false, "qrw_sim_set_terrain: null handle");
  if (const char* bad = sim_bad_terrain(d_heights, rows, cols, x0, y0, dx, dy))
    return fail(-1, (std::string("qrw_sim_set_terrain: ") + bad).c_str());
  return sim_store_terrain(h, "qrw_sim_set_terrain", d_heights, rows, cols, x0, y0, dx, dy, d_origin_xy, hipMemcpyDeviceToDevice,
                           (hipStream_t)stream);
}

extern "C" int qrw_sim_set_terrain_host(qrw_handle h, const double* h_heights, int32_t rows, int32_t cols, double x0, double y0,
                                        double dx, double dy, const double* h_origin_xy) {
  QRW_ENTER_HOST(h, false, "qrw_sim_set_terrain_host: null handle");
  if (const char* bad = sim_bad_terrain(h_heights, rows, cols, x0, y0, dx, dy))
    return fail(-1, (std::string("qrw_sim_set_terrain_host: ") + bad).c_str());
  HIP_OK(wait_family(h, kFamSim), "qrw_sim_set_terrain_host: earlier simulator step of this handle");
  if (const int rc = sim_store_terrain(h, "qrw_sim_set_terrain_host", h_heights, rows, cols, x0, y0, dx, dy, h_origin_xy,
                                       hipMemcpyHostToDevice, h->host_stream))
    return rc;
  HIP_OK(host_done(h), "qrw_sim_set_terrain_host: H2D terrain");
  return 0;
}

extern "C" int qrw_sim_clear_terrain(qrw_handle h) {
  if (!h) return fail(-1, "qrw_sim_clear_terrain: null handle");
  h->sim_terrain_on = h->sim_origin_on = false;  // (the buffers stay for the next qrw_sim_set_terrain of the same size)
  return 0;
}

// ------------------------------------------------------------------ joystick stage (joystick_kernel.hip)
// what every joystick launch of a handle is told: the configuration and the item-major tables carved out of joy_ti / joy_td
static qrw::JoystickArgs joystick_common(qrw_handle h) {
  qrw::JoystickArgs a;
  memset(&a, 0, sizeof(a));
  const qrw_joystick_config& c = h->jcfg;
  const size_t B = h->cfg.batch;
  const size_t ns = c.mode == QRW_JOY_PROFILE ? c.n_switch : 0, nc = c.n_codes, np = c.n_pushes;
  a.t.B = h->cfg.batch; a.t.n_switch = (int)ns; a.t.n_codes = c.n_codes; a.t.n_pushes = c.n_pushes;
  a.t.k_start = c.k_start; a.t.gp_alpha = c.gp_alpha; a.t.gp_deadband = c.gp_deadband;
  int32_t* ti = h->joy_ti;
  a.t.k_switch = ti; ti += ns * B;
  a.t.code_k = ti; ti += nc * B;
  a.t.code_v = ti; ti += nc * B;
  a.t.push_start = ti; ti += np * B;
  a.t.push_dur = ti;
  double* td = h->joy_td;
  a.t.v_switch = td; td += ns * 6 * B;
  a.t.ramp_v = td; td += 3 * B;
  a.t.push_w = td;
  a.st = h->joy_st;
  return a;
}

// Joystick.__init__ (scripts/Joystick.py:14-58) + update_for_analysis (:317-326) / the tables of update_v_ref_predefined (:201-284)
extern "C" int qrw_joystick_init(qrw_handle h, const qrw_joystick_config* cfg, const qrw_joystick_tables* tab, void* stream) {
  QRW_ENTER_HOST(h, !cfg || !tab, "qrw_joystick_init: null argument");
  namespace joy = qrw::joy;
  char text[256];
  auto refuse = [&](const char* what) { return fail(-1, (std::string("qrw_joystick_init: ") + what).c_str()); };
  const int B = h->cfg.batch;
  // ---- validation, on the host, before anything is allocated, copied or launched
  if (cfg->mode != QRW_JOY_PROFILE && cfg->mode != QRW_JOY_RAMP && cfg->mode != QRW_JOY_GAMEPAD)
    return refuse("mode must be QRW_JOY_PROFILE, QRW_JOY_RAMP or QRW_JOY_GAMEPAD");
  if (cfg->n_codes < 0 || cfg->n_codes > joy::kMaxCodes) return refuse("n_codes must be in 0..16");
  if (cfg->n_pushes < 0 || cfg->n_pushes > joy::kMaxPushes) return refuse("n_pushes must be in 0..8");
  if (cfg->n_codes && (!tab->code_k || !tab->code_v)) return refuse("n_codes > 0 needs code_k and code_v");
  if (cfg->n_pushes && (!tab->push_k || !tab->push_w)) return refuse("n_pushes > 0 needs push_k and push_w");
  const int ns = cfg->mode == QRW_JOY_PROFILE ? cfg->n_switch : 0, nc = cfg->n_codes, np = cfg->n_pushes;
  if (cfg->mode == QRW_JOY_PROFILE) {
    if (ns < 1 || ns > joy::kMaxSwitch) return refuse("n_switch must be in 1..32");
    if (!tab->k_switch || !tab->v_switch) return refuse("profile mode needs k_switch and v_switch");
    for (int b = 0; b < B; b++) {
      int entry = 0;
      const int bad = joy::check_profile(tab->k_switch + (size_t)b * ns, ns, &entry);
      if (!bad) continue;
      snprintf(text, sizeof(text), "robot %d, k_switch entry %d: %s", b, entry,
               bad == joy::kBadFirst ? "the table must start at or before tick 0"
               : bad == joy::kBadDecreasing ? "decreasing (k_switch must be non-decreasing)"
                                            : "more than 2^17 ticks after the entry before it (t1^3 must be exact in a double)");
      return refuse(text);
    }
  } else if (cfg->mode == QRW_JOY_RAMP) {
    if (!tab->ramp_v) return refuse("ramp mode needs ramp_v");
    for (int b = 0; b < B; b++) {
      int entry = 0;
      if (joy::check_ramp(tab->ramp_v + (size_t)b * 3, &entry)) {
        snprintf(text, sizeof(text), "robot %d, ramp_v entry %d: not finite, or |V| x scale does not fit an int32", b, entry);
        return refuse(text);
      }
    }
  } else {
    if (!(cfg->gp_alpha > 0.0 && cfg->gp_alpha <= 1.0)) return refuse("gp_alpha must be in (0, 1]");
    if (!(cfg->gp_deadband >= 0.0) || !std::isfinite(cfg->gp_deadband)) return refuse("gp_deadband must be >= 0 and finite");
  }
  std::vector<int32_t> dur((size_t)np);
  for (int b = 0; b < B && np; b++) {
    for (int e = 0; e < np; e++) dur[e] = tab->push_k[((size_t)b * np + e) * 2 + 1];
    int entry = 0;
    if (joy::check_push(dur.data(), np, &entry)) {
      snprintf(text, sizeof(text), "robot %d, push entry %d: duration %d is not in 1..2^13 (t1^4 must be exact in a double)", b, entry,
               dur[entry]);
      return refuse(text);
    }
  }
  // ---- the item-major copies ([entry][B], [entry][6][B]), in the order joystick_common carves them
  const size_t Bz = (size_t)B;
  std::vector<int32_t> ti(((size_t)ns + 2 * (size_t)nc + 2 * (size_t)np) * Bz + 1);
  std::vector<double> td(((size_t)ns * 6 + 3 + (size_t)np * 6) * Bz);
  int32_t *ksw = ti.data(), *ck = ksw + ns * Bz, *cv = ck + nc * Bz, *ps = cv + nc * Bz, *pd = ps + np * Bz;
  double *vsw = td.data(), *rv = vsw + (size_t)ns * 6 * Bz, *pw = rv + 3 * Bz;
  for (size_t b = 0; b < Bz; b++) {
    for (int i = 0; i < ns; i++) {
      ksw[i * Bz + b] = tab->k_switch[b * ns + i];
      for (int c = 0; c < 6; c++) vsw[((size_t)i * 6 + c) * Bz + b] = tab->v_switch[(b * 6 + c) * ns + i];
    }
    for (int c = 0; c < 3; c++) rv[c * Bz + b] = cfg->mode == QRW_JOY_RAMP ? tab->ramp_v[b * 3 + c] : 0.0;
    for (int e = 0; e < nc; e++) {
      ck[e * Bz + b] = tab->code_k[b * nc + e];
      cv[e * Bz + b] = tab->code_v[b * nc + e];
    }
    for (int e = 0; e < np; e++) {
      ps[e * Bz + b] = tab->push_k[(b * np + e) * 2];
      pd[e * Bz + b] = tab->push_k[(b * np + e) * 2 + 1];
      for (int c = 0; c < 6; c++) pw[((size_t)e * 6 + c) * Bz + b] = tab->push_w[(b * np + e) * 6 + c];
    }
  }
  // no step in flight reads the tables while they are replaced (hipFree waits for the device besides)
  HIP_OK(wait_family(h, kFamJoy), "qrw_joystick_init: earlier joystick step of this handle");
  h->joy_ready = false;
  if (!h->joy_st) HIP_OK(h->joy_st.alloc(Bz * qrw::kJoyStItems), "qrw_joystick_init: hipMalloc joy_st");  // (the init launch writes every item)
  if (h->joy_ti.count() != ti.size()) HIP_OK(h->joy_ti.alloc(ti.size()), "qrw_joystick_init: hipMalloc joy_ti");
  if (h->joy_td.count() != td.size()) HIP_OK(h->joy_td.alloc(td.size()), "qrw_joystick_init: hipMalloc joy_td");
  HIP_OK(h2d(h, h->joy_ti.p, ti.data(), ti.size() * sizeof(int32_t)), "qrw_joystick_init: H2D tables");
  HIP_OK(h2d(h, h->joy_td.p, td.data(), td.size() * sizeof(double)), "qrw_joystick_init: H2D tables");
  HIP_OK(host_done(h), "qrw_joystick_init: H2D tables");
  h->jcfg = *cfg;
  qrw::JoystickArgs a = joystick_common(h);
  a.init = 1;
  if (qrw::joystick_launch(a, cfg->mode, (hipStream_t)stream) != 0) return fail(-11, "qrw_joystick_init: launch failed", hipGetLastError());
  note_launch(h, kFamJoy, (hipStream_t)stream);
  h->joy_ready = true;
  return 0;
}

// Joystick.update_v_ref(k_loop, velID) (scripts/Joystick.py:60-79) + apply_external_force (scripts/PyBulletSimulator.py:402-431)
extern "C" int qrw_joystick_step(qrw_handle h, int32_t k, const double* d_v_gp, const int32_t* d_stop, double* d_joy_vref,
                                 int32_t* d_code, double* d_f_ext, void* stream) {
  QRW_ENTER(h, !h->joy_ready, "qrw_joystick_step: joystick not initialised");
  if (k < 0) return fail(-1, "qrw_joystick_step: k must be >= 0");
  if (!d_joy_vref) return fail(-1, "qrw_joystick_step: null output d_joy_vref");
  if (h->jcfg.mode == QRW_JOY_GAMEPAD ? !d_v_gp : d_v_gp != nullptr)
    return fail(-1, h->jcfg.mode == QRW_JOY_GAMEPAD ? "qrw_joystick_step: gamepad mode needs d_v_gp"
                                                     : "qrw_joystick_step: d_v_gp given to a joystick that is not in gamepad mode");
  if (h->jcfg.n_pushes && !d_f_ext) return fail(-1, "qrw_joystick_step: the handle has pushes: d_f_ext must not be NULL");
  qrw::JoystickArgs a = joystick_common(h);
  a.k = k; a.v_gp = d_v_gp; a.stop = d_stop; a.joy_vref = d_joy_vref; a.code = d_code; a.f_ext = d_f_ext;
  if (qrw::joystick_launch(a, h->jcfg.mode, (hipStream_t)stream) != 0) return fail(-11, "qrw_joystick_step: launch failed", hipGetLastError());
  note_launch(h, kFamJoy, (hipStream_t)stream);
  return 0;
}

extern "C" int qrw_joystick_step_host(qrw_handle h, int32_t k, const double* h_v_gp, const int32_t* h_stop, double* h_joy_vref,
                                      int32_t* h_code, double* h_f_ext) {
  QRW_ENTER_HOST(h, !h->joy_ready, "qrw_joystick_step_host: joystick not initialised");
  if (!h_joy_vref) return fail(-1, "qrw_joystick_step_host: null output h_joy_vref");
  const size_t B = h->cfg.batch;
  HIP_OK(wait_family(h, kFamJoy), "qrw_joystick_step_host: earlier joystick step of this handle");
  Stager s(h);
  const double* gp = h_v_gp ? s.in(h_v_gp, B * 6) : nullptr;
  double* vr = s.out(B * 6);
  double* fe = (h_f_ext || h->jcfg.n_pushes) ? s.out(B * 6) : nullptr;
  // (the two int32 rows ride in the doubles' staging area)
  int32_t* st = h_stop ? (int32_t*)s.out((B + 1) / 2) : nullptr;
  int32_t* cd = h_code ? (int32_t*)s.out((B + 1) / 2) : nullptr;
  if (!s.ok) return fail(-12, "qrw_joystick_step_host: staging failed");
  if (st) HIP_OK(h2d(h, st, h_stop, B * sizeof(int32_t)), "qrw_joystick_step_host: H2D stop flags");
  if (const int rc = qrw_joystick_step(h, k, gp, st, vr, cd, fe, (void*)h->host_stream)) return rc;
  if (!(s.back(h_joy_vref, vr, B * 6) && s.back(h_f_ext, fe, B * 6))) return fail(-12, "qrw_joystick_step_host: D2H failed");
  if (cd) HIP_OK(d2h(h, h_code, cd, B * sizeof(int32_t)), "qrw_joystick_step_host: D2H codes");
  HIP_OK(host_done(h), "qrw_joystick_step_host sync");
  return 0;
}

// Joystick.v_ref of the gamepad filter; the outcome of control_loop (scripts/main_solo12_control.py:180,239) per robot
extern "C" int qrw_joystick_get_host(qrw_handle h, int32_t which, int32_t b, int32_t count, double* h_out) {
  QRW_ENTER_HOST(h, !h_out || b < 0 || b >= h->cfg.batch || count < 1, "qrw_joystick_get_host: bad argument");
  if (!h->joy_ready) return fail(-1, "qrw_joystick_get_host: joystick not initialised");
  const size_t B = h->cfg.batch;
  if (which == 1) {  // (state items are [item][B]: the k_stop of consecutive robots are consecutive doubles)
    if (count > h->cfg.batch - b) return fail(-1, "qrw_joystick_get_host: bad item");
    return read_back(h, kFamJoy, "qrw_joystick_get_host", {{h_out, h->joy_st + (size_t)qrw::kJsKstop * B + b, (size_t)count * sizeof(double)}});
  }
  if (which != 0 || count > 6) return fail(-1, "qrw_joystick_get_host: bad item");
  HIP_OK(wait_family(h, kFamJoy), "qrw_joystick_get_host: earlier joystick step of this handle");
  HIP_OK(hipMemcpy2DAsync(h_out, sizeof(double), h->joy_st + (size_t)qrw::kJsVref * B + b, B * sizeof(double), sizeof(double), count,
                          hipMemcpyDeviceToHost, h->host_stream), "qrw_joystick_get_host: D2H joystick state");
  HIP_OK(host_done(h), "qrw_joystick_get_host: D2H joystick state");
  return 0;
}

// ------------------------------------------------------------------ streams on a subset of the compute units
extern "C" int qrw_device_cu_count(int32_t device, int32_t* n_cus) {
  if (!n_cus) return fail(-1, "qrw_device_cu_count: null argument");
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return fail(-10, "qrw_device_cu_count: hipGetDeviceProperties failed", e);
  *n_cus = prop.multiProcessorCount;
  return 0;
}
extern "C" int qrw_stream_create(int32_t device, int32_t first_cu, int32_t n_cus, void** stream) {
  if (!stream) return fail(-1, "qrw_stream_create: null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return fail(-2, "qrw_stream_create: bad device ordinal");
  DeviceScope dev_scope__(device);
  hipError_t e = hipSuccess;
  hipStream_t s = nullptr;
  if (n_cus <= 0) {
    e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  } else {
    int32_t total = 0;
    if (qrw_device_cu_count(device, &total)) return -10;
    if (first_cu < 0 || first_cu + n_cus > total) return fail(-1, "qrw_stream_create: compute-unit range outside the device");
    const int words = (total + 31) / 32;
    uint32_t mask[64] = {0};
    if (words > 64) return fail(-1, "qrw_stream_create: device has more than 2048 compute units");
    for (int c = first_cu; c < first_cu + n_cus; c++) mask[c >> 5] |= 1u << (c & 31);
    e = hipExtStreamCreateWithCUMask(&s, (uint32_t)words, mask);
  }
  if (e != hipSuccess) return fail(-10, "qrw_stream_create: stream creation failed", e);
  *stream = (void*)s;
  return 0;
}
extern "C" int qrw_stream_destroy(void* stream) {
  if (!stream) return 0;
  // whatever the handles launched on it is complete before the stream goes: their getters then have nothing to wait for
  (void)hipStreamSynchronize((hipStream_t)stream);
  {
    std::lock_guard<std::mutex> lock(g_handles_mutex);
    for (qrw_handle_s* h : g_handles)
      for (int f = 0; f < kFamCount; f++)
        if (h->launched[f].load(std::memory_order_acquire) && h->last_stream[f].load(std::memory_order_relaxed) == (hipStream_t)stream)
          h->launched[f].store(false, std::memory_order_release);
  }
  hipError_t e = hipStreamDestroy((hipStream_t)stream);
  return e == hipSuccess ? 0 : fail(-10, "qrw_stream_destroy: hipStreamDestroy failed", e);
}

extern "C" int qrw_stream_wait_stream(qrw_handle h, void* waiter, void* signaller) {
  if (!h) return fail(-1, "qrw_stream_wait_stream: null handle");
  if (waiter == signaller) return 0;
  DeviceScope dev_scope__(h->cfg.device);
  if (!h->order_ev) HIP_OK(hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming), "qrw_stream_wait_stream: hipEventCreate");
  // one event serves every hand-over: hipStreamWaitEvent captures the record that is current when it is called
  HIP_OK(hipEventRecord(h->order_ev, (hipStream_t)signaller), "qrw_stream_wait_stream: hipEventRecord");
  HIP_OK(hipStreamWaitEvent((hipStream_t)waiter, h->order_ev, 0), "qrw_stream_wait_stream: hipStreamWaitEvent");
  return 0;
}

// ------------------------------------------------------------------ fused head of a control iteration
extern "C" int qrw_control_pre(qrw_handle h, int32_t k, const double* d_joy_vref, const double* d_q_filt,
                               const double* d_v_filt, const double* d_rpy, const int32_t* d_code, int32_t code_scalar,
                               const double* d_x_f_mpc, double* d_q, double* d_v, double* d_hv, double* d_vref,
                               double* d_oRh_oTh, double* d_xref, double* d_fsteps, double* d_gait, double* d_target,
                               double* d_feet_pva, double* d_contacts, double* d_x_f_wbc, double* d_q_wbc, double* d_b_v,
                               double* d_f_cmd, double* d_feet_cmd, void* stream) {
  QRW_ENTER(h, !h->plan_ready, "qrw_control_pre: planner not initialised");
  if (!d_joy_vref || !d_q_filt || !d_v_filt || !d_rpy || !d_q || !d_v || !d_hv || !d_vref || !d_xref || !d_feet_pva)
    return fail(-1, "qrw_control_pre: null argument");
  if (d_x_f_mpc && (!d_q_wbc || !d_b_v || !d_feet_cmd)) return fail(-1, "qrw_control_pre: null WBC target output");
  const qrw::ControllerArgs cu = update_state_args(h, d_joy_vref, d_q_filt, d_v_filt, d_rpy, d_q, d_v, d_hv, d_vref, d_oRh_oTh);
  qrw::PlannerArgs p = planner_step_args(h, k, d_q, 19, d_hv, d_vref, d_code, code_scalar, d_xref, d_fsteps, d_gait, d_target, d_feet_pva,
                                         d_contacts);
  // no fsteps wanted = this iteration does not solve: of xref only column 0 and horizon step 1 are read (WBC target assembly)
  p.xref_steps = (!d_fsteps && d_x_f_mpc) ? 1 : 0;
  const qrw::ControllerArgs cw = wbc_inputs_args(h, d_x_f_mpc, d_xref, d_feet_pva, d_v, d_x_f_wbc, d_q_wbc, d_b_v, d_f_cmd, d_feet_cmd);
  debug_poison_lds((hipStream_t)stream);
  if (qrw::control_pre_launch(cu, p, cw, d_x_f_mpc ? 1 : 0, (hipStream_t)stream) != 0)
    return fail(-11, "qrw_control_pre: launch failed", hipGetLastError());
  note_launch(h, kFamPlan, (hipStream_t)stream);
  return 0;
}

// ------------------------------------------------------------------ a non-solving iteration on bound buffers
extern "C" int qrw_iteration_bind(qrw_handle h, const qrw_iteration_buffers* b) {
  if (!h || !b) return fail(-1, "qrw_iteration_bind: null argument");
  if (!h->plan_ready) return fail(-1, "qrw_iteration_bind: planner not initialised");
  if (!b->d_joy_vref || !b->d_q_filt || !b->d_v_filt || !b->d_rpy || !b->d_v_secu || !b->d_q || !b->d_v || !b->d_hv || !b->d_vref ||
      !b->d_xref || !b->d_feet_pva || !b->d_contacts || !b->d_q_wbc || !b->d_b_v || !b->d_f_cmd || !b->d_feet_cmd || !b->d_result)
    return fail(-1, "qrw_iteration_bind: null buffer (only d_code, d_oRh_oTh, d_target, d_x_f_wbc and the WBC outputs other than "
                    "d_result may be NULL)");
  h->iter_bufs = *b;
  h->iter_bound = true;
  return 0;
}

extern "C" int qrw_iteration_step(qrw_handle h, int32_t k, const double* d_x_f_mpc, void* stream) {
  if (!h || !d_x_f_mpc) return fail(-1, "qrw_iteration_step: null argument");
  if (!h->iter_bound) return fail(-1, "qrw_iteration_step: no buffers bound (qrw_iteration_bind)");
  const qrw_iteration_buffers& b = h->iter_bufs;
  const size_t plane = (size_t)h->cfg.batch * 12;  // d_feet_cmd [3][B][3][4]: the planes are the WBC's pgoals / vgoals / agoals
  int rc = qrw_control_pre(h, k, b.d_joy_vref, b.d_q_filt, b.d_v_filt, b.d_rpy, b.d_code, b.code_scalar, d_x_f_mpc, b.d_q, b.d_v, b.d_hv,
                           b.d_vref, b.d_oRh_oTh, b.d_xref, nullptr, nullptr, b.d_target, b.d_feet_pva, b.d_contacts, b.d_x_f_wbc,
                           b.d_q_wbc, b.d_b_v, b.d_f_cmd, b.d_feet_cmd, stream);
  if (rc) return rc;
  return qrw_wbc_compute_result(h, b.d_q_wbc, b.d_b_v, b.d_f_cmd, b.d_contacts, b.d_feet_cmd, b.d_feet_cmd + plane, b.d_feet_cmd + 2 * plane,
                                b.d_tau_ff, b.d_qdes, b.d_vdes, b.d_f_with_delta, b.d_ddq_res, b.d_feet, b.d_q_filt, b.d_v_secu, b.d_result,
                                b.d_error_flag, stream);
}
