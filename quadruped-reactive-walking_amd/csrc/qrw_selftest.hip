// What libqrw_hip.so carries for its own checking, apart from the product entry points (qrw_api.hip): the LDS / register poison
// kernels, the known-answer check of mpc_solve_kernel behind qrw_create, qrw_selftest_sweeps, and the qrw_test_* entry points of
// include/qrw_hip_test.h.
#include <mutex>

#include "kat_table.h"
#include "qrw_host.h"

using namespace qrw::host;

// Tests only: every compute unit's LDS filled with a bit pattern (one 160 000-byte workgroup at a time per compute unit, far more
// workgroups than compute units), then the known-answer solve of mpc_solve_kernel for horizon N in launch form `mode` WITHOUT the
// per-process cache of qrw_create.  A kernel that reads LDS it has not written (an operand "multiplied by zero", a lane whose
// result is dropped later) passes on the zeros or small numbers other kernels usually leave behind and fails on NaN / Inf patterns.
__global__ __launch_bounds__(256) void lds_poison_kernel(unsigned long long pattern, unsigned long long* sink) {
  __shared__ unsigned long long s[20000];
  for (int i = threadIdx.x; i < 20000; i += 256) s[i] = pattern;
  __syncthreads();
  if (sink && s[(threadIdx.x * 77 + blockIdx.x) % 20000] != pattern) *sink = 1ull;  // (keeps the stores alive)
}
// ... and every vector register (256 architectural + 256 accumulation, one 512-register wavefront per SIMD, several rounds over the
// chip): a new wavefront inherits whatever the last one left in the register file.
#include "reg_poison_asm.h"
__global__ __launch_bounds__(64, 1) void reg_poison_kernel(int* sink) {
  asm volatile(QRW_REG_POISON_ASM ::: QRW_REG_POISON_CLOBBERS);
  if (sink && threadIdx.x == 9999) *sink = 1;
}
// Both fills, `rounds` times the smallest grids, on `stream`.
static void poison_launch(int rounds, unsigned long long pattern, hipStream_t stream) {
  hipLaunchKernelGGL(lds_poison_kernel, dim3(2048 * rounds), dim3(256), 0, stream, pattern, (unsigned long long*)nullptr);
  hipLaunchKernelGGL(reg_poison_kernel, dim3(4096 * rounds), dim3(64), 0, stream, (int*)nullptr);
}
// QRW_DEBUG_POISON_LDS=1 (diagnostic): every MPC / WBC / fused control-iteration launch of the library is preceded by that fill with NaN, on the
// launch's stream -- the whole GPU test suite can then be run with "no kernel may depend on LDS leftovers" as an extra condition.
void qrw::host::debug_poison_lds(hipStream_t stream) {
  static const bool on = getenv("QRW_DEBUG_POISON_LDS") && atoi(getenv("QRW_DEBUG_POISON_LDS")) != 0;
  if (on) poison_launch(1, ~0ull, stream);
}

// Known-answer check of THIS build of mpc_solve_kernel, run by qrw_create once per process, device and INSTANTIATION the
// handle will launch (and by qrw_selftest_sweeps for all of them).  Why it exists: the kernel lives at the edge of the register
// file, and one combination of compiler options (docs/HISTORY.md 6b) has produced a library in which every solve diverges; the parity
// tests catch that, a deployment that only rebuilds the library would not -- and each of the ten instantiations is its own piece
// of generated code (the N = 32 forms sit closest to the register limit).  Case: the reference's four-stance immobile scenario
// (scripts/test_mpc.py:54-62: height 0.2447..., feet at (+-0.195, +-0.147)), first MPC call, at the handle's own horizon N.
// Expected values per N: kat_table.h, generated from the CPU restatement by scripts/make_kat_table.py (N = 16: 350 ADMM
// iterations with one rho adaptation at iteration 200, rho 1.03905792582975e-3, four equal vertical forces summing to
// 24.5347812847 N against m g = 24.525 N, horizontal forces zero; N = 32: 375 iterations).
//   mode kKatPlain:    mpc_launch                (<1,true> N = 16, <1,false> N < 16, <2,true> N = 32, <2,false> 16 < N < 32)
//   mode kKatSliced:   mpc_preemptive_launch     (N > 16: the solve is cut after 200 iterations, parked, taken from the queue by
//                                                 another workgroup and finished -- the time-sliced form config 4 runs by default)
//   mode kKatSequence: mpc_sequence_launch, K = 1 (the SEQ instantiations of qrw_mpc_solve_sequence)
static const char* const kKatModeName[kKatModes] = {"one launch per call", "time-sliced launch", "sequence launch"};
struct KatResult { int iters = -1, status = 0, want_iters = 0; double err = 0.0, rho = 0.0, want_rho = 0.0; };
// (rc < 0: -13 bad case, -10 allocation / upload, -11 launch, -12 read-back)
static int mpc_known_answer_check(int N, int mode, KatResult* res) {
  if (N < 1 || N > qrw::kMpcMaxN || mode < 0 || mode >= kKatModes || (mode == kKatSliced && N <= 16)) return -13;
  const int Ng = N > 20 ? N : 20, T = qrw::mpc_threads(N);
  const qrw::KatRow& want = qrw::kKatTable[N];
  std::vector<double> hx(12 * (N + 1), 0.0), hf((size_t)Ng * 12, 0.0), hout(24 * N);
  for (int c = 0; c <= N; c++) hx[2 * (N + 1) + c] = 0.24474949993103629;
  const double feet[12] = {0.195, 0.147, 0., 0.195, -0.147, 0., -0.195, 0.147, 0., -0.195, -0.147, 0.};
  for (int k = 0; k < N; k++) for (int i = 0; i < 12; i++) hf[k * 12 + i] = feet[i];
  DevBuf<double> bx, bf, bo, bst, bd;
  DevBuf<int> bg, bi, bq;
  DevBuf<unsigned> bc;
  const size_t n_int = 16, n_dbl = 16;
  constexpr int kChunk = 200, kCmax = 4000 / kChunk, kLevels = 2;  // sliced: one parked solve at a time, 19 queue-fed workgroups
  const size_t q_ints = (size_t)kLevels * (kCmax - 1) + 8;         // (also covers the sequence launch's one-task queue)
  const size_t c_words = qrw::kPreCtrWords > qrw::kSeqQctrWords ? qrw::kPreCtrWords : qrw::kSeqQctrWords;
  // a private non-blocking stream: the check neither waits for nor stalls the work other streams of the process have queued
  // (the fills and copies below are ordered before the launch by the stream itself; it drains before the buffers above go)
  struct Stream { hipStream_t s = nullptr; ~Stream() { if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } } st;
  if (hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking) != hipSuccess) return -10;
  hipError_t e = hipSuccess;
  auto dev = [&](auto& b, size_t count, int byte, const void* src) {  // allocated, then filled with `byte` or with what is at `src`
    if (e == hipSuccess && (e = b.alloc(count)) == hipSuccess)
      e = src ? hipMemcpyAsync(b.p, src, b.bytes, hipMemcpyHostToDevice, st.s) : b.fill(byte, st.s);
  };
  dev(bx, hx.size(), 0, hx.data());
  dev(bf, hf.size(), 0, hf.data());
  dev(bo, hout.size(), 0xFF, nullptr);
  dev(bst, (size_t)qrw::kMpcStItems * T, 0, nullptr);
  dev(bg, (size_t)Ng * 4, 0, nullptr);
  dev(bi, n_int, 0, nullptr);
  dev(bd, n_dbl, 0, nullptr);
  dev(bq, q_ints, 0xFF, nullptr);
  dev(bc, c_words, 0, nullptr);
  if (e != hipSuccess) return -10;
  qrw::MpcArgs a;
  memset(&a, 0, sizeof(a));
  a.B = 1; a.N = N; a.N_gait = Ng; a.dt = 0.02;
  a.xref = bx; a.fsteps = bf; a.num_iter = nullptr; a.num_iter_scalar = 0;
  a.out = bo; a.st = bst; a.gait = bg;
  int* ip = bi; double* dp = bd;
  a.flags = ip; a.iters = ip + 1; a.status = ip + 2; a.rho_updates = ip + 3;
  a.rho_out = dp; a.pri = dp + 1; a.dua = dp + 2; a.prof = nullptr; a.order = nullptr;
  int lrc;
  if (mode == kKatSliced) {
    a.pre_chunk = kChunk; a.pre_cmax = kCmax; a.pre_cap = kCmax - 1; a.pre_levels = kLevels; a.pre_bin = 200;
    a.pre_queue = bq; a.pre_ctr = bc; a.pause_it = ip + 8;
    lrc = qrw::mpc_preemptive_launch(a, /*resident_slots=*/1 << 20, st.s);  // (one instance: always the two-grid form)
  } else if (mode == kKatSequence) {
    a.seq_K = 1; a.queue = bq; a.qctr = bc; a.seq_hot = ip + 9; a.seq_first = ip + 10; a.seq_groups = 1; a.seq_iters = ip + 11;
    lrc = qrw::mpc_sequence_launch(a, st.s);
  } else {
#ifdef QRW_DEBUG_POISON
    if (const char* sel = getenv("QRW_DEBUG_POISON_SEL")) a.pre_bin = atoi(sel);  // diagnostic build: mpc_kernel.hip, top of the kernel
#endif
    lrc = qrw::mpc_launch(a, st.s);
  }
  if (lrc != 0) return -11;
  int hi[n_int]; double hd[n_dbl]; unsigned hc[8] = {0};
  auto back = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st.s);
  };
  back(hi, bi, sizeof(hi));
  back(hd, bd, sizeof(hd));
  back(hout.data(), bo, hout.size() * sizeof(double));
  if (mode == kKatSliced) back(hc, bc + qrw::kPreErrWord, sizeof(unsigned));
  if (mode == kKatSequence) back(hc, bc + qrw::kSeqErrWord, sizeof(unsigned));
  if (e != hipSuccess || hipStreamSynchronize(st.s) != hipSuccess) return -12;
  double err = 0.0, fz = 0.0;
  for (int j = 0; j < 4; j++) {
    fz += hout[(12 + 3 * j + 2) * N];
    err = fmax(err, fabs(hout[(12 + 3 * j + 2) * N] - hout[14 * N]));      // equal vertical forces
    err = fmax(err, fabs(hout[(12 + 3 * j) * N]) + fabs(hout[(12 + 3 * j + 1) * N]));  // no horizontal force
  }
  err = fmax(err, fabs(fz - want.fz));
  err = fmax(err, fabs(hd[0] / want.rho - 1.0));
  if (hc[0] != 0) err = 1e300;       // the queue of the time-sliced / sequence launch gave up
  if (!(err == err)) err = 1e300;  // NaN
  if (res) { res->iters = hi[1]; res->status = hi[2]; res->err = err; res->rho = hd[0]; res->want_iters = want.iters; res->want_rho = want.rho; }
  // The pass criterion is the ANSWER (status solved, forces and rho to 1e-8).  The iteration count is reported, and
  // only checked loosely: the table's value with the shipped toolchain; a legitimate compiler change may move a borderline
  // termination test by one check interval (25), a miscompiled kernel diverges (status != solved) or lands far away.
  return (hi[2] == qrw::kStatusSolved && err < 1e-8 && hi[1] >= want.iters - 50 && hi[1] <= want.iters + 50) ? 0 : 1;
}
// per device, horizon and launch form: 0 not run, 1 passed, -1 failed; guarded by a mutex (qrw_create may be called from several threads)
static std::mutex g_kat_mutex;
static signed char g_kat_state[64][qrw::kMpcMaxN + 1][kKatModes] = {};
static KatResult g_kat_last;  // result of the most recent check (read under the mutex by the caller that ran it)
static int mpc_known_answer_once(int device, int N, int mode, KatResult* out) {
  if (device < 0 || device >= 64 || N < 1 || N > qrw::kMpcMaxN) return 0;
  std::lock_guard<std::mutex> lock(g_kat_mutex);
  signed char& state = g_kat_state[device][N][mode];
  if (state == 0) {
    const char* skip = getenv("QRW_SKIP_SELFTEST");  // escape hatch (e.g. bring-up on a new toolchain): say so, loudly
    if (skip && skip[0] == '1') {
      fprintf(stderr, "libqrw_hip: QRW_SKIP_SELFTEST=1, the known-answer self-test of mpc_solve_kernel is SKIPPED\n");
      state = 1;
    } else {
      const int rc = mpc_known_answer_check(N, mode, &g_kat_last);
      if (rc < 0) g_kat_last.status = rc;
      state = (rc == 0) ? 1 : -1;
    }
  }
  if (out) *out = g_kat_last;
  return state == 1 ? 0 : 1;
}
int qrw::host::mpc_known_answer_gate(const char* who, int device, int N, int mode) {
  KatResult r;
  if (mpc_known_answer_once(device, N, mode, &r) == 0) return 0;
  char msg[640];
  snprintf(msg, sizeof(msg),
           "%s: the known-answer self-test of mpc_solve_kernel failed on this device for horizon N = %d, %s (got %d ADMM iterations, "
           "status %d, rho %.10g, error %.3g; expected %d, solved, %.10g, < 1e-8): this build of libqrw_hip.so computes wrong results "
           "(a code-generation problem seen with non-shipped compiler options, docs/HISTORY.md 6b); rebuild with the Makefile's flags "
           "(QRW_SKIP_SELFTEST=1 skips this check)", who, N, kKatModeName[mode], r.iters, r.status, r.rho, r.err, r.want_iters, r.want_rho);
  return fail(-20, msg);
}

extern "C" int qrw_selftest_sweeps(double* max_err) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-2, "qrw_selftest_sweeps: no HIP device");
  std::lock_guard<std::mutex> lock(g_kat_mutex);  // one self-test at a time (qrw_create's known-answer check takes the same lock)
  const int rc = qrw::sweeps_selftest(max_err);
  if (rc != 0) return rc;
  // the whole solve, not only its sweeps: every instantiation of mpc_solve_kernel (compile-time and runtime horizon, one and two
  // wavefronts, one launch per call / time-sliced / sequence)
  static const int kat_cases[][2] = {{16, kKatPlain}, {12, kKatPlain}, {32, kKatPlain}, {24, kKatPlain}, {32, kKatSliced}, {24, kKatSliced},
                                     {16, kKatSequence}, {12, kKatSequence}, {32, kKatSequence}, {24, kKatSequence}};
  for (const auto& kc : kat_cases) {
    KatResult kat;
    const int krc = mpc_known_answer_check(kc[0], kc[1], &kat);
    if (krc != 0) {
      char msg[320];
      snprintf(msg, sizeof(msg), "qrw_selftest_sweeps: known-answer MPC solve failed for N = %d, %s (rc %d: %d iterations, status %d, rho %.10g, "
               "error %.3g; expected %d iterations, rho %.10g)", kc[0], kKatModeName[kc[1]], krc, kat.iters, kat.status, kat.rho, kat.err,
               kat.want_iters, kat.want_rho);
      return fail(2, msg);
    }
  }
  return 0;
}

extern "C" int qrw_test_known_answer(int32_t N, int32_t mode, uint64_t lds_pattern, int32_t poison, int32_t* iters, int32_t* status,
                                     double* rho, double* err) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(-2, "qrw_test_known_answer: no HIP device");
  std::lock_guard<std::mutex> lock(g_kat_mutex);
  if (poison) {
    poison_launch(2, (unsigned long long)lds_pattern, nullptr);
    HIP_OK(hipGetLastError(), "qrw_test_known_answer poison launch");
    HIP_OK(hipDeviceSynchronize(), "qrw_test_known_answer poison");
  }
  KatResult r;
  const int rc = mpc_known_answer_check(N, mode, &r);
  if (iters) *iters = r.iters;
  if (status) *status = r.status;
  if (rho) *rho = r.rho;
  if (err) *err = r.err;
  return rc;
}

// Tests only: is the poisoning itself effective on this device?  After both fills a probe wavefront reads, without writing them first,
// one LDS word, v255 and a255: out[0..2] (all-ones if the leftovers are what a new wavefront sees; the hardware clears neither).
__global__ __launch_bounds__(64, 1) void poison_probe_kernel(unsigned* out) {
  __shared__ unsigned s[40000];  // (the whole LDS of the compute unit: the word read below is inside the allocation)
  unsigned v, acc, w;
  const unsigned addr = (unsigned)(size_t)(&s[39000]) + 4u * threadIdx.x;
  // (through asm: the compiler folds a plain read of never-written shared memory to a constant)
  asm volatile("v_mov_b32 %0, v255\n\tv_accvgpr_read_b32 %1, a255\n\tds_read_b32 %2, %3\n\ts_waitcnt lgkmcnt(0)"
               : "=v"(v), "=v"(acc), "=v"(w) : "v"(addr) : "v255", "a255", "memory");
  if (threadIdx.x == 5) { out[0] = w; out[1] = v; out[2] = acc; }
}
extern "C" int qrw_test_poison_probe(uint32_t* h_out3) {
  if (!h_out3) return fail(-1, "qrw_test_poison_probe: null argument");
  std::lock_guard<std::mutex> lock(g_kat_mutex);
  DevBuf<unsigned> d;
  HIP_OK(d.alloc(3), "qrw_test_poison_probe alloc");
  HIP_OK(hipMemset(d, 0, d.bytes), "qrw_test_poison_probe memset");
  poison_launch(2, ~0ull, nullptr);
  hipLaunchKernelGGL(poison_probe_kernel, dim3(1), dim3(64), 0, nullptr, d.p);
  HIP_OK(hipDeviceSynchronize(), "qrw_test_poison_probe");
  HIP_OK(hipMemcpy(h_out3, d, d.bytes, hipMemcpyDeviceToHost), "qrw_test_poison_probe D2H");
  return 0;
}

extern "C" int qrw_test_poke_aborted(qrw_handle h, int32_t parked_at) {
  if (!h || parked_at < 1) return fail(-1, "qrw_test_poke_aborted: bad argument");
  if (!h->pause_it || !mpc_time_sliced(h)) return fail(-1, "qrw_test_poke_aborted: not a time-sliced handle");
  DeviceScope dev_scope__(h->cfg.device);
  HIP_OK(wait_family(h, kFamMpc), "qrw_test_poke_aborted sync");
  const size_t B = h->cfg.batch, T = qrw::mpc_threads(h->cfg.n_steps);
  std::vector<int> pit(B, parked_at);
  HIP_OK(hipMemcpy(h->pause_it, pit.data(), B * sizeof(int), hipMemcpyHostToDevice), "qrw_test_poke_aborted pause_it");
  // the iterate slots (items kStXX .. kStYC + 4) and rho: anything but what the last finished solve left
  std::vector<double> st((size_t)qrw::kMpcStItems * T);
  for (size_t b = 0; b < B; b++) {
    double* d = h->mpc_st + b * qrw::kMpcStItems * T;
    HIP_OK(hipMemcpy(st.data(), d, st.size() * sizeof(double), hipMemcpyDeviceToHost), "qrw_test_poke_aborted D2H");
    for (size_t e = 0; e < (size_t)qrw::kStB * T; e++) st[e] = 3.7 * st[e] + 1.0 + 0.01 * (double)(e % 17);
    for (size_t e = 0; e < T; e++) st[(size_t)qrw::kStRho * T + e] = 0.37;
    HIP_OK(hipMemcpy(d, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice), "qrw_test_poke_aborted H2D");
  }
  return 0;
}

// Tests only: the simulator's forward dynamics alone, for n states given in host buffers (no handle state is read or written).
extern "C" int qrw_test_sim_forward_dynamics(qrw_handle h, int32_t n, const double* h_q19, const double* h_v18, const double* h_tau12,
                                             const double* h_f_ext, const qrw_sim_params* params, double* h_a18, double* h_contact_forces) {
  if (!h || n < 1 || !h_q19 || !h_v18 || !h_tau12 || !params || !h_a18 || !h_contact_forces)
    return fail(-1, "qrw_test_sim_forward_dynamics: bad argument");
  DeviceScope dev_scope__(h->cfg.device);
  const size_t N = (size_t)n;
  // the handle's terrain is used as in the other modes; its per-robot origins hold one row per instance of the handle's batch
  if (h->sim_terrain_on && h->sim_origin_on && n > h->cfg.batch)
    return fail(-1, "qrw_test_sim_forward_dynamics: more states than the terrain's per-robot origins (the handle's batch)");
  DevBuf<double> q, v, tau, fe, a18, cf;
  HIP_OK(q.alloc(N * 19), "qrw_test_sim_forward_dynamics alloc");
  HIP_OK(v.alloc(N * 18), "qrw_test_sim_forward_dynamics alloc");
  HIP_OK(tau.alloc(N * 12), "qrw_test_sim_forward_dynamics alloc");
  HIP_OK(a18.alloc(N * 18), "qrw_test_sim_forward_dynamics alloc");
  HIP_OK(cf.alloc(N * 12), "qrw_test_sim_forward_dynamics alloc");
  HIP_OK(hipMemcpy(q, h_q19, q.bytes, hipMemcpyHostToDevice), "qrw_test_sim_forward_dynamics H2D");
  HIP_OK(hipMemcpy(v, h_v18, v.bytes, hipMemcpyHostToDevice), "qrw_test_sim_forward_dynamics H2D");
  HIP_OK(hipMemcpy(tau, h_tau12, tau.bytes, hipMemcpyHostToDevice), "qrw_test_sim_forward_dynamics H2D");
  if (h_f_ext) {
    HIP_OK(fe.alloc(N * 6), "qrw_test_sim_forward_dynamics alloc");
    HIP_OK(hipMemcpy(fe, h_f_ext, fe.bytes, hipMemcpyHostToDevice), "qrw_test_sim_forward_dynamics H2D");
  }
  qrw::SimArgs a;
  memset(&a, 0, sizeof(a));
  a.B = n; a.mode = 2; a.substeps = 1; a.dt = params->dt;
  a.kn = params->kn; a.dn = params->dn; a.mu = params->mu; a.vs = params->vs; a.foot_radius = params->foot_radius;
  a.fd_q = q; a.fd_v = v; a.fd_tau = tau; a.f_ext = h_f_ext ? fe.p : nullptr; a.fd_a = a18; a.contact_forces = cf;
  HIP_OK(wait_family(h, kFamSim), "qrw_test_sim_forward_dynamics: earlier simulator work of this handle");  // (a terrain copy in flight)
  sim_terrain_args(h, a);
  if (qrw::sim_launch(a, h->host_stream) != 0) return fail(-11, "qrw_test_sim_forward_dynamics: launch failed", hipGetLastError());
  HIP_OK(hipStreamSynchronize(h->host_stream), "qrw_test_sim_forward_dynamics");
  HIP_OK(hipMemcpy(h_a18, a18, a18.bytes, hipMemcpyDeviceToHost), "qrw_test_sim_forward_dynamics D2H");
  HIP_OK(hipMemcpy(h_contact_forces, cf, cf.bytes, hipMemcpyDeviceToHost), "qrw_test_sim_forward_dynamics D2H");
  return 0;
}
