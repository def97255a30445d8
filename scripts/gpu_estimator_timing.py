"""What the state estimator costs per control iteration, measured on the GPU with device events, against the existing
qrw_control_pre launch of the same run (the yardstick):

    python scripts/gpu_estimator_timing.py [rounds=10] [calls per round and leg=200]   ->  profiles/estimator_timing.json
    python scripts/gpu_estimator_timing.py --kalman [rounds] [calls]                   ->  profiles/estimator_kalman_timing.json

Batch 4096 and 256, one process, the four legs alternating round by round (>= 2000 calls per leg in all):
  (a) iteration        the state-in non-solving iteration, qrw_iteration_step (control_pre + wbc_compute_result)
  (b) est+iteration    the same preceded by qrw_estimator_step writing the iteration's bound inputs
  (c) estimator        qrw_estimator_step alone
  (d) control_pre      qrw_control_pre alone (non-solving form)
Two figures per leg, microseconds per call: `device` = the calls queued behind a blocker kernel and timed by two events once it
ends (back-to-back on the device, no host in the window); `issued` = the same calls timed while the host issues them (what a
free-running loop sees: the larger of host issue time and device time).  (b) - (a) is the cost of the extra launch.

--kalman: the Kalman variant of the estimator (qrw_estimator_init_kalman) against the complementary one at the same commit, the
yardstick: two handles of the same batch in one process, the legs `estimator` (complementary) and `kalman_estimator` and the two
`est+iteration` legs alternating round by round, same method."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-reactive-walking_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
from Controller import Controller_batch  # noqa: E402

KALMAN = "--kalman" in sys.argv
ARGS = [a for a in sys.argv[1:] if a != "--kalman"]
ROUNDS = int(ARGS[0]) if len(ARGS) > 0 else 10
CALLS = int(ARGS[1]) if len(ARGS) > 1 else 200
Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])
LEGS = ("iteration", "est+iteration", "estimator", "control_pre")


def legs_of(B, dev, kalman=False):
    """The four legs as argument-free callables on warmed, bound buffers (every call is one or two foreign calls)."""
    ctl = Controller_batch(B, Q_INIT, estimator=dict(h_init=0.22294615, kalman=kalman))
    sen = synth.SyntheticSensors(B, 1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vref = t(np.tile(np.array([0.3, 0.0, 0, 0, 0, 0.1]), (B, 1)))
    s = [t(sen.step(0)[k]) for k in ("lin_acc", "ang_vel", "quat", "q_mes", "v_mes")]
    for k in range(13):  # two solves, the iteration bound (Controller_batch._nonsolve_fast)
        ctl.compute_sensors(vref, *s)
    torch.cuda.synchronize()
    b, lib, h = ctl._b, ctl._b._lib, ctl._b._handle
    step, x_f_mpc = ctl._fast[0], ctl.x_f_mpc
    vp = lambda x: None if x is None else x.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    est_args = [h] + [vp(x) for x in s] + [None] * 4 + [vp(ctl.q_filt), vp(ctl.v_filt), vp(ctl.rpy), vp(ctl.v_secu), stream]
    p = ctl._pre
    pre_args = ([h, 0, vp(vref), vp(ctl.q_filt), vp(ctl.v_filt), vp(ctl.rpy), None, 0, vp(x_f_mpc)]
                + [vp(p[n]) for n in ("q", "v", "h_v", "v_ref", "oRh_oTh", "xref")] + [None, None]
                + [vp(p[n]) for n in ("target", "feet_pva", "contacts", "x_f_wbc", "q_wbc", "b_v", "f_cmd", "feet_cmd")] + [stream])
    k0 = [ctl.k]

    def next_k():  # never a multiple of k_mpc: the iteration that does not solve
        k0[0] += 2 if (k0[0] + 1) % ctl.k_mpc == 0 else 1
        return k0[0]

    def estimator():
        if lib.qrw_estimator_step(*est_args):
            raise RuntimeError(lib.qrw_last_error().decode())

    def control_pre():
        pre_args[1] = next_k()
        if lib.qrw_control_pre(*pre_args):
            raise RuntimeError(lib.qrw_last_error().decode())

    iteration = lambda: step(next_k(), x_f_mpc)

    def both():
        estimator()
        iteration()

    return ctl, dict(zip(LEGS, (iteration, both, estimator, control_pre)))


def timed(fn, calls, blocked):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if blocked:
        torch.cuda._sleep(int(4.0e7))  # ~20 ms: the calls below are all queued when it ends
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / calls


def main_kalman(dev):
    """The Kalman estimator step against the complementary one: alone and in front of the iteration."""
    names = ("estimator", "kalman_estimator", "est+iteration", "kalman_est+iteration")
    out = {"rounds": ROUNDS, "calls_per_round": CALLS, "unit": "us per call", "batches": {}}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        for B in (4096, 256):
            (ctl_c, legs_c), (ctl_k, legs_k) = legs_of(B, dev), legs_of(B, dev, kalman=True)
            legs = dict(zip(names, (legs_c["estimator"], legs_k["estimator"], legs_c["est+iteration"], legs_k["est+iteration"])))
            for fn in legs.values():
                timed(fn, CALLS, False)
            rec = {name: {"device": [], "issued": []} for name in names}
            for _ in range(ROUNDS):
                for name in names:
                    rec[name]["device"].append(timed(legs[name], CALLS, True))
                for name in names:
                    rec[name]["issued"].append(timed(legs[name], CALLS, False))
            res = {name: {kind: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                          for kind, v in kinds.items()} for name, kinds in rec.items()}
            res["kalman_over_complementary_device"] = res["kalman_estimator"]["device"]["median"] / res["estimator"]["device"]["median"]
            res["kalman_extra_per_iteration_device"] = (res["kalman_est+iteration"]["device"]["median"]
                                                        - res["est+iteration"]["device"]["median"])
            res["error_flags_set"] = int((ctl_c.error_flag != 0).sum().item()) + int((ctl_k.error_flag != 0).sum().item())
            out["batches"][str(B)] = res
            print(B, json.dumps(res))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "estimator_kalman_timing.json"), "w"), indent=1, sort_keys=True)


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    if KALMAN:
        return main_kalman(dev)
    out = {"rounds": ROUNDS, "calls_per_round": CALLS, "unit": "us per call", "batches": {}}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        for B in (4096, 256):
            ctl, legs = legs_of(B, dev)
            for fn in legs.values():  # warm-up of every leg
                timed(fn, CALLS, False)
            rec = {name: {"device": [], "issued": []} for name in LEGS}
            for _ in range(ROUNDS):
                for name in LEGS:
                    rec[name]["device"].append(timed(legs[name], CALLS, True))
                for name in LEGS:
                    rec[name]["issued"].append(timed(legs[name], CALLS, False))
            res = {name: {kind: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                          for kind, v in kinds.items()} for name, kinds in rec.items()}
            res["extra_launch_device"] = res["est+iteration"]["device"]["median"] - res["iteration"]["device"]["median"]
            res["extra_launch_issued"] = res["est+iteration"]["issued"]["median"] - res["iteration"]["issued"]["median"]
            res["estimator_no_longer_than_control_pre"] = bool(res["estimator"]["device"]["median"] <= res["control_pre"]["device"]["median"])
            res["error_flags_set"] = int((ctl.error_flag != 0).sum().item())
            out["batches"][str(B)] = res
            print(B, json.dumps(res))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "estimator_timing.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
