"""What the joystick stage costs per control iteration, measured on the GPU with device events, against the qrw_control_pre
launch of the same run (the yardstick) and against the host-side alternative it replaces:

    python scripts/gpu_joystick_timing.py [rounds=10] [calls per round and leg=200]   ->  profiles/joystick_timing.json

Batch 4096 and 256, one process, the legs alternating round by round (the method of scripts/gpu_estimator_timing.py, whose
set-up and timer this imports):
  (a) iteration        the state-in non-solving iteration, qrw_iteration_step
  (b) joy+iteration    the same preceded by qrw_joystick_step on the same stream (the iteration's own inputs unchanged)
  (c) joystick         qrw_joystick_step alone: profile mode (8 columns), 2 pushes, 1 code per robot
  (d) control_pre      qrw_control_pre alone (non-solving form)
`device` = the calls queued behind a blocker kernel and timed by two events once it ends; `issued` = the same calls timed while
the host issues them.  Beside these, in HOST time (time.perf_counter, no device events): `host_alternative` = the numpy
evaluation of the same tables for all B robots (vectorised over the fleet) plus the three copy_ calls that would bring
v_ref, code and f_ext to the device, per tick."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-reactive-walking_amd"), os.path.join(ROOT, "scripts")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gpu_estimator_timing as get  # noqa: E402
import qrw_hip  # noqa: E402

ARGS = sys.argv[1:]
ROUNDS = int(ARGS[0]) if len(ARGS) > 0 else 10
CALLS = int(ARGS[1]) if len(ARGS) > 1 else 200
LEGS = ("iteration", "joy+iteration", "joystick", "control_pre")


def tables(B):
    rng = np.random.default_rng(3)
    K = np.concatenate([np.zeros((B, 1), np.int64), np.cumsum(rng.integers(200, 3000, size=(B, 7)), axis=1)], axis=1).astype(np.int32)
    V = rng.normal(size=(B, 6, 8)) * 0.3
    V[:, :, 0] = 0.0
    code_k, code_v = rng.integers(0, 20000, size=(B, 1)).astype(np.int32), rng.integers(1, 5, size=(B, 1)).astype(np.int32)
    push_k = np.stack([rng.integers(0, 20000, size=(B, 2)), rng.integers(100, 1000, size=(B, 2))], axis=-1).astype(np.int32)
    push_w = rng.normal(size=(B, 2, 6))
    return K, V, code_k, code_v, push_k, push_w


def host_alternative(tab, dev):
    """The same outputs from numpy, all robots at once, and their way to the device: what a host-side joystick costs per tick."""
    K, V, code_k, code_v, push_k, push_w = tab
    B = K.shape[0]
    K64, rows = K.astype(np.int64), np.arange(B)
    d_v = torch.zeros((B, 6), dtype=torch.float64, device=dev)
    d_c = torch.zeros((B,), dtype=torch.int32, device=dev)
    d_f = torch.zeros((B, 6), dtype=torch.float64, device=dev)

    def tick(k):
        ke = np.minimum(k, K64[:, -1] - 1)
        i = np.minimum((K64 <= ke[:, None]).sum(axis=1), K.shape[1] - 1)
        lo, hi = K64[rows, i - 1], K64[rows, i]
        ev, t1 = (ke - lo).astype(np.float64), (hi - lo).astype(np.float64)
        v0, v1 = V[rows, :, i - 1], V[rows, :, i]
        A3 = 2 * (v0 - v1) / (t1**3)[:, None]
        A2 = (-3 / 2) * t1[:, None] * A3
        v = v0 + A2 * (ev**2)[:, None] + A3 * (ev**3)[:, None]
        code = np.where(code_k[:, 0] == k, code_v[:, 0], 0).astype(np.int32)
        e, t = (k - push_k[:, :, 0]).astype(np.float64), push_k[:, :, 1].astype(np.float64)
        A4 = 16 / t**4
        alpha = np.where((e >= 0) & (e <= t), (t**2 * A4) * e**2 + (-2 * t * A4) * e**3 + A4 * e**4, 0.0)
        f = (alpha[:, :, None] * push_w).sum(axis=1)
        d_v.copy_(torch.from_numpy(v))
        d_c.copy_(torch.from_numpy(code))
        d_f.copy_(torch.from_numpy(f))

    return tick


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    out = {"rounds": ROUNDS, "calls_per_round": CALLS, "unit": "us per call", "batches": {}}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        for B in (4096, 256):
            ctl, est_legs = get.legs_of(B, dev)
            tab = tables(B)
            K, V, code_k, code_v, push_k, push_w = tab
            ctl._b.joystick_init(qrw_hip.JOY_PROFILE, k_switch=K, v_switch=V, code_k=code_k, code_v=code_v, push_k=push_k, push_w=push_w)
            # The stage writes a tensor of its own, NOT the iteration's bound reference velocity: the iteration's device time depends on
            # its data (measured with the stage writing it in place: +37 us at batch 4096, against 5.5 us for the stage alone), and
            # (b) - (a) is to be the cost of the extra launch on the same stream, not of other velocities.
            vref = torch.zeros((B, 6), dtype=torch.float64, device=dev)
            code = torch.zeros((B,), dtype=torch.int32, device=dev)
            f_ext = torch.zeros((B, 6), dtype=torch.float64, device=dev)
            stop = torch.zeros((B,), dtype=torch.int32, device=dev)  # (read like the controller's error flags; nobody stops)
            lib, h, stream = ctl._b._lib, ctl._b._handle, torch.cuda.current_stream(dev).cuda_stream
            kk = [0]

            def joystick():
                kk[0] += 1
                if lib.qrw_joystick_step(h, kk[0], None, stop.data_ptr(), vref.data_ptr(), code.data_ptr(), f_ext.data_ptr(),
                                         stream):
                    raise RuntimeError(lib.qrw_last_error().decode())

            def both():
                joystick()
                est_legs["iteration"]()

            legs = dict(zip(LEGS, (est_legs["iteration"], both, joystick, est_legs["control_pre"])))
            for fn in legs.values():
                get.timed(fn, CALLS, False)
            rec = {name: {"device": [], "issued": []} for name in LEGS}
            host, alt = [], host_alternative(tab, dev)
            for _ in range(ROUNDS):
                for name in LEGS:
                    rec[name]["device"].append(get.timed(legs[name], CALLS, True))
                for name in LEGS:
                    rec[name]["issued"].append(get.timed(legs[name], CALLS, False))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for k in range(CALLS):
                    alt(1000 + k)
                host.append(1e6 * (time.perf_counter() - t0) / CALLS)
            res = {name: {kind: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                          for kind, v in kinds.items()} for name, kinds in rec.items()}
            res["host_alternative_host_time"] = {"median": float(np.median(host)), "min": float(np.min(host)), "max": float(np.max(host))}
            res["extra_launch_device"] = res["joy+iteration"]["device"]["median"] - res["iteration"]["device"]["median"]
            res["extra_launch_issued"] = res["joy+iteration"]["issued"]["median"] - res["iteration"]["issued"]["median"]
            res["error_flags_set"] = int((ctl.error_flag != 0).sum().item())
            res["robots_stopped_by_the_latch"] = int((ctl._b.joystick_get("k_stop") >= 0).sum())
            out["batches"][str(B)] = res
            print(B, json.dumps(res))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "joystick_timing.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
