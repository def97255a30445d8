"""What one tick of the rigid-body simulator costs, measured on the GPU with device events, beside the existing launches of the
same run (the yardsticks):

    python scripts/gpu_sim_timing.py [rounds=10] [calls per round and leg=200]   ->  profiles/sim_timing.json

Batch 4096 and 256, one process, the four legs alternating round by round (>= 2000 calls per leg in all):
  (a) sim_step_8     qrw_sim_step with the default 8 sub-steps
  (b) sim_step_1     qrw_sim_step with 1 sub-step (a handle of its own)
  (c) control_pre    qrw_control_pre alone (non-solving form)
  (d) iteration      the state-in non-solving iteration, qrw_iteration_step (control_pre + wbc_compute_result)
Two figures per leg, microseconds per call, as scripts/gpu_estimator_timing.py takes them: `device` = the calls queued behind a
blocker kernel and timed by two events once it ends; `issued` = the same calls timed while the host issues them.
The simulated robots hold the stance under P = 3, D = 0.2 and are re-initialised before every timed window (outside it); `frozen`
counts robots whose status was set in a window -- a frozen robot's quad leaves early, so a figure with frozen robots is too low.

    python scripts/gpu_sim_timing.py --terrain [rounds=10] [calls=200]          ->  profiles/sim_terrain_timing.json

The two instantiations of sim_kernel side by side, by the same method: `flat` = qrw_sim_step (8 sub-steps) on a handle without a
terrain, `terrain` = the same on a second handle that holds the reference's rough ground (Simulator.reference_rough_ground, 512 x
512) with one origin per robot on a grid over the field, so that the fleet's height loads spread over the whole 2 MiB.  The two
legs alternate round by round in one process, at batch 4096 and 256.  The flat figure is the one to hold against
profiles/sim_timing.json (sim_step_8): that file's run-to-run spread is its min..max."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "quadruped-reactive-walking_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import qrw_hip  # noqa: E402
import synth  # noqa: E402
from Controller import Controller_batch  # noqa: E402

TERRAIN = "--terrain" in sys.argv
ARGV = [a for a in sys.argv if a != "--terrain"]
ROUNDS = int(ARGV[1]) if len(ARGV) > 1 else 10
CALLS = int(ARGV[2]) if len(ARGV) > 2 else 200
Q_INIT = np.array([0.0, 0.7, -1.4, -0.0, 0.7, -1.4, 0.0, -0.7, +1.4, -0.0, -0.7, +1.4])
LEGS = ("sim_step_8", "sim_step_1", "control_pre", "iteration")


def sim_leg(b, substeps, dev):
    """(tick, reset, frozen) on handle b (whatever terrain it holds): argument-free callables on fixed buffers."""
    B = b.B
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    q0, out = t(np.tile(Q_INIT, (B, 1))), b.sim_outputs()
    cmd = [t(np.full((B, 12), 3.0)), t(np.full((B, 12), 0.2)), q0, t(np.zeros((B, 12))), t(np.zeros((B, 12)))]
    bufs = b._sim_buffers(out)
    lib, stream = b._lib, torch.cuda.current_stream(dev).cuda_stream
    args = [b._handle] + [x.data_ptr() for x in cmd] + [12, None, C.byref(bufs), stream]
    keep = (q0, out, cmd, bufs)

    def tick():
        if lib.qrw_sim_step(*args):
            raise RuntimeError(lib.qrw_last_error().decode())

    reset = lambda: b.sim_init(q0, out, substeps=substeps)
    frozen = lambda: int(b.sim_state()["status"].sum())
    reset()
    return tick, reset, frozen, keep


def legs_of(B, dev):
    ctl = Controller_batch(B, Q_INIT, estimator=dict(h_init=0.22294615))
    sen = synth.SyntheticSensors(B, 1)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    vref = t(np.tile(np.array([0.3, 0.0, 0, 0, 0, 0.1]), (B, 1)))
    s = [t(sen.step(0)[k]) for k in ("lin_acc", "ang_vel", "quat", "q_mes", "v_mes")]
    for k in range(13):  # two solves, the iteration bound (Controller_batch._nonsolve_fast)
        ctl.compute_sensors(vref, *s)
    torch.cuda.synchronize()
    lib, h = ctl._b._lib, ctl._b._handle
    step, x_f_mpc = ctl._fast[0], ctl.x_f_mpc
    vp = lambda x: None if x is None else x.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = ctl._pre
    pre_args = ([h, 0, vp(vref), vp(ctl.q_filt), vp(ctl.v_filt), vp(ctl.rpy), None, 0, vp(x_f_mpc)]
                + [vp(p[n]) for n in ("q", "v", "h_v", "v_ref", "oRh_oTh", "xref")] + [None, None]
                + [vp(p[n]) for n in ("target", "feet_pva", "contacts", "x_f_wbc", "q_wbc", "b_v", "f_cmd", "feet_cmd")] + [stream])
    k0 = [ctl.k]

    def next_k():  # never a multiple of k_mpc: the iteration that does not solve
        k0[0] += 2 if (k0[0] + 1) % ctl.k_mpc == 0 else 1
        return k0[0]

    def control_pre():
        pre_args[1] = next_k()
        if lib.qrw_control_pre(*pre_args):
            raise RuntimeError(lib.qrw_last_error().decode())

    iteration = lambda: step(next_k(), x_f_mpc)
    sim8 = sim_leg(ctl._b, 8, dev)
    sim1 = sim_leg(qrw_hip.Batch(B), 1, dev)
    nothing = lambda: None
    legs = dict(zip(LEGS, (sim8[0], sim1[0], control_pre, iteration)))
    resets = dict(zip(LEGS, (sim8[1], sim1[1], nothing, nothing)))
    frozen = dict(zip(LEGS, (sim8[2], sim1[2], lambda: 0, lambda: 0)))
    return (ctl, sim8, sim1, s), legs, resets, frozen


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


def main():
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    out = {"rounds": ROUNDS, "calls_per_round": CALLS, "unit": "us per call", "batches": {}}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        for B in (4096, 256):
            keep, legs, resets, frozen = legs_of(B, dev)
            for name in LEGS:  # warm-up of every leg
                timed(legs[name], CALLS, False)
            rec = {name: {"device": [], "issued": []} for name in LEGS}
            stuck = {name: 0 for name in LEGS}
            for _ in range(ROUNDS):
                for kind, blocked in (("device", True), ("issued", False)):
                    for name in LEGS:
                        resets[name]()
                        torch.cuda.current_stream().synchronize()
                        rec[name][kind].append(timed(legs[name], CALLS, blocked))
                        stuck[name] = max(stuck[name], frozen[name]())
            res = {name: {kind: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                          for kind, v in kinds.items()} for name, kinds in rec.items()}
            for name in LEGS[:2]:
                res[name]["frozen"] = stuck[name]
            res["sim_step_8_over_control_pre"] = res["sim_step_8"]["device"]["median"] / res["control_pre"]["device"]["median"]
            res["per_substep"] = (res["sim_step_8"]["device"]["median"] - res["sim_step_1"]["device"]["median"]) / 7.0
            out["batches"][str(B)] = res
            print(B, json.dumps(res))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "sim_timing.json"), "w"), indent=1, sort_keys=True)


def main_terrain():
    assert torch.cuda.is_available(), "needs a GPU"
    from Simulator import reference_rough_ground

    dev = torch.device("cuda", 0)
    ground = reference_rough_ground()
    legs = ("flat", "terrain")
    out = {"rounds": ROUNDS, "calls_per_round": CALLS, "unit": "us per call", "substeps": 8,
           "field": "reference_rough_ground(): 512 x 512, 0.05 m, one origin per robot on a grid", "batches": {}}
    with torch.cuda.stream(torch.cuda.Stream(dev)):
        for B in (4096, 256):
            side = int(np.ceil(np.sqrt(B)))
            at = np.linspace(ground["x0"] + 2.0, -ground["x0"] - 2.0, side)
            origin = np.stack(np.meshgrid(at, at), axis=-1).reshape(-1, 2)[:B].copy()
            flat, rough = qrw_hip.Batch(B), qrw_hip.Batch(B)
            rough.sim_set_terrain(ground["heights"], ground["dx"], ground["dy"], x0=ground["x0"], y0=ground["y0"], origin=origin)
            leg = {"flat": sim_leg(flat, 8, dev), "terrain": sim_leg(rough, 8, dev)}
            for name in legs:
                timed(leg[name][0], CALLS, False)
            rec = {name: {"device": [], "issued": []} for name in legs}
            stuck = {name: 0 for name in legs}
            for _ in range(ROUNDS):
                for kind, blocked in (("device", True), ("issued", False)):
                    for name in legs:
                        tick, reset, frozen, _ = leg[name]
                        reset()
                        torch.cuda.current_stream().synchronize()
                        rec[name][kind].append(timed(tick, CALLS, blocked))
                        stuck[name] = max(stuck[name], frozen())
            res = {name: {kind: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
                          for kind, v in kinds.items()} for name, kinds in rec.items()}
            for name in legs:
                res[name]["frozen"] = stuck[name]
            res["terrain_over_flat"] = res["terrain"]["device"]["median"] / res["flat"]["device"]["median"]
            ref = os.path.join(ROOT, "profiles", "sim_timing.json")
            if os.path.exists(ref):  # the flat figure of the commit before the terrain, and that file's own spread
                was = json.load(open(ref))["batches"][str(B)]["sim_step_8"]["device"]
                res["flat_recorded_before"] = was
                res["flat_over_recorded"] = res["flat"]["device"]["median"] / was["median"]
            out["batches"][str(B)] = res
            print(B, json.dumps(res))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "sim_terrain_timing.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main_terrain() if TERRAIN else main()
