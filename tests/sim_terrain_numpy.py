"""numpy restatement of the simulator's contact with a heightfield terrain (csrc/sim_terrain.h, sim_terrain_force in
csrc/sim_dynamics.h), on top of tests/sim_numpy.py, which it imports unchanged: the rigid-body terms, rhs_of, the dense 18x18
solve and the integrator are that module's; only contact_forces is this one's.  TEST CODE: the product never imports it.

Field: heights H[rows][cols], vertex (r, c) at x = x0 + c dx, y = y0 + r dy; every cell cut by the diagonal (r, c) - (r+1, c+1).
A foot at world (xf, yf, zf) of a robot with origin (ox, oy) is looked up at (xf + ox, yf + oy)."""
import numpy as np

import oracle
import sim_numpy as sn

DEFAULTS, Q_STANCE = sn.DEFAULTS, sn.Q_STANCE


class Terrain:
    def __init__(self, heights, dx, dy, x0=0.0, y0=0.0):
        self.H = np.array(heights, dtype=float)
        assert self.H.ndim == 2 and min(self.H.shape) >= 2 and dx > 0 and dy > 0
        self.dx, self.dy, self.x0, self.y0 = float(dx), float(dy), float(x0), float(y0)

    def cell(self, X, Y):
        """(r, c, fu, fv): clamped in floating point before the conversion; a NaN coordinate gives index 0 and a NaN fraction."""
        rows, cols = self.H.shape
        with np.errstate(all="ignore"):
            u, v = (X - self.x0) / self.dx, (Y - self.y0) / self.dy
            tc, tr = np.floor(u), np.floor(v)
            tc = 0.0 if not tc >= 0.0 else min(tc, cols - 2.0)
            tr = 0.0 if not tr >= 0.0 else min(tr, rows - 2.0)
            fu, fv = np.clip(u - tc, 0.0, 1.0), np.clip(v - tr, 0.0, 1.0)  # (np.clip keeps a NaN)
        return int(tr), int(tc), float(fu), float(fv)

    def surface(self, X, Y):
        """(h, gx, gy, (r, c, fu, fv)) of the triangle under (X, Y)."""
        r, c, fu, fv = self.cell(X, Y)
        H = self.H
        h00, h10, h01, h11 = H[r, c], H[r, c + 1], H[r + 1, c], H[r + 1, c + 1]
        if fu >= fv:
            h, gx, gy = h00 + fu * (h10 - h00) + fv * (h11 - h10), (h10 - h00) / self.dx, (h11 - h10) / self.dy
        else:
            h, gx, gy = h00 + fv * (h01 - h00) + fu * (h11 - h01), (h11 - h01) / self.dx, (h01 - h00) / self.dy
        return h, gx, gy, (r, c, fu, fv)


def foot_force(h, gx, gy, zf, v, prm):
    """The force on one foot and its d from the triangle's plane (h, gx, gy) under it."""
    n = np.array([-gx, -gy, 1.0]) / np.sqrt(gx * gx + gy * gy + 1.0)
    d = prm["foot_radius"] - n[2] * (zf - h)
    vn = n @ v
    fn = max(0.0, prm["kn"] * d - prm["dn"] * vn) if d > 0 else 0.0
    vt = v - vn * n
    return fn * n - prm["mu"] * fn * vt / np.sqrt(vt @ vt + prm["vs"] ** 2), d


def contact_forces(q19, v18, prm, terrain, origin=(0.0, 0.0), cells=None):
    """World forces on the four feet (4,3), the distances d (4,) and the feet Jacobian; `cells`, a list, receives one
    (r, c, fu, fv) per foot."""
    R = sn.quat_to_rot(q19[3:7])
    pf_b = oracle.fixed_feet(q19[7:], v18[6:])[0]
    J = oracle.feet_jacobians(q19)
    pw = q19[:3] + pf_b @ R.T
    vw = (J @ v18).reshape(4, 3)
    f, d = np.zeros((4, 3)), np.zeros(4)
    for j in range(4):
        h, gx, gy, cell = terrain.surface(pw[j, 0] + origin[0], pw[j, 1] + origin[1])
        f[j], d[j] = foot_force(h, gx, gy, pw[j, 2], vw[j], prm)
        if cells is not None:
            cells.append(cell)
    return f, d, J


def forward_dynamics(q19, v18, tau12, terrain, origin=(0.0, 0.0), prm=DEFAULTS, f_ext=None, solve=np.linalg.solve, cells=None):
    """a18 with M(q) a = rhs, the contact forces (4,3) and the distances d (4,)."""
    f, d, J = contact_forces(q19, v18, prm, terrain, origin, cells)
    a = solve(oracle.crba(q19), sn.rhs_of(q19, v18, tau12, f, J, f_ext))
    return a, f, d


def init_height(q12, terrain, origin=(0.0, 0.0), base_height=0.2596):
    """Base height of the 12-joint initialisation: base_height above the highest ground under the feet of the level robot at (0, 0)."""
    pf = oracle.fixed_feet(np.asarray(q12, dtype=float), np.zeros(12))[0]
    return base_height + max(terrain.surface(pf[j, 0] + origin[0], pf[j, 1] + origin[1])[0] for j in range(4))


class SimTerrainNumpy(sn.SimNumpy):
    """sim_numpy.SimNumpy on a terrain: its substep (and through it the dense solve and the integrator) with this module's
    contact forces.  Records what the switches of the law came near: min_abs_d (the parent's), min_diag = min |fu - fv|,
    min_edge = min over fu, fv of the distance to 0 or 1, and the triangle kinds seen in contact."""

    def __init__(self, q_init, terrain, origin=(0.0, 0.0), **params):
        q_init = np.asarray(q_init, dtype=float).ravel()
        if q_init.size == 12:
            params = dict(params, base_height=init_height(q_init, terrain, origin, params.get("base_height", 0.2596)))
        super().__init__(q_init, **params)
        self.terrain, self.origin = terrain, tuple(origin)
        self.min_diag, self.min_edge, self.kinds = np.inf, np.inf, set()

    def _contact(self, q19, v18, prm):
        cells = []
        f, d, J = contact_forces(q19, v18, prm, self.terrain, self.origin, cells)
        for (r, c, fu, fv), dj in zip(cells, d):
            if np.isfinite(fu) and np.isfinite(fv):
                self.min_diag = min(self.min_diag, abs(fu - fv))
                self.min_edge = min(self.min_edge, fu, fv, 1.0 - fu, 1.0 - fv)
                if dj > 0:
                    self.kinds.add("lower" if fu >= fv else "upper")
        return f, d, J

    def step(self, P, D, q_des, v_des, tau_ff, f_ext=None):
        flat = sn.contact_forces
        sn.contact_forces = self._contact  # (sim_numpy.forward_dynamics looks the name up at call time)
        try:
            return super().step(P, D, q_des, v_des, tau_ff, f_ext)
        finally:
            sn.contact_forces = flat
