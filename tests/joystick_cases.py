"""The scenarios the joystick tests share (tests/test_joystick_cpu.py builds csrc/joystick_profile.h for the host on them,
tests/test_gpu_joystick.py runs the kernel on them): per-robot tables, every robot's different, the ticks at which they are
compared, and the checker's outputs there (tests/joystick_numpy.py, stepped through EVERY tick from 0 as the reference's loop)."""
import numpy as np

import joystick_numpy as jn


def profile_tables(B, n_cols, seed, max_gap=40):
    """B pairs (k_switch, v_switch): robot 0 has n_cols columns, the others 2 .. n_cols (they get padded), k_switch starts at 0,
    some consecutive entries are equal, all six components are nonzero somewhere."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        n = n_cols if b == 0 or n_cols == 2 else int(rng.integers(2, n_cols + 1))
        gaps = rng.integers(1, max_gap + 1, size=n - 1)
        if n > 3:
            gaps[int(rng.integers(1, n - 1))] = 0  # (equal consecutive entries: never selected as a segment)
        ks = np.concatenate([[0], np.cumsum(gaps)])
        vs = rng.normal(size=(6, n)) * np.array([[0.5], [0.3], [0.05], [0.2], [0.2], [0.6]])
        vs[:, 0] = 0.0
        out.append((ks, vs))
    return out


def profile_ticks(tables, past=1000):
    """Every k_switch[i] - 1, k_switch[i], k_switch[i] + 1, the middle of every segment, 0, and `past` ticks past the end."""
    ticks = {0}
    for ks, _ in tables:
        ks = np.asarray(ks, dtype=np.int64)
        for i, k in enumerate(ks):
            ticks.update((int(k) - 1, int(k), int(k) + 1))
            if i:
                ticks.add(int(ks[i - 1] + ks[i]) // 2)
        ticks.add(int(ks[-1]) + past)
    return sorted(t for t in ticks if t >= 0)


def push_tables(B, n_max, seed):
    """B lists of up to n_max pushes; robot 1 has two that overlap, robot 2 none."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        n = 0 if b == 2 else (n_max if b == 0 else int(rng.integers(1, n_max + 1)))
        entries = []
        for e in range(n):
            start, dur = int(rng.integers(0, 60)), int(rng.integers(1, 50))
            entries.append((start, dur, rng.normal(size=3) * 4.0, rng.normal(size=3) * 0.5))
        if b == 1:
            entries = [(10, 20, np.array([0.0, 3.0, -1.0]), np.array([0.1, 0.0, 0.2])),
                       (18, 31, np.array([2.0, -3.0, 0.5]), np.array([0.0, -0.3, 0.0]))][:max(n_max, 1)]
        out.append(entries[:n_max])
    return out


def push_ticks(pushes):
    ticks = {0}
    for entries in pushes:
        for start, dur, _, _ in entries:
            ticks.update((start - 1, start, start + dur // 2, start + dur, start + dur + 1))
    return sorted(t for t in ticks if t >= 0)


def code_tables(B, n_max, seed):
    """B lists of (tick, code); robot 0 has n_max pairs with a tie on one tick (the later pair must win), robot 2 none."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        n = 0 if b == 2 else (n_max if b == 0 else int(rng.integers(1, n_max + 1)))
        pairs = [(int(rng.integers(0, 80)), int(rng.integers(1, 6))) for _ in range(n)]
        if b == 0 and n >= 2:
            pairs[0], pairs[-1] = (20, 2), (20, 4)
        out.append(pairs)
    return out


def code_ticks(codes):
    ticks = {0}
    for pairs in codes:
        for k, _ in pairs:
            ticks.update((k - 1, k, k + 1))
    return sorted(t for t in ticks if t >= 0)


def ramp_speeds(B, seed):
    """(B,3): speeds whose beta hits the floor of 100 (|V| 10000 <= 100), speeds above it, negative ones, zeros."""
    rng = np.random.default_rng(seed)
    V = rng.uniform(-1.0, 1.0, size=(B, 3)) * np.array([1.2, 0.6, 0.9])
    V[0] = [0.005, -0.01, 0.03]      # beta: 100 (floor), 100 (exactly), 100 (75 -> floor)
    V[1] = [0.0, 0.0, 0.0]
    V[2] = [-0.3, 0.01001, -0.0401]  # 3000, 100 (100.1 truncated), 100 (100.25 truncated)
    return V


def ramp_ticks(V, k_start):
    ticks = {0, max(k_start - 1, 0), k_start, k_start + 1, k_start + 50, k_start + 99, k_start + 100, k_start + 101}
    for v, scale in zip(np.abs(V).T, (10000, 10000, 2500)):
        for x in v:
            beta = int(max(x * scale, 100.0))
            ticks.update((k_start + beta // 2, k_start + beta - 1, k_start + beta, k_start + beta + 1))
    ticks.add(k_start + 20000)
    return sorted(ticks)


def gamepad_commands(B, T, seed, alpha=0.0020 / 0.02):
    """(T,B,6) step and sign-changing commands; robots 0..3 approach the four dead-band neighbours from a filter state of zero."""
    rng = np.random.default_rng(seed)
    g = np.zeros((T, B, 6))
    level = rng.uniform(-1.0, 1.0, size=(B, 6))
    for t in range(T):
        if t % 37 == 0:
            level = rng.uniform(-1.0, 1.0, size=(B, 6)) * (rng.random((B, 6)) > 0.2)
        if t % 90 == 45:
            level = -level
        g[t] = level
    for b, target in enumerate(DEADBAND_NEIGHBOURS):
        g[0, b, 0] = command_for(target, alpha)
    return g


# 0.005 and -0.005 survive the strict comparisons, their neighbours one ulp inside are zeroed
DEADBAND_NEIGHBOURS = (0.005, -0.005, float(np.nextafter(0.005, 0.0)), float(np.nextafter(-0.005, 0.0)))


def command_for(target, alpha):
    """The command that takes a filter at rest (v_ref = 0) to exactly `target`: alpha g + (1 - alpha) 0 == target."""
    g = target / alpha
    for _ in range(64):
        p = alpha * g + (1 - alpha) * 0.0
        if p == target:
            return float(g)
        g = np.nextafter(g, np.inf if p < target else -np.inf)
    raise AssertionError("no command gives %r" % target)


def robots(B, profiles=None, ramp=None, k_start=0, gamepad=None, codes=None, pushes=None):
    """The checker's objects for a fleet (one per robot)."""
    out = []
    for b in range(B):
        kw = dict(codes=codes[b] if codes else (), pushes=pushes[b] if pushes else ())
        if profiles is not None:
            out.append(jn.JoystickNumpy(k_switch=profiles[b][0], v_switch=profiles[b][1], **kw))
        elif ramp is not None:
            out.append(jn.JoystickNumpy(ramp=ramp[b], k_start=k_start, **kw))
        else:
            out.append(jn.JoystickNumpy(gamepad=True, **(gamepad or {}), **kw))
    return out


def expected(fleet, ticks, every_tick=True):
    """The checker's v_ref, code, f_ext (len(ticks),B,..) at `ticks`, the fleet stepped through every tick from 0 to the last one
    (every_tick=False: only through `ticks`, which must then hold k_switch[-1] - 1 of every profile: the hold's source)."""
    ticks = list(ticks)
    if not every_tick:
        return jn.run(fleet, ticks)
    allt = list(range(ticks[-1] + 1))
    v, c, f = jn.run(fleet, allt)
    return v[ticks], c[ticks], f[ticks]
