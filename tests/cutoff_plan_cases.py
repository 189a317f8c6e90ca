"""Clouds at which a stage of the device-side build of the cutoff plan (csrc/kmvp_cutoff_plan_device.hpp) can go wrong --
TEST INFRASTRUCTURE ONLY.  Shared by tests/test_host_cutoff_plan_device.py (the rules run serially on the host) and
tests/test_gpu_cutoff_plan_device.py (the kernels): each case is (name, y, x or None for targets = sources, R, factor) with
the coordinates rounded to the working precision and widened back to float64, which is what the context holds."""
import numpy as np

import cutoff_reference as cr


def _rnd(a, precision):
    return None if a is None else np.asarray(a, dtype=precision).astype(np.float64)


def boundary_cloud(D, precision):
    """A cloud whose extent is [0, 1] along every axis, with points at the working precision's neighbours of the cell
    boundaries lo + k h -- the value below, the nearest value and the value above, for several k along every axis -- next
    to random points: where floor((v - lo) / h) of the device and of the host must agree."""
    rs = np.random.RandomState(40 + D)
    R = 0.0625 * (1 + 2.0 ** -7)
    base = np.concatenate([rs.rand(1000 if D == 3 else 200, D), np.zeros((1, D)), np.ones((1, D))])   # (D = 3: 2 (N + M) >= 16^3 cells)
    h = R * (1.0 + 1.0 / 65536.0)
    rows = []
    for d in range(D):
        for k in (1, 2, 3, 5, 8, 11, 14):
            v = np.asarray(k * h, dtype=precision)
            for w in (np.nextafter(v, np.asarray(0, dtype=precision)), v, np.nextafter(v, np.asarray(2, dtype=precision))):
                p = rs.rand(D)
                p[d] = float(w)
                rows.append(p)
    y = _rnd(np.concatenate([base, np.array(rows)]), precision)
    p = cr.plan(y, y, R)
    assert p["h"] == h and np.all(p["lo"][:D] == 0) and np.all(p["g"][:D] == 16), "the cloud no longer probes the boundaries it was built for"
    return y, R


def cases(precision):
    out = []
    for name in cr.CLOUDS:
        y, x, R = cr.cloud(name, precision)
        for factor in (1.0, 1.5):
            out.append((f"cloud {name} x{factor}", y, x, R, factor))
    for D, R in ((1, 0.01), (2, 0.07), (3, 0.15)):
        rs = np.random.RandomState(10 * D)
        y, x = _rnd(rs.rand(900, D), precision), _rnd(rs.rand(333, D) * 1.2 - 0.1, precision)
        out.append((f"uniform D={D}", y, x, R, 1.0))
        out.append((f"uniform D={D} same", y, None, R, 1.5))
        yb, Rb = boundary_cloud(D, precision)
        out.append((f"boundaries D={D}", yb, None, Rb, 1.0))
        out.append((f"boundaries D={D} other targets", yb[::2], yb[1::2], Rb, 1.0))
    rs = np.random.RandomState(3)
    # rows of cells with exactly 64 and with 65 targets: the second coordinate picks the row
    y = rs.rand(400, 2)
    x = np.concatenate([np.stack([rs.rand(64), np.full(64, 0.30)], axis=1), np.stack([rs.rand(65), np.full(65, 0.62)], axis=1),
                        np.stack([rs.rand(7), np.full(7, 0.91)], axis=1)])
    out.append(("rows of 64 and 65", _rnd(y, precision), _rnd(x[rs.permutation(len(x))], precision), 0.2, 1.0))
    # more than a tile of identical points: ties in the caller's order cross a tile boundary
    base = rs.rand(60, 3)
    y = np.concatenate([base[:30], np.repeat(base[:1], 150, axis=0), base[30:]])
    out.append(("identical points", _rnd(y, precision), None, 0.3, 1.0))
    out.append(("identical targets", _rnd(base, precision), _rnd(y, precision), 0.3, 1.0))
    # 130 targets with a NaN or infinite coordinate: three loose tiles; non-finite sources
    y, x = rs.rand(300, 3), rs.rand(330, 3)
    bad = rs.permutation(330)[:130]
    x[bad, rs.randint(0, 3, 130)] = np.array([np.nan, np.inf, -np.inf])[rs.randint(0, 3, 130)]
    y[[3, 77, 150], [0, 2, 1]] = [np.nan, np.inf, -np.inf]
    out.append(("130 loose targets", _rnd(y, precision), _rnd(x, precision), 0.2, 1.0))
    z = y.copy()
    z[rs.permutation(300)[:70], 1] = np.nan
    out.append(("non-finite same points", _rnd(z, precision), None, 0.2, 1.0))
    out.append(("all sources non-finite", np.full((40, 3), np.nan), _rnd(rs.rand(90, 3), precision), 0.2, 1.0))
    out.append(("everything non-finite", np.full((70, 2), np.inf), None, 0.2, 1.0))
    pts = _rnd(rs.rand(130, 3), precision)
    out.append(("M = 0", np.zeros((0, 3)), pts, 0.2, 1.0))
    out.append(("N = 0", pts, np.zeros((0, 3)), 0.2, 1.0))
    out.append(("one cell", _rnd(rs.rand(100, 3), precision), _rnd(rs.rand(70, 3), precision), 2.0, 1.0))
    out.append(("cell cap", _rnd(rs.rand(50, 3), precision), None, 1e-9, 1.0))
    out.append(("cell cap D=1", _rnd(rs.rand(30, 1), precision), _rnd(rs.rand(20, 1), precision), 1e-9, 1.0))
    # clustered: most rows and cells are empty
    c = rs.rand(4, 3)
    y = np.concatenate([c[i] + 0.01 * rs.randn(120, 3) for i in range(4)])
    out.append(("clustered", _rnd(y, precision), _rnd(y[::3] + 0.005, precision), 0.03, 1.0))
    out.append(("one point", _rnd(rs.rand(1, 2), precision), None, 0.1, 1.0))
    return out


def equal_plans(got, want):
    """Entry for entry; lo compares with ==, so the sign of a zero may differ."""
    for key in ("n_pad", "m_pad", "m_alloc", "live_tiles", "walked", "h"):
        assert got[key] == want[key], (key, got[key], want[key])
    for key in ("g", "lo", "tiles", "runs", "tmap", "smap"):
        assert got[key].shape == want[key].shape and np.array_equal(got[key], want[key]), key
