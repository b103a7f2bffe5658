"""Generates tests/golden/geometry_cases.npz: the named case table of tests/test_device_geometry.py and the small graphs
of its optimize / KLD / new-edge tests, with the float64-rounded outputs of the multiprecision reference
tests/geom_ref.py (needs mpmath; the GPU tests read only the file).
    python tests/golden/make_geometry_cases.py

Every input is built in multiprecision from a SplitMix64 stream seeded by the case's name and rounded to float64 once, so
the file is reproducible bit for bit (tests/test_device_geometry.py::test_fixture_is_what_the_reference_generates); the
reference then starts from the rounded inputs."""
import os
import sys
import zlib

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import geom_ref as gr   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "geometry_cases.npz")
_M = (1 << 64) - 1


class Rng:
    """SplitMix64 -> uniform numbers in [-1, 1), as multiprecision values (no platform arithmetic involved)"""

    def __init__(self, name):
        self.s = zlib.crc32(name.encode()) * 0x9E3779B97F4A7C15 & _M

    def u(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M
        x = self.s
        x ^= x >> 30
        x = x * 0xBF58476D1CE4E5B9 & _M
        x ^= x >> 27
        x = x * 0x94D049BB133111EB & _M
        x ^= x >> 31
        return mp.mpf(x >> 11) / (1 << 52) - 1

    def vec(self, n, scale=1):
        return [scale * self.u() for _ in range(n)]

    def axis(self):
        while True:
            a = self.vec(3)
            if sum(c * c for c in a) > mp.mpf("0.05"):
                return a

    def near(self, k, spread="0.05"):
        a = self.vec(3, mp.mpf(spread))
        a[k] += 1
        return a

    def pose(self, tscale=3):
        return self.vec(3, tscale), gr.qunit(self.vec(4))

    def spd(self, d, block_diagonal=False):
        """Q diag(1 .. 1e3, geometric) Q^T with Q a product of three Householder reflections: condition 1e3, no structure.
        block_diagonal: two independent 3 x 3 blocks of that kind (no translation-rotation coupling)."""
        if block_diagonal:
            a, b = self.spd(3), self.spd(3)
            z = mp.mpf(0)
            return [a[i] + [z] * 3 for i in range(3)] + [[z] * 3 + b[i] for i in range(3)]
        Q = [[mp.mpf(int(i == j)) for j in range(d)] for i in range(d)]
        for _ in range(3):
            v = self.vec(d)
            vv = sum(c * c for c in v)
            Q = [[Q[i][j] - 2 * v[j] * sum(Q[i][k] * v[k] for k in range(d)) / vv for j in range(d)] for i in range(d)]
        lam = [mp.mpf(10) ** (mp.mpf(3 * k) / (d - 1)) for k in range(d)]
        return [[sum(Q[i][k] * lam[k] * Q[j][k] for k in range(d)) for j in range(d)] for i in range(d)]


def f64(x):
    return np.array(gr.to_float(x), np.float64)


def tq(X):
    """(t, q) -> 7 float64"""
    return f64(list(X[0]) + list(X[1]))


def upper(om):
    d = len(om)
    return f64([om[i][j] for i in range(d) for j in range(i, d)])


def rot(axis, deg):
    return gr.axis_angle(axis, deg)


ZERO3 = [mp.mpf(0)] * 3
EX, EY, EZ = [1, 0, 0], [0, 1, 0], [0, 0, 1]


# ------------------------------------------------------------------------------------------ the SE3 table
def se3_table():
    """name -> dict(E=(t_E, q_E) wanted error | zero=relative rotation, lever=bool, exact=bool, negate=...)"""
    T = []

    def add(name, axis, deg, **kw):
        T.append((name, axis, deg, kw))

    gen = lambda n: Rng("axis:" + n).axis()          # noqa: E731
    near = lambda n, k, spread="0.05": Rng("axis:" + n).near(k, spread)     # noqa: E731
    # the four extraction branches
    for k, ax in enumerate("xyz"):
        add(f"branch_150_near_{ax}", near(f"b150{ax}", k), 150)
        add(f"branch_165_near_{ax}", near(f"b165{ax}", k, "0.3"), 165)
    for n in range(3):
        add(f"branch_150_generic_{n}", gen(f"g150{n}"), 150)
    for n in range(2):
        add(f"branch_30_generic_{n}", gen(f"g30{n}"), 30)
    add("branch_100_generic", gen("g100"), 100)
    # borders: tr(E) = 1 + 2 cos(angle) = +-1e-3, +-1e-9
    for tag, tau in (("p1e-3", "1e-3"), ("m1e-3", "-1e-3"), ("p1e-9", "1e-9"), ("m1e-9", "-1e-9")):
        ang = mp.acos((mp.mpf(tau) - 1) / 2) * 180 / mp.pi
        for k, ax in enumerate("xyz"):
            add(f"border_tr_{tag}_near_{ax}", near(f"tr{tag}{ax}", k, "0.3"), ang)
    # borders: two diagonal entries of E equal -> R_to_quat and dq_dR may extract through different components
    for n, ax in (("xy", [1, 1, 0]), ("yz", [0, 1, 1]), ("zx", [1, 0, 1])):
        add(f"border_diag_170_{n}", ax, 170)
        add(f"border_diag_190_{n}", ax, 190)
    # sign: w < 0 before normalisation
    for k, ax in enumerate("xyz"):
        add(f"sign_200_near_{ax}", near(f"s200{ax}", k), 200)
    add("sign_200_generic", gen("s200g"), 200)
    add("sign_270_generic", gen("s270g"), 270)
    add("sign_340_generic", gen("s340g"), 340)
    add("sign_240_near_y", near("s240y", 1, "0.3"), 240)
    # exact half-turns: qw == 0 (sign-invariant outputs only, Omega without translation-rotation coupling)
    for n, ax in (("x", EX), ("y", EY), ("z", EZ), ("111", [1, 1, 1])):
        add(f"halfturn_{n}", ax, 180, exact=True)
    # zero error at a large relative rotation (the new-edge case: Z = between(Xi, Xj))
    for k, ax in enumerate("xyz"):
        add(f"zero_error_rel_150_near_{ax}", near(f"z150{ax}", k), 150, zero=True)
    add("zero_error_rel_30_generic", gen("z30"), 30, zero=True)
    add("zero_error_rel_200_generic", gen("z200"), 200, zero=True)
    # lever arm: translations of order 1e3
    for k, ax in enumerate("xyz"):
        add(f"lever_150_near_{ax}", near(f"l150{ax}", k), 150, lever=True)
    return T


def build_se3_case(name, axis, deg, exact=False, zero=False, lever=False):
    r = Rng(name)
    tscale = 1000 if lever else 3
    if exact:
        # identity orientations of Xi and Z: E's rotation is Xj's, bit for bit, on every implementation
        ident = [mp.mpf(0)] * 3 + [mp.mpf(1)]
        Xi = (r.vec(3, 3), ident)
        a = gr.vec(axis)
        n = mp.sqrt(sum(c * c for c in a))
        Xj = (r.vec(3, 3), [a[0] / n, a[1] / n, a[2] / n, mp.mpf(0)])
        Z = (r.vec(3, 3), ident)
    elif zero:
        Xi = r.pose(tscale)
        Xj = gr.se3_mul(Xi, (r.vec(3, 2), rot(axis, deg)))
        Z = None
    else:
        Xi, Xj = r.pose(tscale), r.pose(tscale)
        E = (r.vec(3, 1), rot(axis, deg))
        Z = gr.se3_mul(gr.se3_mul(gr.se3_inv(Xi), Xj), gr.se3_inv(E))
        if r.u() < 0:
            Xj = (Xj[0], [-c for c in Xj[1]])          # stored quaternions of either sign
        if r.u() < 0:
            Z = (Z[0], [-c for c in Z[1]])
    xi, xj = tq(Xi), tq(Xj)
    if zero:
        z = f64(gr.se3_between(gr.se3(xi), gr.se3(xj)))
    else:
        z = tq(Z)
    om = upper(r.spd(6, block_diagonal=exact))
    # the chain a - i - j: a plain edge a - i with a small error
    Xa = r.pose(tscale)
    xa = tq(Xa)
    Zai = gr.se3_mul(gr.se3_mul(gr.se3_inv(gr.se3(xa)), gr.se3(xi)), (r.vec(3, mp.mpf("0.1")), rot(r.axis(), 10)))
    zai = tq((Zai[0], gr._canonical(Zai[1])))
    om_ai = upper(r.spd(6))
    return xi, xj, z, om, xa, zai, om_ai


def reference_of_case(d, xi, xj, z, om, xa, zai, om_ai):
    P = {0: gr.pose(d, xa), 1: gr.pose(d, xi), 2: gr.pose(d, xj)}
    Z, Zai = gr.pose(d, z), gr.pose(d, zai)
    O, Oai = gr.omega(d, om), gr.omega(d, om_ai)
    err, Ji, Jj = gr.edge_terms(d, P[1], P[2], Z)
    chi2 = sum(err[a] * O[a][b] * err[b] for a in range(d) for b in range(d))
    chi2_chain, H = gr.chi2_and_information(d, P, [(0, 1, Zai, Oai), (1, 2, Z, O)])
    out = dict(err=f64(err), Ji=f64(Ji), Jj=f64(Jj), chi2=float(chi2), H=f64(H), between=f64(gr.between(d, P[1], P[2])))
    if d == 6:
        out["qw"] = float(gr.se3_error_full(P[1], P[2], Z)[1][3])
    return out


# ------------------------------------------------------------------------------------------ the SE2 table
def se2_table():
    pi = mp.mpf(np.pi)      # the fp64 constant
    eps = mp.mpf("1e-12")
    h = mp.mpf("0.5")
    # name, theta_i, theta_j, z_theta
    return [
        ("dtheta_plus_pi_minus_1e-12", h, h + pi - eps, mp.mpf("0.3")),
        ("dtheta_minus_pi_plus_1e-12", h, h - pi + eps, mp.mpf("-0.2")),
        ("dtheta_exactly_pi", mp.mpf(0), pi, mp.mpf("0.25")),
        ("dtheta_exactly_pi_halves", -pi / 2, pi / 2, mp.mpf("-0.4")),
        ("dtheta_exactly_minus_pi", pi, mp.mpf(0), mp.mpf("0.25")),
        ("stored_theta_7.5_and_-40", mp.mpf("7.5"), mp.mpf("-40.0"), mp.mpf("1.0")),
        ("stored_theta_-40_and_7.5", mp.mpf("-40.0"), mp.mpf("7.5"), mp.mpf("-2.0")),
        ("wraps_at_second_normalize", mp.mpf("0.125"), mp.mpf("3.125"), mp.mpf("-1.0")),
        ("wraps_at_second_normalize_negative", mp.mpf("3.0"), mp.mpf("0.0"), mp.mpf("1.0")),
        ("error_exactly_pi_at_second_normalize", mp.mpf(0), pi / 2, -pi / 2),
        ("wraps_at_first_normalize_only", mp.mpf("3.1"), mp.mpf("-3.1"), mp.mpf("0.05")),
        ("no_wrap", mp.mpf("0.7"), mp.mpf("1.9"), mp.mpf("1.0")),
    ]


def build_se2_case(name, thi, thj, zth):
    r = Rng(name)
    xi = f64(r.vec(2, 5) + [thi])
    xj = f64(r.vec(2, 5) + [thj])
    zt = gr.se2_between(gr.se2(xi), gr.se2(xj))
    e = r.vec(2, mp.mpf("0.3"))
    z = f64([zt[0] - e[0], zt[1] - e[1], zth])
    om = upper(r.spd(3))
    xa = f64(r.vec(2, 5) + [3 * r.u()])
    b = gr.se2_between(gr.se2(xa), gr.se2(xi))
    zai = f64([b[0] + r.u() / 10, b[1] + r.u() / 10, b[2] + r.u() / 20])
    om_ai = upper(r.spd(3))
    return xi, xj, z, om, xa, zai, om_ai


# ------------------------------------------------------------------------------------------ small graphs
def ring_graph(d, name, n, chords, orient):
    """Noise-free graph: vertices on a circle, ring edges plus chords, measurements = reference between of the rounded poses."""
    r = Rng(name)
    poses = []
    for i in range(n):
        a = 2 * mp.pi * i / n
        if d == 6:
            poses.append(tq(([5 * mp.cos(a), 5 * mp.sin(a), r.u()], gr._canonical(orient[i]))))
        else:
            poses.append(f64([5 * mp.cos(a), 5 * mp.sin(a), orient[i]]))
    poses = np.array(poses)
    ij = [(i, (i + 1) % n) for i in range(n)] + list(chords)
    data = []
    for a, b in ij:
        z = f64(gr.between(d, gr.pose(d, poses[a]), gr.pose(d, poses[b])))
        data.append(np.concatenate([z, upper(r.spd(d))]))
    return poses, np.array(ij, np.int32), np.array(data)


def displaced(d, poses, name, rad, dist, skip=(0,)):
    """Every vertex but `skip` moved by a rotation of `rad` about a random axis and a translation of length `dist` (X * delta)."""
    r = Rng(name)
    out = poses.copy()
    for i in range(len(poses)):
        if i in skip:
            continue
        if d == 6:
            t = r.axis()
            n = mp.sqrt(sum(c * c for c in t))
            dl = ([dist * c / n for c in t], rot(r.axis(), rad * 180 / mp.pi))
            X = gr.se3_mul(gr.se3(poses[i]), dl)
            out[i] = tq((X[0], gr._canonical(X[1])))
        else:
            a = mp.pi * r.u()
            sgn = 1 if r.u() < 0 else -1
            out[i] = f64([poses[i][0] + dist * mp.cos(a), poses[i][1] + dist * mp.sin(a), mp.mpf(float(poses[i][2])) + sgn * rad])
    return out


def turned(poses, v, axis, deg=150):
    out = poses.copy()
    X = gr.se3_mul(gr.se3(poses[v]), (ZERO3, rot(axis, deg)))
    out[v] = tq((X[0], gr._canonical(X[1])))
    return out


def generate():
    out = {}
    # ---- SE3 table
    names, rows, refs = [], [], []
    for name, axis, deg, kw in se3_table():
        c = build_se3_case(name, axis, deg, **kw)
        names.append(name)
        rows.append(c)
        refs.append(reference_of_case(6, *c))
    out["se3_names"] = np.array(names)
    for k, key in enumerate(("xi", "xj", "z", "omega", "xa", "z_ai", "omega_ai")):
        out["se3_" + key] = np.array([c[k] for c in rows])
    for key in ("err", "Ji", "Jj", "chi2", "H", "between", "qw"):
        out["se3_ref_" + key] = np.array([r[key] for r in refs])
    # ---- SE2 table
    names, rows, refs = [], [], []
    for name, thi, thj, zth in se2_table():
        c = build_se2_case(name, thi, thj, zth)
        names.append(name)
        rows.append(c)
        refs.append(reference_of_case(3, *c))
    out["se2_names"] = np.array(names)
    for k, key in enumerate(("xi", "xj", "z", "omega", "xa", "z_ai", "omega_ai")):
        out["se2_" + key] = np.array([c[k] for c in rows])
    for key in ("err", "Ji", "Jj", "chi2", "H", "between"):
        out["se2_ref_" + key] = np.array([r[key] for r in refs])
    # ---- SE3 ring of 8 with two chords: absolute orientations in every extraction branch, both signs
    g = lambda n: Rng("ring8:" + n)    # noqa: E731
    orient = [rot(g("0").axis(), 20), rot(g("1").near(0), 150), rot(g("2").near(1), 150), rot(g("3").near(2), 150),
              rot(g("4").near(0), 200), rot(g("5").axis(), 120), rot([1, 1, 0], 170), rot(g("7").near(2), 210)]
    P, ij, data = ring_graph(6, "ring8", 8, [(0, 4), (2, 6)], orient)
    out["ring3_truth"], out["ring3_ij"], out["ring3_data"] = P, ij, data
    out["ring3_start"] = displaced(6, P, "ring8:start", mp.mpf("0.3"), mp.mpf("0.2"))
    out["ring3_turned"] = np.array([turned(P, 3, ax) for ax in (EX, EY, EZ)])
    # ---- SE2 twin: headings on both sides of +-pi
    th = [mp.mpf(s) for s in ("0.3", "3.1", "-3.1", "3.0", "-2.9", "3.14", "-3.14", "2.7")]
    P, ij, data = ring_graph(3, "ring8se2", 8, [(0, 4), (2, 6)], th)
    out["ring2_truth"], out["ring2_ij"], out["ring2_data"] = P, ij, data
    out["ring2_start"] = displaced(3, P, "ring8se2:start", mp.mpf("0.3"), mp.mpf("0.2"))
    # ---- KLD: 6 vertices, `other` displaced by branch-spanning rotations; reference estimate difference
    g = lambda n: Rng("kld6:" + n)    # noqa: E731
    orient = [rot(g(str(i)).axis(), a) for i, a in enumerate((10, 70, 130, 160, 220, 300))]
    P, ij, data = ring_graph(6, "kld6", 6, [(0, 3)], orient)
    moves = [None, (g("m1").axis(), 30), (g("m2").near(0), 150), (g("m3").near(1), 150), (g("m4").near(2), 150), (g("m5").near(0), 200)]
    Po = P.copy()
    for i in range(1, 6):
        X = gr.se3_mul(gr.se3(P[i]), (g(f"t{i}").vec(3, mp.mpf("0.5")), rot(*moves[i])))
        Po[i] = tq((X[0], gr._canonical(X[1])))
    out["kld_base"], out["kld_other"], out["kld_ij"], out["kld_data"] = P, Po, ij, data
    out["kld_ref_diff"] = np.array([f64(gr.se3_diff(gr.se3(P[i]), gr.se3(Po[i]))) for i in range(1, 6)])
    # ---- star: a root and 4 neighbours whose relative rotations lie in every branch; reference between of every ordered pair
    g = lambda n: Rng("star5:" + n)    # noqa: E731
    q = [rot(g("0").axis(), 25)]
    for step in ((g("1").axis(), 40), (g("2").near(0), 150), (g("3").near(1), 150), (g("4").near(2), 150)):
        q.append(gr.qmul(q[-1], rot(*step)))
    P = np.array([tq((g(f"p{i}").vec(3, 4), gr._canonical(q[i]))) for i in range(5)])
    out["star_poses"] = P
    out["star_ref_between"] = np.array([[f64(gr.se3_between(gr.se3(P[a]), gr.se3(P[b]))) for b in range(5)] for a in range(5)])
    out["star_omega"] = np.array([upper(g(f"o{e}").spd(6)) for e in range(7)])
    return out


if __name__ == "__main__":
    out = generate()
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out['se3_names'])} SE3 + {len(out['se2_names'])} SE2 cases, {os.path.getsize(OUT)} bytes")
