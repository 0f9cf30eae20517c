"""Independent fp64 equations of motion for the collapsed T1 articulation (TEST INFRASTRUCTURE).

PhysX (the reference's physics) cannot run anywhere here, so the HIP dynamics is pinned against physics
itself: this module derives the floating-base equations of motion with a formulation that shares nothing
with the product's CRBA/RNEA/LTDL code -- Kane's projected Newton-Euler equations

    sum_b  Jv_b^T (m_b a_b - m_b g) + Jw_b^T (I_b alpha_b + w_b x I_b w_b) = [0, 0, tau]

with partial-velocity Jacobians Jv_b, Jw_b of every body's COM velocity / angular velocity w.r.t. the
generalized speeds u = [omega_base (world), v_base_origin (world), qd], obtained by central finite
differences of plain homogeneous-transform forward kinematics, and the velocity-product terms J_dot u by
differentiating J along the motion.  Armature adds to the joint diagonal (PhysX joint-space armature).
"""
import numpy as np


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    x, y, z = axis
    C = 1 - c
    return np.array([[c + x * x * C, x * y * C - z * s, x * z * C + y * s],
                     [y * x * C + z * s, c + y * y * C, y * z * C - x * s],
                     [z * x * C - y * s, z * y * C + x * s, c + z * z * C]])


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    """(x, y, z, w) of a rotation matrix (Shepperd: the branch with the largest of w^2, x^2, y^2, z^2)"""
    t = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2],
                  R[2, 2] - R[0, 0] - R[1, 1]])
    i = int(np.argmax(t))
    s = 2.0 * np.sqrt(1.0 + t[i])
    if i == 0:
        out = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif i == 1:
        out = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif i == 2:
        out = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        out = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    return np.array(out)


class Robot:
    def __init__(self, tab, mass=None, inertia_scale=None, com_disp=(0, 0, 0), armature=None):
        self.parent = tab["parent"]
        self.off = np.array(tab["joint_offset"])
        self.axis = np.array(tab["joint_axis"], dtype=float)
        self.mass = np.array(tab["mass"] if mass is None else mass, dtype=float)
        self.com = np.array(tab["com"], dtype=float)
        self.com[0] += np.asarray(com_disp, float)
        sc = np.ones(13) if inertia_scale is None else np.asarray(inertia_scale, float)
        self.I = []
        for b, (xx, yy, zz, xy, xz, yz) in enumerate(tab["inertia"]):
            self.I.append(sc[b] * np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]]))
        self.arm = np.zeros(12) if armature is None else np.asarray(armature, float)

    def fk(self, p, R, q):
        Rs, ps = [R], [p]
        for b in range(1, 13):
            pr = self.parent[b]
            ps.append(ps[pr] + Rs[pr] @ self.off[b])
            Rs.append(Rs[pr] @ _rot(self.axis[b], q[b - 1]))
        coms = [ps[b] + Rs[b] @ self.com[b] for b in range(13)]
        return Rs, ps, coms

    @staticmethod
    def _move(p, R, q, u, eps):
        """configuration after moving for time eps with generalized speeds u (first order in eps)."""
        w, v, qd = u[0:3], u[3:6], u[6:18]
        n = np.linalg.norm(w)
        Rw = _rot(w / n, n * eps) if n > 0 else np.eye(3)
        return p + eps * v, Rw @ R, q + eps * qd

    def jacobians(self, p, R, q, eps=1e-6):
        Jv = np.zeros((13, 3, 18))
        Jw = np.zeros((13, 3, 18))
        for k in range(18):
            e = np.zeros(18)
            e[k] = 1.0
            Rp, _, cp = self.fk(*self._move(p, R, q, e, eps))
            Rm, _, cm = self.fk(*self._move(p, R, q, e, -eps))
            for b in range(13):
                Jv[b, :, k] = (cp[b] - cm[b]) / (2 * eps)
                W = (Rp[b] - Rm[b]) @ Rp[b].T / (2 * eps)   # skew(w) to first order
                Jw[b, :, k] = [W[2, 1], W[0, 2], W[1, 0]]
        return Jv, Jw

    def accel(self, p, quat, w, v, q, qd, tau, g=9.81, eps=1e-5, f_base=None):
        """generalized accelerations; f_base: an external world-frame force on the base body at its COM (Isaac Gym
        apply_rigid_body_force_tensors without positions), entering as Jv_base^T f."""
        R = quat_to_R(quat)
        u = np.concatenate([w, v, qd])
        Jv, Jw = self.jacobians(p, R, q)
        Jvp, Jwp = self.jacobians(*self._move(p, R, q, u, eps))
        Jvm, Jwm = self.jacobians(*self._move(p, R, q, u, -eps))
        Rs, _, _ = self.fk(p, R, q)
        M = np.zeros((18, 18))
        h = np.zeros(18)
        grav = np.array([0, 0, -g])
        for b in range(13):
            Ib = Rs[b] @ self.I[b] @ Rs[b].T
            wb = Jw[b] @ u
            Jvd_u = (Jvp[b] - Jvm[b]) @ u / (2 * eps)
            Jwd_u = (Jwp[b] - Jwm[b]) @ u / (2 * eps)
            M += self.mass[b] * Jv[b].T @ Jv[b] + Jw[b].T @ Ib @ Jw[b]
            h += Jv[b].T @ (self.mass[b] * (Jvd_u - grav)) + Jw[b].T @ (Ib @ Jwd_u + np.cross(wb, Ib @ wb))
        M[6:, 6:] += np.diag(self.arm)
        f = np.concatenate([np.zeros(6), tau])
        if f_base is not None:
            f = f + Jv[0].T @ np.asarray(f_base, float)
        return np.linalg.solve(M, f - h), M


# ---------------------------------------------------------------------------------------------------------------
# One implicit substep WITH contact, written independently of the product's assembly (TEST INFRASTRUCTURE).
#
# The product (t1_dynamics.h) folds its contact and joint-limit terms into a tree-sparse LTDL; this restates the
# same discrete law densely from plain kinematics:
#   * point Jacobians J_x (velocity of a body-fixed point w.r.t. u = [omega, v_O, qd]) by central differences of
#     forward kinematics -- no spatial algebra shared with the product;
#   * terrain: the plane z = 0 (normal +z), contact candidates = the model's contact points below it; or, with a
#     MeshTerrain, the triangle mesh of a height field: a point is in contact when it is below the triangle over / under
#     it (h - z > 0), the depth is (h - z) n_z along that triangle's unit normal n;
#   * self-collision: the legs' capsules (utils/urdf.py self_capsules: left shank, left foot, right shank, right foot);
#     per overlapping pair one contact at the middle of the overlap along the segments' closest points (found here by
#     enumerating the 2-parameter problem's interior stationary point and its four edges; near-parallel segments,
#     sin^2 < 1e-3, by the overlap-midpoint rule the product documents); pairs {l, r} x {shank, foot} across the legs
#     and shank-foot within a leg; each body gets the force at that point, the other body the reaction;
#   * the law per contact: normal spring k pen, damper d while approaching (implicit: cn = dt k + d) and,
#     with a restitution target v_tgt, while separating slower than it (cn = d, f_n += d v_tgt), regularised Coulomb friction ct = mu fn_est / max(|v_t|, v_s) as an implicit tangential
#     damper: C = cn n n^T + ct (I - n n^T), f = (k pen - cn v_n + d v_tgt) n - ct v_t;
#   * restitution: each terrain-contact body (shanks, feet, the base box's two halves) keeps the approach speed v_imp
#     of its contact episode; v_tgt = e v_imp above the bounce threshold, else 0 (self-contacts: 0);
#   * soft joint limits k_l, d_l (implicit damper when moving further out);
#   * implicit Euler in the contact / limit velocities with each body's own terms implicit (a self-contact's other
#     body enters through its current velocity):
#       (M + dt sum J^T C J + dt diag(c_l)) du = dt (tau - h + sum J^T f + f_limit).
# ---------------------------------------------------------------------------------------------------------------
SELF_BODIES = (4, 6, 10, 12)


def _capsules(tab):
    """{body: (a, b, r)}: each self-collision box (tab["self_box"], link frame) as the capsule along its longest axis,
    radius the smaller cross-section half extent, ends inset by the radius (the model's definition)"""
    out = {}
    for body, box in zip(SELF_BODIES, tab["self_box"]):
        c, h = np.asarray(box[:3], float), np.asarray(box[3:], float)
        ax = int(np.argmax(h))
        r = float(np.min(np.delete(h, ax)))
        e = np.eye(3)[ax] * max(h[ax] - r, 1e-3)
        out[body] = (c - e, c + e, r)
    return out


def _closest_segments(p1, q1, p2, q2):
    """closest points of the segments p1-q1, p2-q2: min over the interior stationary point (if inside [0,1]^2) and the
    best point of each edge of the parameter square; near-parallel segments: the overlap-midpoint rule"""
    d1, d2 = q1 - p1, q2 - p2
    a, e, b = d1 @ d1, d2 @ d2, d1 @ d2
    clip = lambda x: min(max(x, 0.0), 1.0)  # noqa: E731
    if a * e - b * b < 1e-3 * a * e:
        s0, s1 = sorted(((p2 - p1) @ d1 / a, (q2 - p1) @ d1 / a))
        c1 = p1 + 0.5 * (clip(s0) + clip(s1)) * d1
        return c1, p2 + clip((c1 - p2) @ d2 / e) * d2
    cands = []
    st = np.linalg.solve(np.array([[a, -b], [-b, e]]), np.array([-(p1 - p2) @ d1, (p1 - p2) @ d2]))
    if 0 <= st[0] <= 1 and 0 <= st[1] <= 1:
        cands.append(tuple(st))
    for sv in (0.0, 1.0):
        cands.append((sv, clip((p1 + sv * d1 - p2) @ d2 / e)))
    for tv in (0.0, 1.0):
        cands.append((clip((p2 + tv * d2 - p1) @ d1 / a), tv))
    dist = [np.linalg.norm(p1 + sv * d1 - p2 - tv * d2) for sv, tv in cands]
    sv, tv = cands[int(np.argmin(dist))]
    return p1 + sv * d1, p2 + tv * d2


class MeshTerrain:
    """A height field as the explicit triangle mesh the reference's trimesh construction makes of it (without its
    slope-threshold correction, which the product leaves out too): vertex (i, j) at (i hs - border, j hs - border,
    vs h[i, j]), rows along x, and per cell the two triangles on either side of the diagonal (i, j)-(i+1, j+1).

    Queries work on the mesh alone: the triangle containing (x, y) by a 2-D barycentric test over all triangles, the
    height by barycentric interpolation of its vertices, the normal from the cross product of its edges."""

    def __init__(self, heights, hs, vs, border):
        h = np.asarray(heights)
        rows, cols = h.shape
        ii, jj = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        self.vertices = np.stack([ii * float(hs) - float(border), jj * float(hs) - float(border),
                                  float(vs) * h.astype(np.float64)], -1).reshape(-1, 3)
        tris, half = [], []
        for i in range(rows - 1):
            for j in range(cols - 1):
                v00, v01, v10, v11 = i * cols + j, i * cols + j + 1, (i + 1) * cols + j, (i + 1) * cols + j + 1
                tris += [(v00, v11, v01), (v00, v10, v11)]
                half += [0, 1]          # 0: the triangle with the cell's (i, j+1) corner, 1: the one with (i+1, j)
        self.triangles = np.array(tris)
        self.half = np.array(half)
        a, b, c = (self.vertices[self.triangles[:, k]] for k in range(3))
        self._a, self._ab, self._ac = a, b - a, c - a
        self._det = self._ab[:, 0] * self._ac[:, 1] - self._ab[:, 1] * self._ac[:, 0]
        n = np.cross(self._ab, self._ac)
        n *= np.sign(n[:, 2:3])                                      # upward
        self.normals = n / np.linalg.norm(n, axis=1, keepdims=True)

    def query(self, x, y):
        """(height, unit normal, barycentric margin, half) of the triangle over / under (x, y); the margin is the
        smallest barycentric coordinate (0 on an edge of the triangle)"""
        dx, dy = x - self._a[:, 0], y - self._a[:, 1]
        l1 = (dx * self._ac[:, 1] - dy * self._ac[:, 0]) / self._det
        l2 = (dy * self._ab[:, 0] - dx * self._ab[:, 1]) / self._det
        l0 = 1.0 - l1 - l2
        margin = np.minimum(l0, np.minimum(l1, l2))
        t = int(np.argmax(margin))
        if margin[t] < 0:
            raise ValueError(f"({x}, {y}) is outside the height field")
        h = self._a[t, 2] + l1[t] * self._ab[t, 2] + l2[t] * self._ac[t, 2]
        return float(h), self.normals[t].copy(), float(margin[t]), int(self.half[t])


class ContactRobot(Robot):
    def __init__(self, tab, mass=None, inertia_scale=None, com_disp=(0, 0, 0), armature=None, solver=None,
                 limits=None, terrain=None):
        super().__init__(tab, mass, inertia_scale, com_disp, armature)
        self.tab = tab
        self.terrain = terrain               # a MeshTerrain, or None: the plane z = 0
        self.sv = dict(solver)
        lim = np.asarray(tab["limits"], float) if limits is None else np.asarray(limits, float)
        self.lo, self.hi = lim[:, 0], lim[:, 1]

    def _points(self, Rs, ps, b, local):
        return ps[b] + Rs[b] @ local

    def point_jacobian(self, p, R, q, b, local, eps=1e-6):
        """d x / d u of the body-fixed point `local` of body b (world position x)"""
        J = np.zeros((3, 18))
        for k in range(18):
            e = np.zeros(18)
            e[k] = 1.0
            Rp, pp, _ = self.fk(*self._move(p, R, q, e, eps))
            Rm, pm, _ = self.fk(*self._move(p, R, q, e, -eps))
            J[:, k] = (self._points(Rp, pp, b, local) - self._points(Rm, pm, b, local)) / (2 * eps)
        return J

    def terrain_points(self, p, R, q):
        """every contact point of the robot against the mesh terrain: [(body, point index, world position, terrain
        height h there, the triangle's normal, its barycentric margin, its half of the cell)]; in contact: h - z > 0"""
        Rs, ps, _ = self.fk(p, R, q)
        pts = np.asarray(self.tab["contact_point"], float)
        out = []
        for b in range(13):
            s, n = self.tab["contact_start"][b], self.tab["contact_count"][b]
            for c in range(s, s + n):
                x = self._points(Rs, ps, b, pts[c])
                out.append((b, c, x) + self.terrain.query(x[0], x[1]))
        return out

    def contacts(self, p, R, q, u, mu_ground, e_ground, mu_self, e_self, self_collision=True):
        """[(body, local point, normal, pen, other body's point or None, mu, episode slot or None)] of the state;
        episode slots: 2 leg + (0 shank, 1 foot), 4 + leg for the base box half the point belongs to"""
        Rs, ps, _ = self.fk(p, R, q)
        out = []
        pts = np.asarray(self.tab["contact_point"], float)
        for b in range(13):
            s, n = self.tab["contact_start"][b], self.tab["contact_count"][b]
            for c in range(s, s + n):
                x = self._points(Rs, ps, b, pts[c])
                slot = 4 + (c - s) * 2 // n if b == 0 else 2 * ((b - 1) // 6) + (1 if (b - 1) % 6 == 5 else 0)
                if self.terrain is not None:
                    h, nrm, _, _ = self.terrain.query(x[0], x[1])
                    if h - x[2] > 0:
                        out.append((b, pts[c], nrm, (h - x[2]) * nrm[2], None, mu_ground, slot))
                elif x[2] < 0:
                    out.append((b, pts[c], np.array([0.0, 0.0, 1.0]), -x[2], None, mu_ground, slot))
        if self_collision:
            caps = _capsules(self.tab)
            pairs = [(4, 10), (4, 12), (6, 10), (6, 12), (4, 6), (10, 12)]
            for a, bb in pairs:
                (a0, a1, ra), (b0, b1, rb) = caps[a], caps[bb]
                ca, cb = _closest_segments(self._points(Rs, ps, a, a0), self._points(Rs, ps, a, a1),
                                           self._points(Rs, ps, bb, b0), self._points(Rs, ps, bb, b1))
                dist = np.linalg.norm(ca - cb)
                if dist >= ra + rb:
                    continue
                n = (ca - cb) / dist            # pushes a out of b
                pen = ra + rb - dist
                x = cb + (rb - 0.5 * pen) * n   # the middle of the overlap
                la, lb = Rs[a].T @ (x - ps[a]), Rs[bb].T @ (x - ps[bb])
                out.append((a, la, n, pen, (bb, lb), mu_self, None))
                out.append((bb, lb, -n, pen, (a, la), mu_self, None))
        return out

    def velocities(self, p, R, q, u, points=(), eps=1e-6):
        """(COM velocity (13, 3), angular velocity (13, 3), velocity of each (body, local point) of `points`) at
        generalized speeds u: central differences of forward kinematics along the motion itself, J u as one
        directional difference (x(+eps u) - x(-eps u)) / 2 eps instead of jacobians() / point_jacobian()'s 18 columns
        times u (the same quantity to O(eps^2)); angular velocity from (R+ - R-) R^T / 2 eps, skew to O(eps^2)"""
        Rs, _, _ = self.fk(p, R, q)
        Rp, pp, cp = self.fk(*self._move(p, R, q, u, eps))
        Rm, pm, cm = self.fk(*self._move(p, R, q, u, -eps))
        vc = (np.array(cp) - np.array(cm)) / (2 * eps)
        wb = np.zeros((13, 3))
        for b in range(13):
            W = (Rp[b] - Rm[b]) @ Rs[b].T / (2 * eps)
            wb[b] = 0.5 * np.array([W[2, 1] - W[1, 2], W[0, 2] - W[2, 0], W[1, 0] - W[0, 1]])
        vx = np.array([(self._points(Rp, pp, b, local) - self._points(Rm, pm, b, local)) / (2 * eps)
                       for b, local in points]).reshape(len(points), 3)
        return vc, wb, vx

    def _target(self, e_ground, vimp):
        return e_ground * vimp if vimp > self.sv["bounce_threshold"] else 0.0

    def _contact_velocities(self, p, R, q, u, cons):
        """velocity of each contact's point relative to the surface it touches (the terrain: at rest; a self-contact:
        the other body's velocity at the same point)"""
        pts = [(c[0], c[1]) for c in cons] + [c[4] for c in cons if c[4] is not None]
        _, _, vx = self.velocities(p, R, q, u, pts)
        out, nxt = [], len(cons)
        for i, c in enumerate(cons):
            vp = vx[i]
            if c[4] is not None:
                vp, nxt = vp - vx[nxt], nxt + 1
            out.append(vp)
        return out

    def episodes_after(self, p, quat, w, v, q, qd, vimp, detail=None):
        """the restitution episodes after a substep that starts at this state with episodes vimp -- step()'s rule (a
        slot without a point in contact closes, an open one keeps its speed, a closed one opens at its fastest
        approach) without its dense solve; detail (a list): (slot, v_n) of every terrain point in contact is appended"""
        R = quat_to_R(quat)
        u = np.concatenate([w, v, qd])
        vimp = np.asarray(vimp, float)
        cons = [c for c in self.contacts(p, R, q, u, 0.0, 0.0, 0.0, 0.0, self_collision=False)]
        amax = np.full(6, -1.0)
        if cons:
            for c, vp in zip(cons, self._contact_velocities(p, R, q, u, cons)):
                amax[c[6]] = max(amax[c[6]], max(-(c[2] @ vp), 0.0))
                if detail is not None:
                    detail.append((c[6], float(c[2] @ vp)))
        return np.where(amax < 0, 0.0, np.where(vimp > 0, vimp, np.maximum(amax, 1e-6)))

    def report(self, p, quat, w, v, q, qd, vimp, mu_ground, e_ground, mu_self, self_collision=True, detail=None):
        """(rigid (13, 13), contact (13, 3)): the end-of-step report of DESIGN.md §4 at the state (p, quat, w, v_O, q,
        qd) with the restitution episodes vimp (6).  Rigid rows: frame origin, xyzw quaternion of the FK rotation, COM
        velocity, angular velocity.  Force rows: per contact point in contact f_n = max(k pen - [v_n < v_tgt] d (v_n -
        v_tgt), 0), f = f_n n - mu f_n v_t / max(|v_t|, v_s); v_tgt from the body's episode (the base box: the larger of
        its halves' targets), self-contact pairs with v_tgt = 0 and mu_self against the other body's point velocity.
        detail (a list): one dict per contact point is appended (body, other body or None, slot, v_n, v_tgt, |v_t|,
        the unclamped f_n, the force)."""
        k, d, vs = self.sv["k_contact"], self.sv["d_contact"], self.sv["friction_vs"]
        R = quat_to_R(quat)
        u = np.concatenate([w, v, qd])
        vimp = np.asarray(vimp, float)
        Rs, ps, _ = self.fk(p, R, q)
        cons = self.contacts(p, R, q, u, mu_ground, e_ground, mu_self, 0.0, self_collision)
        pts = [(c[0], c[1]) for c in cons] + [c[4] for c in cons if c[4] is not None]
        vc, wb, vx = self.velocities(p, R, q, u, pts)
        rigid = np.zeros((13, 13))
        for b in range(13):
            rigid[b] = np.concatenate([ps[b], R_to_quat(Rs[b]), vc[b], wb[b]])
        contact = np.zeros((13, 3))
        vt_base = max(self._target(e_ground, vimp[4]), self._target(e_ground, vimp[5]))
        nxt = len(cons)
        for i, (b, local, n, pen, other, mu, slot) in enumerate(cons):
            vp = vx[i]
            if other is not None:
                vp, nxt = vp - vx[nxt], nxt + 1
            vtg = 0.0 if slot is None else (vt_base if b == 0 else self._target(e_ground, vimp[slot]))
            vn = n @ vp
            vt = vp - vn * n
            raw = k * pen - (d * (vn - vtg) if vn < vtg else 0.0)
            fn = max(raw, 0.0)
            f = fn * n - mu * fn * vt / max(np.linalg.norm(vt), vs)
            contact[b] += f
            if detail is not None:
                detail.append({"body": b, "other": None if other is None else other[0], "slot": slot, "vn": vn,
                               "vtg": vtg, "vt": float(np.linalg.norm(vt)), "raw": raw, "force": f})
        return rigid, contact

    def switch_distance(self, p, quat, q):
        """per body (13), the smallest distance [m] of one of its contact candidates from the surface at which it
        switches between in and out of contact: |h - z| of a terrain point, |dist - (r_a + r_b)| of a capsule pair
        (both bodies); inf for bodies without candidates"""
        R = quat_to_R(quat)
        Rs, ps, _ = self.fk(p, R, q)
        out = np.full(13, np.inf)
        pts = np.asarray(self.tab["contact_point"], float)
        for b in range(13):
            s, n = self.tab["contact_start"][b], self.tab["contact_count"][b]
            for c in range(s, s + n):
                x = self._points(Rs, ps, b, pts[c])
                h = self.terrain.query(x[0], x[1])[0] if self.terrain is not None else 0.0
                out[b] = min(out[b], abs(h - x[2]))
        caps = _capsules(self.tab)
        for a, bb in [(4, 10), (4, 12), (6, 10), (6, 12), (4, 6), (10, 12)]:
            (a0, a1, ra), (b0, b1, rb) = caps[a], caps[bb]
            ca, cb = _closest_segments(self._points(Rs, ps, a, a0), self._points(Rs, ps, a, a1),
                                       self._points(Rs, ps, bb, b0), self._points(Rs, ps, bb, b1))
            gap = abs(np.linalg.norm(ca - cb) - ra - rb)
            out[a], out[bb] = min(out[a], gap), min(out[bb], gap)
        return out

    def step(self, p, quat, w, v, q, qd, tau, dt, mu_ground, e_ground, mu_self, e_self, f_base=None,
             self_collision=True, g=9.81, vimp=None):
        """(du over one substep (u = [omega, v_O, qd]), the restitution episodes after it)"""
        sv = self.sv
        k, d, vs = sv["k_contact"], sv["d_contact"], sv["friction_vs"]
        R = quat_to_R(quat)
        u = np.concatenate([w, v, qd])
        acc, Mm = self.accel(p, quat, w, v, q, qd, np.zeros(12), g=g, f_base=f_base)
        # accel() gives the classical acceleration of the (moving) base origin; the substep's du is taken about the point
        # O fixed where the base origin is at the substep's start: the spatial acceleration a_O - w x v_O
        acc = acc.copy()
        acc[3:6] -= np.cross(w, v)
        f0 = Mm @ acc                        # the generalized force without tau: J_base^T f_base - h(q, u)
        A = Mm.copy()
        rhs = dt * (np.concatenate([np.zeros(6), tau]) + f0)
        vimp = np.zeros(6) if vimp is None else np.asarray(vimp, float)
        amax = np.full(6, -1.0)
        for b, local, n, pen, other, mu, slot in self.contacts(p, R, q, u, mu_ground, e_ground, mu_self, e_self,
                                                               self_collision):
            J = self.point_jacobian(p, R, q, b, local)
            vp = J @ u
            if other is not None:
                vp = vp - self.point_jacobian(p, R, q, other[0], other[1]) @ u
            vn = n @ vp
            vt = vp - vn * n
            vtg = 0.0
            if slot is not None:
                vtg = e_ground * vimp[slot] if vimp[slot] > sv["bounce_threshold"] else 0.0
                amax[slot] = max(amax[slot], max(-vn, 0.0))
            approach, below = vn < 0, 0 <= vn < vtg
            cn = dt * k + d if approach else (d if below else 0.0)
            fn_est = k * pen + (-d * vn if approach else (d * (vtg - vn) if below else 0.0))
            ct = mu * fn_est / max(np.linalg.norm(vt), vs)
            f = (k * pen - cn * vn + (d * vtg if below else 0.0)) * n - ct * vt
            C = cn * np.outer(n, n) + ct * (np.eye(3) - np.outer(n, n))
            A += dt * J.T @ C @ J
            rhs += dt * J.T @ f
        for j in range(12):
            kl, dl = sv["k_limit"], sv["d_limit"]
            if q[j] < self.lo[j]:
                cl = dt * kl + dl if qd[j] < 0 else 0.0
                A[6 + j, 6 + j] += dt * cl
                rhs[6 + j] += dt * (kl * (self.lo[j] - q[j]) - cl * qd[j])
            elif q[j] > self.hi[j]:
                cl = dt * kl + dl if qd[j] > 0 else 0.0
                A[6 + j, 6 + j] += dt * cl
                rhs[6 + j] += dt * (kl * (self.hi[j] - q[j]) - cl * qd[j])
        new = np.where(amax < 0, 0.0, np.where(vimp > 0, vimp, np.maximum(amax, 1e-6)))
        return np.linalg.solve(A, rhs), new   # du = change of [omega, v_O (spatial, about O), qd]; episodes
