"""The robot description as it stands, every link its own rigid body (TEST INFRASTRUCTURE, fp64 numpy).

utils/urdf.py collapses the description's 24 links into 13 bodies (fixed-joint merge, parallel-axis sums, rotated
inertial frames), and both the kernels and every fp64 reference of oracle/dynamics_ref.py read those tables.  This module
reads the URDF on its own -- its own parser, its own rpy conversion (Rodrigues' formula per axis), no body list, nothing
imported from utils/urdf.py -- and keeps the tree uncollapsed: a fixed joint is a zero-DOF edge with its own xyz / rpy,
and every link keeps its own mass, COM and inertia.  `accel` is Kane's projected Newton-Euler summed over all links, in
oracle/dynamics_ref.py Robot.accel's convention (u = [omega world, v base origin, qd]); of that module it uses only the
first-order configuration move and the quaternion conversion, never Robot.fk or a collapsed table entry.
"""
import os
import xml.etree.ElementTree as ET

import numpy as np

from oracle.dynamics_ref import Robot, quat_to_R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t1_robot", "urdf", "t1.urdf")


def floats(s, n=3):
    return np.array([float(x) for x in s.split()], dtype=np.float64) if s else np.zeros(n)


def rodrigues(axis, angle):
    """rotation by `angle` about the unit vector `axis`: I + sin K + (1 - cos) K^2"""
    a = np.asarray(axis, float)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def rpy_matrix(rpy):
    """URDF fixed-axis roll, pitch, yaw: about x, then y, then z of the parent frame"""
    return rodrigues([0, 0, 1], rpy[2]) @ rodrigues([0, 1, 0], rpy[1]) @ rodrigues([1, 0, 0], rpy[0])


def origin(el):
    """(xyz, rotation) of an element's <origin> child (identity when absent)"""
    o = el.find("origin") if el is not None else None
    if o is None:
        return np.zeros(3), np.eye(3)
    return floats(o.get("xyz")), rpy_matrix(floats(o.get("rpy")))


class LinkTree:
    """Every link and joint of a URDF.  dof_names: the joint name of each generalized coordinate, in order."""

    def __init__(self, urdf_path, dof_names):
        self.path = urdf_path
        root = ET.parse(urdf_path).getroot()
        self.dof = {n: k for k, n in enumerate(dof_names)}
        self.links = {}      # name -> (mass, COM in the link frame, inertia about the COM in the link frame)
        self.elements = {}   # name -> the <link> element (collision geometry for the geometry checks)
        for ln in root.findall("link"):
            inert = ln.find("inertial")
            c, Rc = origin(inert)
            I = inert.find("inertia")
            g = {k: float(I.get(k)) for k in ("ixx", "ixy", "ixz", "iyy", "iyz", "izz")}
            Il = np.array([[g["ixx"], g["ixy"], g["ixz"]], [g["ixy"], g["iyy"], g["iyz"]], [g["ixz"], g["iyz"], g["izz"]]])
            self.links[ln.get("name")] = (float(inert.find("mass").get("value")), c, Rc @ Il @ Rc.T)
            self.elements[ln.get("name")] = ln
        self.joints = {}     # name -> dict(type, parent, child, xyz, R, axis, limit)
        self.children = {}   # parent link -> [joint name]
        kids = set()
        for j in root.findall("joint"):
            xyz, Rj = origin(j)
            ax, lim = j.find("axis"), j.find("limit")
            rec = {"type": j.get("type"), "parent": j.find("parent").get("link"), "child": j.find("child").get("link"),
                   "xyz": xyz, "R": Rj, "axis": floats(ax.get("xyz")) if ax is not None else None,
                   "limit": None if lim is None else {k: float(lim.get(k)) for k in ("lower", "upper", "effort", "velocity")}}
            assert rec["type"] in ("fixed", "revolute"), (j.get("name"), rec["type"])
            self.joints[j.get("name")] = rec
            self.children.setdefault(rec["parent"], []).append(j.get("name"))
            kids.add(rec["child"])
        roots = [n for n in self.links if n not in kids]
        assert len(roots) == 1, roots
        self.root = roots[0]
        moving = sorted(n for n, j in self.joints.items() if j["type"] != "fixed")
        assert moving == sorted(self.dof), (moving, sorted(self.dof))
        self.order = [name for name, _, _ in self._walk(np.zeros(3), np.eye(3), np.zeros(len(self.dof)))]
        assert sorted(self.order) == sorted(self.links), "a link is not reached from the root"

    def _walk(self, p, R, q):
        """(link, frame origin, frame rotation) of every link, depth first from the root"""
        stack = [(self.root, np.asarray(p, float), np.asarray(R, float))]
        while stack:
            name, pl, Rl = stack.pop()
            yield name, pl, Rl
            for jn in self.children.get(name, []):
                j = self.joints[jn]
                Rn = Rl @ j["R"]
                if j["type"] != "fixed":
                    Rn = Rn @ rodrigues(j["axis"], q[self.dof[jn]])
                stack.append((j["child"], pl + Rl @ j["xyz"], Rn))

    def frames(self, p, R, q):
        """{link: (frame origin, frame rotation)} in the world"""
        return {name: (pl, Rl) for name, pl, Rl in self._walk(p, R, q)}

    def fk(self, p, R, q):
        """per link (self.order): world COM, rotation, inertia about the COM in the link frame"""
        out = []
        for name, pl, Rl in self._walk(p, R, q):
            _, c, I = self.links[name]
            out.append((pl + Rl @ c, Rl, I))
        return out

    def rigid_group(self, name):
        """(mass, COM in `name`'s frame) of a link together with everything fixed to it: what moves as one body"""
        m_tot, mc = 0.0, np.zeros(3)
        stack = [(name, np.zeros(3), np.eye(3))]
        while stack:
            ln, pl, Rl = stack.pop()
            m, c, _ = self.links[ln]
            m_tot += m
            mc += m * (pl + Rl @ c)
            for jn in self.children.get(ln, []):
                j = self.joints[jn]
                if j["type"] == "fixed":
                    stack.append((j["child"], pl + Rl @ j["xyz"], Rl @ j["R"]))
        return m_tot, mc / m_tot

    def masses(self):
        return np.array([self.links[n][0] for n in self.order])

    def jacobians(self, p, R, q, eps=1e-6):
        nl, nu = len(self.order), 6 + len(self.dof)
        Jv, Jw = np.zeros((nl, 3, nu)), np.zeros((nl, 3, nu))
        for k in range(nu):
            e = np.zeros(nu)
            e[k] = 1.0
            A = self.fk(*Robot._move(p, R, q, e, eps))
            B = self.fk(*Robot._move(p, R, q, e, -eps))
            for b in range(nl):
                Jv[b, :, k] = (A[b][0] - B[b][0]) / (2 * eps)
                W = (A[b][1] - B[b][1]) @ A[b][1].T / (2 * eps)   # skew(w) to first order
                Jw[b, :, k] = [W[2, 1], W[0, 2], W[1, 0]]
        return Jv, Jw

    def accel(self, p, quat, w, v, q, qd, tau, armature, g=9.81, eps=1e-5):
        """(generalized accelerations [omega_dot, a of the base origin (classical), qdd], M)"""
        R = quat_to_R(quat)
        u = np.concatenate([w, v, qd])
        Jv, Jw = self.jacobians(p, R, q)
        Jvp, Jwp = self.jacobians(*Robot._move(p, R, q, u, eps))
        Jvm, Jwm = self.jacobians(*Robot._move(p, R, q, u, -eps))
        m = self.masses()
        nu = len(u)
        M, h = np.zeros((nu, nu)), np.zeros(nu)
        grav = np.array([0.0, 0.0, -g])
        for b, (_, Rl, I) in enumerate(self.fk(p, R, q)):
            Iw = Rl @ I @ Rl.T
            wb = Jw[b] @ u
            M += m[b] * Jv[b].T @ Jv[b] + Jw[b].T @ Iw @ Jw[b]
            h += Jv[b].T @ (m[b] * ((Jvp[b] - Jvm[b]) @ u / (2 * eps) - grav)) \
                + Jw[b].T @ (Iw @ ((Jwp[b] - Jwm[b]) @ u / (2 * eps)) + np.cross(wb, Iw @ wb))
        M[6:, 6:] += np.diag(np.asarray(armature, float))
        return np.linalg.solve(M, np.concatenate([np.zeros(6), tau]) - h), M
