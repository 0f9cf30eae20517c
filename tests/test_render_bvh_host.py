"""csrc/t1render_bvh.h on the host: the builder of the robot mesh's hierarchies compiled with tests/render_bvh_main.cpp by
the host compiler, once more with -fsanitize=address,undefined (a plain executable, run directly), and its output
examined: every triangle in exactly one leaf, leaves of at most four, every box around what lies below it, the depth
bound, the same bytes on a second build, termination on identical triangles, and the refusals."""
import math
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import render_scenes_mesh as SM  # noqa: E402

NB = 13
NODE = np.dtype([("lo", "<f4", 3), ("hi", "<f4", 3), ("a", "<i4"), ("b", "<i4")])
TRI = np.dtype([("v0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("idx", "<i4"), ("rgb", "<u4"), ("body", "<i4")])
OK, E_NULL, E_NTRI, E_BODY, E_FINITE = 0, 1, 2, 3, 4


def _compile(tmp, flags, name):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, "-o", exe, os.path.join(HERE, "render_bvh_main.cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bvh")
    return tmp, (_compile(tmp, ["-Wall", "-Wextra", "-Werror"], "bvh_plain"),
                 _compile(tmp, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "bvh_san"))


def _run(exe, tmp, tri, body, rgb, tag):
    src, dst = str(tmp / (tag + ".in")), str(tmp / (tag + ".out"))
    tri = np.ascontiguousarray(tri, "<f4").reshape(-1, 9)
    with open(src, "wb") as f:
        f.write(struct.pack("<i", len(tri)) + tri.tobytes() + np.asarray(body, "<i4").tobytes() +
                np.asarray(rgb, "<u4").tobytes())
    subprocess.run([exe, src, dst], check=True, timeout=120)
    raw = open(dst, "rb").read()
    status, same, nnodes, ntri, depth = struct.unpack("<5i", raw[:20])
    out = dict(status=status, same=same, nnodes=nnodes, ntri=ntri, max_depth=depth, raw=raw)
    if status == OK:
        o = 20
        for k, t in (("root", "<i4"), ("first", "<i4"), ("count", "<i4"), ("radius", "<f4")):
            out[k] = np.frombuffer(raw, t, NB, o)
            o += 4 * NB
        out["nodes"] = np.frombuffer(raw, NODE, nnodes, o)
        out["tris"] = np.frombuffer(raw, TRI, ntri, o + nnodes * NODE.itemsize)
        assert len(raw) == o + nnodes * NODE.itemsize + ntri * TRI.itemsize
    return out


def _check(out, tri, body, rgb):
    """The invariants of a build of (tri, body, rgb)."""
    tri = np.asarray(tri, np.float32).reshape(-1, 3, 3)
    n = len(tri)
    assert out["status"] == OK and out["same"] == 1 and out["ntri"] == n
    nodes, tris = out["nodes"], out["tris"]
    assert sorted(tris["idx"].tolist()) == list(range(n))            # every triangle once in leaf order
    assert np.array_equal(tris["body"], np.asarray(body)[tris["idx"]]) and np.array_equal(tris["rgb"], np.asarray(rgb)[tris["idx"]])
    assert np.array_equal(tris["v0"], tri[tris["idx"], 0])
    in_leaf = np.zeros(n, int)
    seen = np.zeros(len(nodes), int)
    deepest = 0
    for b in range(NB):
        cnt = int((np.asarray(body) == b).sum())
        assert out["count"][b] == cnt
        if cnt == 0:
            assert out["root"][b] == -1 and out["radius"][b] == 0
            continue
        assert (tris["body"][out["first"][b]:out["first"][b] + cnt] == b).all()
        stack = [(int(out["root"][b]), 0)]
        deep_b = 0   # this body's deepest leaf
        while stack:
            i, depth = stack.pop()
            seen[i] += 1
            N = nodes[i]
            assert (N["lo"] <= N["hi"]).all()
            if N["b"] > 0:
                assert N["b"] <= 4 and out["first"][b] <= N["a"] and N["a"] + N["b"] <= out["first"][b] + cnt
                deep_b = max(deep_b, depth)
                for k in range(N["a"], N["a"] + N["b"]):
                    in_leaf[k] += 1
                    v = tri[tris["idx"][k]]
                    assert (v >= N["lo"]).all() and (v <= N["hi"]).all()       # the caller's vertices, all three
                    assert (np.linalg.norm(v.astype(np.float64), axis=1) <= out["radius"][b]).all()
            else:
                assert N["b"] == 0
                for c in (N["a"], N["a"] + 1):
                    assert (nodes[c]["lo"] >= N["lo"]).all() and (nodes[c]["hi"] <= N["hi"]).all()
                    stack.append((int(c), depth + 1))
        assert deep_b <= (math.ceil(math.log2(cnt)) if cnt > 1 else 0), (b, cnt, deep_b)
        deepest = max(deepest, deep_b)
    assert (in_leaf == 1).all() and (seen == 1).all()
    assert out["max_depth"] == deepest and deepest <= (math.ceil(math.log2(n)) if n > 1 else 0) and deepest <= 18
    # a triangle's stored edges are its own, or zero where it has no area
    e1 = tri[tris["idx"], 1].astype(np.float64) - tri[tris["idx"], 0]
    e2 = tri[tris["idx"], 2].astype(np.float64) - tri[tris["idx"], 0]
    flat = (np.cross(e1, e2) == 0).all(1)
    assert np.array_equal(tris["e1"], np.where(flat[:, None], 0, e1).astype(np.float32))
    assert np.array_equal(tris["e2"], np.where(flat[:, None], 0, e2).astype(np.float32))
    return flat


def _random(n, seed):
    rng = np.random.default_rng(seed)
    tri = (rng.uniform(-0.5, 0.5, (n, 1, 3)) + rng.uniform(-0.03, 0.03, (n, 3, 3))).astype(np.float32)
    return tri, rng.integers(0, NB, n).astype(np.int32), rng.integers(0, 1 << 24, n).astype(np.uint32)


@pytest.mark.parametrize("n", [0, 1, 4, 5, 9, 4096])
def test_random_meshes_on_one_body_and_on_thirteen(programs, n):
    tmp, exes = programs
    tri, body, rgb = _random(n, 100 + n)
    for k, exe in enumerate(exes):   # plain, then under the sanitizers
        _check(_run(exe, tmp, tri, body, rgb, "r%d_%d" % (n, k)), tri, body, rgb)
        one = np.full(n, 7, np.int32)
        out = _run(exe, tmp, tri, one, rgb, "o%d_%d" % (n, k))
        _check(out, tri, one, rgb)
        if n:
            assert out["nnodes"] >= 1 and out["root"][7] == 0
    if n == 4096:   # two runs of one program, two programs: the same bytes
        assert _run(exes[0], tmp, tri, body, rgb, "a")["raw"] == _run(exes[1], tmp, tri, body, rgb, "b")["raw"]


def test_the_ankle_stl(programs):
    tmp, exes = programs
    tri = SM.ankle("L")
    assert 1900 <= len(tri) <= 2100
    body, rgb = np.full(len(tri), 6, np.int32), np.arange(len(tri), dtype=np.uint32)
    for k, exe in enumerate(exes):
        out = _run(exe, tmp, tri, body, rgb, "ankle%d" % k)
        _check(out, tri, body, rgb)
        assert out["max_depth"] <= 9 and 0 < out["radius"][6] < 0.3


def test_identical_triangles_terminate_and_ties_go_to_the_lower_index(programs):
    tmp, exes = programs
    one = np.array([[(0.1, 0.2, 0.3), (0.2, 0.2, 0.3), (0.1, 0.3, 0.35)]], np.float32)
    tri = np.repeat(one, 37, 0)
    body, rgb = np.zeros(37, np.int32), np.arange(37, dtype=np.uint32)
    for k, exe in enumerate(exes):
        out = _run(exe, tmp, tri, body, rgb, "same%d" % k)
        _check(out, tri, body, rgb)
        assert out["tris"]["idx"].tolist() == list(range(37))   # equal centroids: the caller's order throughout


def test_zero_area_triangles_keep_their_place_with_zero_edges(programs):
    tmp, exes = programs
    tri, body, rgb = _random(9, 5)
    tri[3, 1] = tri[3, 0]                                  # two equal vertices
    tri[6] = np.float32([(0, -1, 0), (0, 0, 0), (0, 2, 0)])  # three on a line
    flat = _check(_run(exes[1], tmp, tri, body, rgb, "flat"), tri, body, rgb)
    assert flat.sum() == 2


def test_refusals(programs):
    tmp, exes = programs
    tri, body, rgb = _random(5, 9)
    for bad_body in (-1, 13):
        b = body.copy()
        b[2] = bad_body
        assert _run(exes[1], tmp, tri, b, rgb, "bb")["status"] == E_BODY
    for bad in (np.nan, np.inf, -np.inf):
        t = tri.copy()
        t[4, 2, 1] = bad
        assert _run(exes[1], tmp, t, body, rgb, "bf")["status"] == E_FINITE
