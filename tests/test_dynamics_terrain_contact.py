"""The solver's terrain contact ON A SLOPED HEIGHT FIELD against an independent formulation that works on the triangle
mesh -- host builds of the product header, no GPU.

tests/test_dynamics_contact.py compares one substep in contact on the plane z = 0, where every normal is (0, 0, 1).
Here the same comparison runs on a small synthetic height field (tests/terrain_contact_scenarios.py: a rough tilted
region and a 0.25 m step), with oracle/dynamics_ref.py ContactRobot given a MeshTerrain: the explicit triangle list of
the field, the containing triangle found by a barycentric test, the height interpolated and the normal taken from the
triangle's edges -- none of the header's cell indexing, diagonal split or slope formulas.  What it pins: the
(x + border) / hscale indexing with rows along x, the choice of triangle, the slopes, the normal, the depth
(h - z) n_z, and the contact law (approach speed n . v, friction's tangential projector, the restitution episodes)
with tilted normals, for both fp64 compositions and both height-field mesh types.

Bound: |du_solver - du_ref| <= 1e-5 (1 + |du_ref|_max) per env, the episodes after the substep at rtol 1e-5 / atol
1e-6 (tests/test_dynamics_contact.py's; measured worst 1e-6 .. 2e-6).  Control: the same solver output against the
reference made blind to the field (the plane z = 0) must miss by at least 100 x the bound in each kind's worst env, so
the comparison cannot pass with the terrain ignored.  The host fp32 builds' worst errors are printed: they are the
yardstick for the GPU kernels' bound in tests/test_gpu_dynamics_terrain_contact.py.

Not covered: points beyond the field's edge (the header clamps, extruding the edge profile but keeping an interior
slope in the normal) and the reference's steep-slope vertex correction.  The contact_forces / rigid_state report on
the same field is pinned by tests/test_dynamics_report.py and tests/test_gpu_dynamics_report.py.
"""
import numpy as np
import pytest

import terrain_contact_scenarios as tcs
from test_dynamics_contact import host_du, make_setup, ref_du

BOUND, BOUND_FP32 = 1e-5, 1e-4


@pytest.fixture(scope="module")
def setup():
    return make_setup()


_CASES = {}


def case(setup, kind):
    """one kind's inputs, the mesh reference's du / episodes and the blind (plane) reference's du -- computed once"""
    if kind not in _CASES:
        dyn, m, tab = setup
        assert abs(m.bounce_threshold - tcs.BOUNCE_THRESHOLD) < 1e-6
        field = tcs.make_field()
        terrain = tcs.mesh_terrain(field)
        root, dof, vimp, facts = tcs.scenario(kind, tab, terrain)
        rng = np.random.default_rng(900 + tcs.KINDS.index(kind))
        n = root.shape[0]
        c = {"field": field, "root": root, "dof": dof, "vimp": vimp, "facts": facts,
             "tau": rng.normal(0, 20, (n, 12)).astype(np.float32), "fr": rng.uniform(0.2, 1.3, n),
             "rst": rng.uniform(0.0, 0.4, n), "episodes": []}
        c["ref"] = ref_du(setup, root, dof, c["tau"], c["fr"], c["rst"], vimp=vimp, episodes=c["episodes"],
                          terrain=terrain)
        c["blind"] = ref_du(setup, root, dof, c["tau"], c["fr"], c["rst"], vimp=vimp)
        _CASES[kind] = c
    return _CASES[kind]


def solver_du(setup, c, flags, mesh):
    du, r0, d0, ep = host_du(setup, c["root"], c["dof"], c["tau"], c["fr"], c["rst"], flags, vimp=c["vimp"],
                             terrain=(c["field"], tcs.HS, tcs.VS, tcs.BORDER, mesh))
    assert np.array_equal(r0, c["root"]) and np.array_equal(d0, c["dof"])   # the scenario's states are fp32-exact
    return du, ep


def rel_err(du, ref):
    return np.abs(du - ref).max(axis=1) / (1.0 + np.abs(ref).max(axis=1))


@pytest.mark.parametrize("kind", tcs.KINDS)
def test_scenario_conditions(setup, kind):
    c = case(setup, kind)
    tcs.check_kind(kind, c["facts"], c["vimp"])
    f = c["facts"]
    print(kind, "contacts", sum(x["contacts"] for x in f), "min margin %.2e" % min(x["margin"] for x in f),
          "min |h - z| %.2e" % min(x["clearance"] for x in f), "cull-condition envs",
          sum(x["cull_condition"] > 0 for x in f), "base contacts", sum(x["base_contacts"] for x in f))


@pytest.mark.parametrize("mesh", [1, 2], ids=["heightfield", "trimesh"])
@pytest.mark.parametrize("flags", [1, 3], ids=["assembled", "split"])
@pytest.mark.parametrize("kind", tcs.KINDS)
def test_terrain_contact_substep_matches_mesh_reference(setup, kind, flags, mesh):
    c = case(setup, kind)
    tcs.check_kind(kind, c["facts"], c["vimp"])
    du, ep = solver_du(setup, c, flags, mesh)
    err = rel_err(du, c["ref"])
    blind = rel_err(du, c["blind"])
    print(f"{kind}: worst |solver - ref| / (1 + |ref|max) {err.max():.2e}; against the plane z = 0 {blind.max():.2e}")
    np.testing.assert_allclose(ep, np.array(c["episodes"]), rtol=1e-5, atol=1e-6)
    for i in range(len(err)):
        assert err[i] <= BOUND, f"{kind} env {i} ({c['facts'][i]['contacts']} contacts): |solver - ref| {err[i]:.3g}"
    assert blind.max() >= 100 * BOUND, f"{kind}: a reference blind to the terrain is only {blind.max():.3g} away"


@pytest.mark.parametrize("kind", tcs.KINDS)
def test_host_fp32_error_on_terrain(setup, kind, capsys):
    """the host fp32 builds of the same header (flags 0, 2) against the mesh reference: the figure the GPU kernels'
    bound (1e-4) is judged against -- printed per kind, and itself inside that bound"""
    c = case(setup, kind)
    worst = {}
    for name, flags in (("assembled", 0), ("split", 2)):
        for mesh in (1, 2):
            du, _ = solver_du(setup, c, flags, mesh)
            err = rel_err(du, c["ref"])
            worst[name] = max(worst.get(name, 0.0), float(err.max()))
            assert err.max() <= BOUND_FP32, f"{kind} {name}: host fp32 |solver - ref| {err.max():.3g} (env {err.argmax()})"
    with capsys.disabled():
        print(f"\nhost fp32 on terrain, {kind}: worst |solver - ref| / (1 + |ref|max)",
              {k: f"{v:.2e}" for k, v in worst.items()})
