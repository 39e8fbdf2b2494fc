"""CPU: user-defined implicit surfaces as verified 3-D Chebyshev series (optable_amd/implicit.py) — the fit (degrees, measured
error), what is refused under the opt-in and with it off, the compiled node and its record, the C header against abi.py."""
import os
import re
import types

import numpy as np
import pytest

import implicit_scenes
import optable_amd as oa
from optable_amd import abi, implicit, shapes
from optable_amd.scene import SceneError, compile_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = implicit_scenes.implicit_surface_classes(oa)


class Quadric(oa.Surface):
    """x + 0.1 y^2 + 0.05 z^2 + 0.02 x y + 0.03 x^2 = 0: a tilted, non-rotational quadric."""

    def __init__(self, a=1.0):
        super().__init__()
        self.planar, self.a = False, a

    def f(self, P):
        return P[0] + 0.1 * P[1] ** 2 + 0.05 * P[2] ** 2 + 0.02 * P[0] * P[1] + 0.03 * P[0] ** 2

    def normal(self, P):
        g = np.array([1 + 0.02 * P[1] + 0.06 * P[0], 0.2 * P[1] + 0.02 * P[0], 0.1 * P[2]])
        return g / np.linalg.norm(g)

    def within_boundary(self, P):
        return True

    def get_bbox_local(self):
        return (-0.2, 0.05, -self.a, self.a, -self.a, self.a)


class Biconic(oa.Surface):
    """x = -(cy y^2 / (1 + sqrt(1 - (1 + ky) cy^2 y^2)) + cz z^2 / (1 + sqrt(1 - (1 + kz) cz^2 z^2))): not a polynomial."""

    def __init__(self, cy=0.2, cz=0.1, ky=-0.5, kz=0.3, a=1.0):
        super().__init__()
        self.planar = False
        self.cy, self.cz, self.ky, self.kz, self.a = cy, cz, ky, kz, a

    @staticmethod
    def _sag(c, k, u):
        return c * u * u / (1 + np.sqrt(1 - (1 + k) * c * c * u * u))

    @staticmethod
    def _slope(c, k, u):
        return c * u / np.sqrt(1 - (1 + k) * c * c * u * u)

    def f(self, P):
        return P[0] + self._sag(self.cy, self.ky, P[1]) + self._sag(self.cz, self.kz, P[2])

    def normal(self, P):
        g = np.array([1.0, self._slope(self.cy, self.ky, P[1]), self._slope(self.cz, self.kz, P[2])])
        return g / np.linalg.norm(g)

    def within_boundary(self, P):
        return abs(P[1]) <= self.a and abs(P[2]) <= self.a

    def get_bbox_local(self):
        return (-0.2, 0.01, -self.a, self.a, -self.a, self.a)


def _mirror(surf):
    return U["CurvedMirror"]([0, 0, 0], surf)


@pytest.mark.parametrize("name,surf,max_deg", [
    ("torus", U["Torus"](10.0, 4.0, 1.5), 5),
    ("saddle", U["Saddle"](8.0, 1.5), 3),
    ("quadric", Quadric(), 3),
    ("biconic", Biconic(), 47),
])
def test_fit_degrees_and_measured_error(name, surf, max_deg):
    m = implicit.measure(surf, name)
    assert max(m.degrees) <= max_deg, m.degrees
    assert m.rel_err <= implicit.REL_TOL, m.rel_err
    rng = np.random.default_rng(3)
    P = m.lo[:, None] + (m.hi - m.lo)[:, None] * rng.random((3, 500))
    want = np.array([surf.f(P[:, k]) for k in range(P.shape[1])])
    assert np.abs(m.evaluate(P) - want).max() <= implicit.REL_TOL * m.fmax
    rec = m.record()
    assert rec[18] == m.rel_err and len(rec) == implicit.HEADER + 4 * int(np.prod(m.coef.shape))


def test_polynomials_come_out_at_their_own_degree():
    assert implicit.measure(U["Torus"](10.0, 4.0, 1.5)).degrees == (4, 4, 4)
    assert implicit.measure(U["Saddle"](8.0, 1.5)).degrees == (1, 2, 2)
    assert implicit.measure(U["ImplicitSphere"](20.0, 0.2)).degrees == (2, 2, 2)


def test_apertures_and_normal_sign_are_measured():
    m = implicit.measure(U["Torus"](10.0, 4.0, 1.5))
    assert m.aperture == implicit.APERTURE_DISC and m.radius == pytest.approx(1.5) and m.sign == 1.0
    assert implicit.measure(U["ImplicitCylinder"](1.0, 2.0)).aperture == implicit.APERTURE_BOX
    assert implicit.measure(Biconic()).aperture == implicit.APERTURE_BOX

    class Inward(U["ImplicitSphere"]):
        def normal(self, P):
            return -super().normal(P)

    assert implicit.measure(Inward(20.0, 0.2)).sign == -1.0


def _refused(surf, match):
    with pytest.raises(SceneError, match=match):
        compile_scene([_mirror(surf)], implicit_surfaces=True)


def test_refusals_name_what_was_measured():
    class Kink(U["Saddle"]):
        def f(self, P):
            return P[0] + 0.1 * abs(P[1])

    _refused(Kink(8.0, 1.5), "kink")

    class Pole(U["Saddle"]):
        def f(self, P):
            return P[0] + 0.01 / (P[1] - 0.123)

    _refused(Pole(8.0, 1.5), "not finite|kink|degree cap")

    class Raises(U["Saddle"]):
        def f(self, P):
            raise ValueError("no")

    _refused(Raises(8.0, 1.5), "f raised ValueError")

    class HalfFlipped(U["Saddle"]):
        def normal(self, P):
            n = super().normal(P)
            return n if P[1] >= 0 else -n

    _refused(HalfFlipped(8.0, 1.5), "normal")

    class Annulus(U["Torus"]):
        def within_boundary(self, P):
            return 0.5 <= np.hypot(P[1], P[2]) <= self.a

    _refused(Annulus(10.0, 4.0, 1.5), "none of the aperture families")

    class Flat(U["Saddle"]):
        def get_bbox_local(self):
            return (0.0, 0.0, -1.0, 1.0, -1.0, 1.0)

    _refused(Flat(8.0, 1.5), "degenerate")


def test_a_callable_roc_is_refused():
    class WithRoc(U["Saddle"]):
        def roc(self, P):
            return 10.0

    comp = U["CurvedInterface"]([0, 0, 0], WithRoc(8.0, 1.5), n1=1.0, n2=1.5)
    comp.roc = comp.surface.roc  # what the reference's constructor keeps when given the surface (optical_component.py:615)
    with pytest.raises(SceneError, match="callable roc"):
        compile_scene([comp], implicit_surfaces=True)
    comp.roc = 12.5  # a number is the constant ROC
    scene = compile_scene([comp], implicit_surfaces=True)
    assert scene.nodes[0].shape == shapes.IMPLICIT_CHEB and scene.nodes[0].roc == 12.5


def test_without_the_switch_the_old_refusals_stand():
    import scenes

    class Saddle(scenes.user_surface_classes(oa)["Saddle"]):
        def normal(self, P):  # (the fixture class keeps its paraboloid's normal: the implicit path refuses that one)
            n = np.array([1.0, P[1] / (2 * self.focal), -P[2] / (2 * self.focal)])
            return n / np.linalg.norm(n)

    saddle = Saddle(4.0, 2.0)
    with pytest.raises(SceneError, match="normal"):
        compile_scene([U["CurvedMirror"]([0, 0, 0], scenes.user_surface_classes(oa)["Saddle"](4.0, 2.0))], implicit_surfaces=True)
    comp = U["CurvedMirror"]([0, 0, 0], saddle)
    with pytest.raises(SceneError, match="not c \\* \\(x \\+ F\\(r\\)\\).*implicit_surfaces=True"):
        compile_scene([comp])
    assert compile_scene([comp], implicit_surfaces=True).nodes[0].shape == shapes.IMPLICIT_CHEB  # (the memo is keyed on the switch)
    with pytest.raises(SceneError, match="not c \\* \\(x \\+ F\\(r\\)\\)"):
        compile_scene([comp])
    t = oa.OpticalTable()
    t.add_components([comp])
    with pytest.raises(SceneError):
        t.compile()
    t.implicit_surfaces = True
    assert t.compile().nodes[0].shape == shapes.IMPLICIT_CHEB
    # surfaces that a built-in shape reproduces keep that shape under the switch
    para = scenes.user_surface_classes(oa)["Paraboloid"](4.0, 2.0)
    assert compile_scene([U["CurvedMirror"]([0, 0, 0], para)], implicit_surfaces=True).nodes[0].shape == shapes.ASPHERE_CHEB

    class Blob(oa.Plane):  # planar user surfaces keep their path and refusals
        def within_boundary(self, P):
            return P[1] ** 2 + 3 * P[2] ** 2 < 1

        def get_bbox_local(self):
            return (0, 0, -1, 1, -1, 1)

    with pytest.raises(SceneError, match="neither the disc nor the rectangle"):
        compile_scene([U["CurvedMirror"]([0, 0, 0], Blob())], implicit_surfaces=True)


def test_installed_mode_reads_the_switch_from_the_table():
    class Table:
        components, unit = [], 1e-2

        def ray_tracing(self, rays, perfomance_limit=None):
            return []

    class Monitor:
        def record(self, rays):
            pass

    module = types.SimpleNamespace(OpticalTable=Table, Monitor=Monitor, Ray=object)
    undo = oa.install(module)
    try:
        t = Table()
        t.components = [U["CurvedMirror"]([0, 0, 0], U["Torus"](10.0, 4.0, 1.5))]
        with pytest.raises(SceneError, match="implicit_surfaces=True"):
            t.compile()
        Table.implicit_surfaces = True
        assert t.compile().nodes[0].shape == shapes.IMPLICIT_CHEB
    finally:
        undo()


def test_node_box_record_and_table_round_trip():
    sc = implicit_scenes.g29_implicit_surfaces(oa)
    scene = compile_scene(sc["components"], implicit_surfaces=True)
    leaves = [n for n in scene.nodes[: scene.n_nodes] if n.kind == abi.NODE_LEAF]
    assert [n.shape for n in leaves] == [shapes.IMPLICIT_CHEB, shapes.CIRCLE] + [shapes.IMPLICIT_CHEB] * 3
    for node, comp in zip(leaves, scene.leaves):
        if node.shape == shapes.IMPLICIT_CHEB:
            np.testing.assert_array_equal(node.lbox[:], np.asarray(comp.surface.get_bbox_local(), dtype=float))
            aux = np.ctypeslib.as_array(scene.aux)[node.aux: node.aux + implicit.HEADER]
            nx, ny, nz = aux[:3].astype(int)
            assert node.aux + implicit.HEADER + 4 * nx * ny * nz <= scene.n_aux
    assert sorted(scene.implicit) == [0, 2, 3, 4]
    back = type(scene).from_tables(scene.to_tables())
    assert bytes(back.nodes) == bytes(scene.nodes) and bytes(back.materials) == bytes(scene.materials)
    np.testing.assert_array_equal(np.ctypeslib.as_array(back.aux)[: back.n_aux], np.ctypeslib.as_array(scene.aux)[: scene.n_aux])


def test_header_enum_and_abi_version():
    header = open(os.path.join(ROOT, "include", "optable_hip.h")).read()
    assert int(re.search(r"OT_SHAPE_IMPLICIT_CHEB = (\d+)", header).group(1)) == shapes.IMPLICIT_CHEB == 11
    assert int(re.search(r"#define OT_IMPLICIT_HEADER (\d+)", header).group(1)) == implicit.HEADER
    assert int(re.search(r"#define OT_ABI_VERSION (\d+)", header).group(1)) == abi.ABI_VERSION == 14
    for name, value in (("BOX", implicit.APERTURE_BOX), ("DISC", implicit.APERTURE_DISC), ("RECT", implicit.APERTURE_RECT),
                        ("BALL", implicit.APERTURE_BALL)):
        assert int(re.search(rf"OT_APERTURE_{name} = (\d+)", header).group(1)) == value


def test_a_hole_finer_than_the_sampling_passes_the_measurement():
    """The run-time check of ray_tracing is what catches it (tests/test_gpu_implicit.py)."""
    m = implicit.measure(_holed(U)(10.0, 4.0, 1.5))
    assert m.aperture == implicit.APERTURE_DISC


def _holed(U):
    class Holed(U["Torus"]):
        """A disc aperture with a round hole of diameter 2 % of its radius, off the axis."""

        def within_boundary(self, P):
            return P[1] ** 2 + P[2] ** 2 <= self.a**2 and np.hypot(P[1] - 0.4, P[2] - 0.3) > 0.01 * self.a

    return Holed
